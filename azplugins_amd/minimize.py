"""Energy minimization under the name and parameter keys of ``hoomd.md.minimize.FIRE``: an ``Integrator`` that relaxes a
built configuration (stretched bonds, bent angles, near-overlaps) to a local minimum of the potential energy, as in

    fire = minimize.FIRE(dt=0.005, force_tol=1e-3, angmom_tol=1e-3, energy_tol=1e-7, forces=[...],
                         methods=[ConstantVolume(All())])
    sim.operations.integrator = fire
    while not fire.converged:
        sim.run(100)

HOOMD-blue's source is not available to this project: the scheme is defined in ``include/azp.h`` and ``DESIGN.md`` 4.19
and runs in libazp (``csrc/fire.hip``). FIRE (Bitzek, Koskinen, Gaehler, Moseler, Gumbsch 2006) is velocity Verlet in
which, ahead of every step one, the velocities are steered towards the force, v <- (1 - alpha) v + alpha |v| / |f| f.
While the power P = f . v stays positive for more than ``min_steps_adapt`` steps the time step grows by ``finc_dt`` (up to
``dt``) and alpha shrinks by ``fdec_alpha``; when P <= 0 the velocities are dropped, the time step shrinks by ``fdec_dt``
and alpha returns to ``alpha_start``. The time step has no floor: a system that never gains power (a force that is not
the gradient of the energy) halves it without end. Masses do not enter P, |v| and |f|, as in HOOMD.

The run has converged once, after at least ``max(1, min_steps_conv)`` steps, sqrt(sum |f|^2 / (3 N)) < ``force_tol`` and
the energy per particle changed by less than ``energy_tol`` in the last step. From then on ``run`` moves nothing (the
kernels return at once) but still counts timesteps.

The control state, the time step included, is a small float64 device tensor owned by the ``FIRE`` object, made at the first
run. Nothing is read back inside ``run``; ``converged``, ``energy`` and ``force_rms`` read it and synchronise. It persists
across ``run`` calls: ``run(a); run(b)`` equals ``run(a + b)`` bit for bit.

Out of scope: rotational degrees of freedom (``angmom_tol`` is stored and unused), ``Type`` filters, decomposed runs,
``DisplacementCapped``, box relaxation (``ConstantPressure``), an ``_azplugins`` pybind class."""

import math
import weakref

from . import _lib
from .filter import All
from .methods import ConstantVolume, _ControlState, _DeviceControlled, _bind_partials, _launch
from .simulation import Integrator


def _positive(name, value):
    value = float(value)
    if not (math.isfinite(value) and value > 0.0):
        raise _lib.AzpError("minimize.FIRE: %s must be a finite float > 0, got %r" % (name, value))
    return value


def _in_unit_interval(name, value):
    value = float(value)
    if not (math.isfinite(value) and 0.0 < value < 1.0):
        raise _lib.AzpError("minimize.FIRE: %s must be in (0, 1), got %r" % (name, value))
    return value


def _count(name, value):
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(value) or int(value) != value or value < 0:
        raise _lib.AzpError("minimize.FIRE: %s must be an integer >= 0, got %r" % (name, value))
    if int(value) > 0xFFFFFFFF:
        raise _lib.AzpError("minimize.FIRE: %s must fit 32 bits, got %r" % (name, value))
    return int(value)


class FIRE(Integrator, _DeviceControlled):
    """``hoomd.md.minimize.FIRE`` reduced to translational degrees of freedom of all particles of a single-domain run.

    ``dt``: the largest time step, and the one the minimization starts from (``sim.dt`` keeps returning it; the step in
    use lives on the device). ``methods`` must hold exactly one ``ConstantVolume(All())`` without a thermostat; anything
    else, ``integrate_rotational_dof=True``, a decomposed run and an empty state are refused at ``run``."""

    def __init__(self, dt, force_tol, angmom_tol, energy_tol, integrate_rotational_dof=False, forces=None, methods=None,
                 min_steps_adapt=5, finc_dt=1.1, fdec_dt=0.5, alpha_start=0.1, fdec_alpha=0.99, min_steps_conv=10):
        super().__init__(_positive("dt", dt), forces=forces, methods=methods, integrate_rotational_dof=integrate_rotational_dof)
        self.force_tol = _positive("force_tol", force_tol)
        self.angmom_tol = _positive("angmom_tol", angmom_tol)  # (stored: rotational degrees of freedom are out of scope)
        self.energy_tol = _positive("energy_tol", energy_tol)
        self.finc_dt = float(finc_dt)
        if not (math.isfinite(self.finc_dt) and self.finc_dt > 1.0):
            raise _lib.AzpError("minimize.FIRE: finc_dt must be a finite float > 1, got %r" % (finc_dt,))
        self.fdec_dt = _in_unit_interval("fdec_dt", fdec_dt)
        self.alpha_start = _in_unit_interval("alpha_start", alpha_start)
        self.fdec_alpha = _in_unit_interval("fdec_alpha", fdec_alpha)
        self.min_steps_adapt = _count("min_steps_adapt", min_steps_adapt)
        self.min_steps_conv = _count("min_steps_conv", min_steps_conv)
        self._control = _ControlState("minimize.FIRE", self._initial())
        self._partials = None
        self._n = 0            # N of the last run
        self._sim = None       # (weak) the simulation of the last run

    def _initial(self):
        """What the control state (AZP_FIRE_NSTATE doubles) starts from."""
        start = [0.0] * _lib.FIRE_NSTATE
        start[_lib.FIRE_DT] = self.dt
        start[_lib.FIRE_ALPHA] = self.alpha_start
        start[_lib.FIRE_KEEP] = 1.0
        return start

    # -- the driver's side -----------------------------------------------------
    def _check(self, sim):
        """What the minimizer cannot do, each refused with its reason."""
        if self.integrate_rotational_dof:
            raise _lib.AzpError("minimize.FIRE: rotational degrees of freedom are not minimized (integrate_rotational_dof=True)")
        m = self.methods[0] if len(self.methods) == 1 else None
        if not isinstance(m, ConstantVolume) or not isinstance(m.filter, All) or m.thermostat is not None:
            raise _lib.AzpError("minimize.FIRE: methods must hold exactly one ConstantVolume(All()) without a thermostat (the "
                                "minimizer moves all particles and sets their velocities itself), got %r" % (self.methods,))
        if sim.domain is not None:
            raise _lib.AzpError("minimize.FIRE does not run decomposed (its four sums would need a collective every step)")
        if sim.state.N == 0:
            raise _lib.AzpError("minimize.FIRE: the state holds no particles (N = 0)")

    # The stepper: the thermostatted step's shape with a control state that holds the time step itself.
    # Step two leaves the partials of P = f . v, |v|^2, |f|^2 and U behind, one wave turns them into the next step's time
    # step and velocity coefficients on the device, and step one reads them from there. Nothing is read back: once the
    # state says converged the kernels return at once, and the loop only counts.
    _fusable = False
    _updaters_split = False

    def _begin(self, sim):
        """The argument struct of this run, the state tensor and the partials buffer on the state's device, and the sums
        of the first step from a pass of their own: the velocities may have been changed between runs (after a run that
        ended with step two it leaves the partials that step two left, bit for bit)."""
        st = sim.state
        a = self._args = _lib.FireArgs()
        if self._state is None:
            self._control.reset(self._initial())  # (dt and alpha_start as they are at the first run)
        a.d_state = self._control.bind(st.vel.device)
        self._partials = _bind_partials(a, st, "azp_fire_partials_size", self._partials)
        a.dt_max, a.force_tol, a.energy_tol = self.dt, self.force_tol, self.energy_tol
        a.finc_dt, a.fdec_dt, a.alpha_start, a.fdec_alpha = self.finc_dt, self.fdec_dt, self.alpha_start, self.fdec_alpha
        a.min_steps_adapt, a.min_steps_conv = self.min_steps_adapt, self.min_steps_conv
        self._n = st.N
        self._sim = weakref.ref(sim)
        self._stream = _lib.raw_stream(st.device)
        _launch(a, st, self._stream, "azp_fire_measure")

    def _step_one(self, sim, timestep, fused):
        _launch(self._args, sim.state, self._stream, "azp_fire_advance", "azp_fire_step_one")

    def _step_two(self, sim, timestep):
        _launch(self._args, sim.state, self._stream, "azp_fire_step_two")

    # -- results ----------------------------------------------------------------
    def _read(self):
        """The state on the host (synchronises), refusing a minimization whose sums became non-finite."""
        s = self._control.host()
        if s[_lib.FIRE_NONFINITE] != 0.0:
            raise _lib.AzpError("minimize.FIRE: forces or velocities became non-finite (overlapping particles, or a time step "
                                "too large for the stiffest force); nothing was moved from that step on")
        return s

    @property
    def converged(self):
        """True once both tolerances were met. Reads the device state and synchronises; False before the first run."""
        if self._state is None:
            return False
        return self._read()[_lib.FIRE_CONVERGED] != 0.0

    @property
    def energy(self):
        """The potential energy per particle, U / N, as the last advance saw it (0.0 before the first run)."""
        if self._state is None:
            return 0.0
        return self._read()[_lib.FIRE_U] / self._n

    @property
    def force_rms(self):
        """sqrt(sum |f|^2 / (3 N)) as the last advance saw it: the quantity ``force_tol`` is compared with."""
        if self._state is None:
            return 0.0
        return math.sqrt(self._read()[_lib.FIRE_FF] / (3.0 * self._n))

    def reset(self):
        """Back to the initial control state (time step ``dt``, alpha ``alpha_start``, not converged); the velocities of
        the attached state are zeroed, the masses in ``vel.w`` stay."""
        self._control.reset(self._initial())
        sim = self._sim() if self._sim is not None else None
        if sim is not None and sim.state is not None:
            sim.state.vel[:, :3] = 0.0

    def __repr__(self):
        return ("FIRE(dt=%r, force_tol=%r, angmom_tol=%r, energy_tol=%r, min_steps_adapt=%r, finc_dt=%r, fdec_dt=%r, alpha_start=%r, "
                "fdec_alpha=%r, min_steps_conv=%r)" % (self.dt, self.force_tol, self.angmom_tol, self.energy_tol, self.min_steps_adapt,
                                                       self.finc_dt, self.fdec_dt, self.alpha_start, self.fdec_alpha, self.min_steps_conv))


__all__ = ["FIRE"]
