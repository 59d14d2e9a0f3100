"""Thermostats of ``ConstantVolume`` under the names and parameter keys of ``hoomd.md.methods.thermostats``:
``Berendsen(kT, tau)``, ``Bussi(kT, tau=0.0)`` and ``MTTK(kT, tau)``, as in
``ConstantVolume(filter=All(), thermostat=thermostats.Bussi(kT=1.0, tau=0.5))``. All three rescale the velocities of
all particles by one factor per step, so the total momentum keeps its direction and a zero momentum stays zero: a
canonical ensemble without the friction against a fixed frame that ``flow.Langevin`` adds.

HOOMD-blue's source is not available to this project: the scheme is defined in ``include/azp.h`` and ``DESIGN.md``
4.18 and runs in libazp (``csrc/thermostat.hip``). A thermostat acts once per step, at the start of step t, on the
full-step velocities v(t): from K = sum 1/2 m |v|^2, Nf = 3 N - 3 and its own state it computes a scale factor alpha
on the device, and step one does v <- alpha v ahead of the half kick. Nothing is read back inside ``run``.

``kT``: a positive float or a callable of the timestep (evaluated on the host at the step's timestep, as
``external.HarmonicBarrier.location``). ``energy`` (every thermostat) and ``MTTK.translational_dof`` can be read and
set between runs; reading synchronises. The state lives in a small device tensor owned by the thermostat and persists
across ``run`` calls: ``run(10); run(10)`` equals ``run(20)`` bit for bit.

``ConstantPressure(..., thermostat=...)`` takes the same objects: there the barostat's advance runs the thermostat's on this
state (``DESIGN.md`` 4.23). One thermostat object belongs to one method.

Out of scope: rotational degrees of freedom, ``Type`` filters, decomposed runs, Nose-Hoover chains longer than one, an
``_azplugins`` pybind class."""

import math
import weakref

from . import _lib
from .methods import _ControlState, _DeviceControlled, _bind_partials, _launch


class _Thermostat(_DeviceControlled):
    _name = None
    _kind = None
    _tau_may_be_zero = False

    def __init__(self, kT, tau):
        self.kT = kT
        self.tau = tau
        self._holders = weakref.WeakSet()  # the methods (ConstantVolume, ConstantPressure) that hold this thermostat
        self._control = _ControlState(self._name, [0.0] * _lib.THERMOSTAT_NSTATE)  # (AZP_THERMOSTAT_NSTATE doubles)
        self._partials = None
        self._ndof = 0.0     # Nf of the last run
        self._last_kT = 0.0  # kT of the last step run

    @property
    def kT(self):
        return self._kT

    @kT.setter
    def kT(self, kT):
        if not callable(kT):
            kT = float(kT)
            if not (math.isfinite(kT) and kT > 0.0):
                raise _lib.AzpError("%s: kT must be a positive float or a callable of the timestep, got %r" % (self._name, kT))
        self._kT = kT

    @property
    def tau(self):
        return self._tau

    @tau.setter
    def tau(self, tau):
        tau = float(tau)
        ok = math.isfinite(tau) and (tau >= 0.0 if self._tau_may_be_zero else tau > 0.0)
        if not ok:
            raise _lib.AzpError("%s: tau must be %s, got %r" % (self._name, ">= 0" if self._tau_may_be_zero else "> 0", tau))
        self._tau = tau

    def _kT_at(self, timestep):
        kT = float(self._kT(timestep)) if callable(self._kT) else self._kT
        if not (math.isfinite(kT) and kT > 0.0):
            raise _lib.AzpError("%s: kT must be > 0, got %r at timestep %d" % (self._name, kT, timestep))
        return kT

    # -- what a holder asks of its thermostat (ConstantVolume: the stepper below; ConstantPressure: in its advance) -------
    def _bind(self, sim):
        """Bind for this run: the seed warning (Bussi), Nf, and the state on the particles' device; returns its pointer."""
        if self._kind == _lib.THERMOSTAT_BUSSI:
            sim._warn_if_seed_unset()
        self._ndof = float(3 * sim.state.N - 3)
        return self._control.bind(sim.state.vel.device)

    def _open_step(self, timestep):
        """kT for the step that opens at ``timestep``, which becomes the kT of the last step run."""
        self._last_kT = self._kT_at(timestep)
        return self._last_kT

    # -- the stepper of a thermostatted ConstantVolume ---------------
    # The thermostat needs the kinetic energy of all particles between step two of one step and step one of the next,
    # so the two are never fused: step two leaves the partial sums of K behind, one wave turns them into the scale
    # factor alpha on the device, and step one reads alpha from there. Nothing is read back.
    _fusable = False
    _updaters_split = False

    def _begin(self, sim):
        """The refusals, the argument struct of this run, the state tensor and the partials buffer on the state's device,
        and K of the first step from a pass of its own (the velocities may have been changed between runs)."""
        integ, st = sim.operations.integrator, sim.state
        sim._check_thermostat(integ, integ.methods[0])
        a = self._args = _lib.ThermostatArgs()
        a.d_state = self._bind(sim)
        self._partials = _bind_partials(a, st, "azp_thermostat_partials_size", self._partials)
        a.dt = integ.dt
        a.tau = self._tau
        a.ndof = self._ndof
        a.seed = int(sim.seed or 0) & 0xFFFF
        a.kind = self._kind
        self._stream = _lib.raw_stream(st.device)
        _launch(a, st, self._stream, "azp_thermostat_kinetic")

    def _step_one(self, sim, timestep, fused):
        a = self._args
        a.timestep = timestep
        a.kT = self._open_step(timestep)
        _launch(a, sim.state, self._stream, "azp_thermostat_advance", "azp_thermostat_step_one")

    def _step_two(self, sim, timestep):
        _launch(self._args, sim.state, self._stream, "azp_thermostat_step_two")

    @property
    def energy(self):
        """The energy the thermostat has taken out of the particles: the running sum of K - alpha^2 K, so that
        K + U + ``energy`` is conserved up to the integrator's error."""
        return self._control.get(_lib.THERMOSTAT_ENERGY)[0]

    @energy.setter
    def energy(self, value):
        self._control.set(_lib.THERMOSTAT_ENERGY, [value], "energy")

    def __repr__(self):
        return "%s(kT=%r, tau=%r)" % (type(self).__name__, self._kT, self._tau)


class Berendsen(_Thermostat):
    """Weak coupling: alpha = sqrt(1 + (dt / tau) (Kbar / K - 1)), Kbar = Nf kT / 2. It relaxes K towards Kbar with the
    time constant ``tau`` but does not sample the canonical ensemble. ``tau`` > 0; ``tau`` < dt is rejected at ``run``
    (the radicand can turn negative)."""

    _name = "thermostats.Berendsen"
    _kind = _lib.THERMOSTAT_BERENDSEN


class Bussi(_Thermostat):
    """Stochastic velocity rescaling (Bussi, Donadio, Parrinello 2007): K is moved to K' = (sqrt(c K) + R1 sqrt((1 - c)
    kT / 2))^2 + (1 - c)(kT / 2) S with c = exp(-dt / tau), R1 standard normal and S chi-square with Nf - 1 degrees of
    freedom; alpha = sqrt(K' / K). Canonical. ``tau`` >= 0; ``tau`` = 0 (the default) draws K from its canonical
    distribution every step. The random numbers come from ``sim.seed`` and the timestep."""

    _name = "thermostats.Bussi"
    _kind = _lib.THERMOSTAT_BUSSI
    _tau_may_be_zero = True

    def __init__(self, kT, tau=0.0):
        super().__init__(kT, tau)


class MTTK(_Thermostat):
    """One Nose-Hoover degree of freedom (the equations of Martyna, Tobias, Tuckerman and Klein with a chain of one):
    xi' = g(K) = (2 K / (Nf kT) - 1) / tau^2, eta' = xi, v' = a - xi v, integrated per step as xi += (dt / 2) g(K),
    alpha = exp(-xi dt), eta += xi dt, xi += (dt / 2) g(alpha^2 K). Canonical and deterministic. ``tau`` > 0."""

    _name = "thermostats.MTTK"
    _kind = _lib.THERMOSTAT_MTTK

    @property
    def translational_dof(self):
        """(xi, eta): the thermostat's momentum and position."""
        return self._control.get(_lib.THERMOSTAT_XI, 2)

    @translational_dof.setter
    def translational_dof(self, value):
        xi, eta = value
        self._control.set(_lib.THERMOSTAT_XI, [xi, eta], "translational_dof")

    @property
    def energy(self):
        """Nf kT (tau^2 xi^2 / 2 + eta), which makes K + U + ``energy`` the conserved quantity of the equations, with
        Nf and kT of the last step run (0 before the first). It follows from ``translational_dof`` and cannot be set
        on its own."""
        xi, eta = self.translational_dof
        return (self._ndof * self._last_kT) * (0.5 * ((self._tau * self._tau) * (xi * xi)) + eta)

    @energy.setter
    def energy(self, value):
        raise _lib.AzpError("thermostats.MTTK: energy = Nf kT (tau^2 xi^2 / 2 + eta) follows from translational_dof; set that")


__all__ = ["Berendsen", "Bussi", "MTTK"]
