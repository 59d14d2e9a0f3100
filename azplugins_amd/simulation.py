"""Minimal simulation driver: the slice of ``hoomd.Simulation`` /
``hoomd.md.Integrator`` the reference's tests exercise -- attach forces to a
state, ``run(0)`` to evaluate them, and a velocity-Verlet NVE step
(``hoomd.md.methods.ConstantVolume``) so thermostatting pair forces can be
validated as in src/pytest/test_pair_dpd.py.
"""

import ctypes as C
import math
import warnings

import numpy as np

from . import _lib
from .state import State


class All:
    """``hoomd.filter.All``: every particle. The only filter the NVE kernels implement."""

    def __eq__(self, other):
        return isinstance(other, All)

    def __hash__(self):
        return hash("All")


class Type:
    """``hoomd.filter.Type``: the particles of the named types. ``types`` is one type name or an iterable of type
    names. Computes and the flow methods (``flow.Langevin``, ``flow.Brownian``) accept it; ``ConstantVolume``
    integrates all particles (``All`` only)."""

    def __init__(self, types):
        if isinstance(types, str):
            types = [types]
        self.types = tuple(types)
        if not all(isinstance(t, str) for t in self.types):
            raise _lib.AzpError("Type: type names must be strings, got %r" % (types,))

    def mask(self, type_names):
        """One byte per type of ``type_names`` (the state's types): 1 if the type is selected."""
        missing = [t for t in self.types if t not in type_names]
        if missing:
            raise _lib.AzpError("Type filter names %s, which the state does not have (types %s)" % (missing, list(type_names)))
        return np.array([1 if t in self.types else 0 for t in type_names], dtype=np.uint8)

    def __eq__(self, other):
        return isinstance(other, Type) and set(self.types) == set(other.types)

    def __hash__(self):
        return hash(("Type", frozenset(self.types)))

    def __repr__(self):
        return "Type(%r)" % (list(self.types),)


class Periodic:
    """``hoomd.trigger.Periodic``: fires at the timesteps t with ``(t - phase) % period == 0``."""

    def __init__(self, period, phase=0):
        if isinstance(period, bool) or int(period) != period or int(period) < 1:
            raise _lib.AzpError("Periodic: period must be a positive integer, got %r" % (period,))
        if isinstance(phase, bool) or int(phase) != phase:
            raise _lib.AzpError("Periodic: phase must be an integer, got %r" % (phase,))
        self.period, self.phase = int(period), int(phase)

    def __call__(self, timestep):
        return (int(timestep) - self.phase) % self.period == 0

    def __eq__(self, other):
        return isinstance(other, Periodic) and (other.period, other.phase) == (self.period, self.phase)

    def __hash__(self):
        return hash(("Periodic", self.period, self.phase))

    def __repr__(self):
        return "Periodic(period=%d, phase=%d)" % (self.period, self.phase)


def _launch(a, st, stream, *names):
    """Queue the libazp integration entries ``names`` with their argument struct ``a`` pointed at the state's arrays of
    this moment (they are replaced when particles migrate between ranks or are re-sorted), and at the state's box when
    ``box_generation`` has moved since the struct's box was written (``State.set_box``, ``update.BoxResize``)."""
    generation = getattr(st, "box_generation", 0)  # (a stand-in state without the counter keeps its box)
    if getattr(a, "_box_generation", None) != generation:
        a.box = st.box.to_c()
        a._box_generation = generation
    a.d_pos = st.pos.data_ptr()
    a.d_vel = st.vel.data_ptr()
    a.d_net_force = st.net_force.data_ptr()
    a.d_image = st.image.data_ptr()
    a.N = st.N
    lib = _lib.lib()
    for name in names:
        _lib.check(getattr(lib, name)(C.byref(a), stream), name)


class _DeviceControlled:
    """A stepper whose step is controlled on the device (the thermostats, ``minimize.FIRE``, ``ConstantPressure``, which
    sizes no partials: its sums are ``azp_thermo_sums``') and the buffers it owns: the
    control state, float64 doubles made at the first run, which persist across runs and follow the particles to their
    device, and the partials that its sums pass through."""

    _state = None
    _partials = None

    def _bind_control(self, a, st, start, size_entry):
        """Make the state from the list ``start`` (first run) or move it to the device of ``st``, size the partials with
        libazp's ``size_entry``, and point the argument struct ``a`` at both and at the box."""
        import torch

        dev = st.vel.device
        if self._state is None or self._state.device != dev:
            start = start if self._state is None else self._state.cpu().tolist()
            self._state = torch.tensor(start, dtype=torch.float64, device=dev)
        need = C.c_uint64(0)
        _lib.check(getattr(_lib.lib(), size_entry)(st.N, C.byref(need)), size_entry)
        if self._partials is None or self._partials.numel() * 8 < need.value or self._partials.device != dev:
            self._partials = torch.zeros(int(need.value) // 8, dtype=torch.float64, device=dev)
        a.d_partials = self._partials.data_ptr()
        a.partials_bytes = self._partials.numel() * 8
        a.d_state = self._state.data_ptr()
        a.box = st.box.to_c()


class ConstantVolume:
    """NVE integration method (velocity Verlet) on all particles
    (``hoomd.md.methods.ConstantVolume(filter=hoomd.filter.All())``; without a
    thermostat it is the dummy integrator of the reference's tests,
    src/pytest/test_pair.py:325-327). Any other filter is rejected: the kernels
    integrate all N particles.

    ``thermostat``: None (NVE, the fused kernels) or one of ``azplugins_amd.thermostats`` (``Berendsen``, ``Bussi``,
    ``MTTK``), which rescales the velocities of all particles once per step on the device. A
    thermostatted method integrates translational degrees of freedom of a single-domain run only; out of scope:
    rotational degrees of freedom, ``Type`` filters, decomposed runs, Nose-Hoover chains. Constant pressure:
    ``ConstantPressure``."""

    def __init__(self, filter=None, thermostat=None):
        if filter is not None and not isinstance(filter, All):
            raise _lib.AzpError("ConstantVolume: only filter=All() (or None) is supported, got %r" % (filter,))
        self.filter = All() if filter is None else filter
        self._thermostat = None
        self.thermostat = thermostat

    @property
    def thermostat(self):
        return self._thermostat

    @thermostat.setter
    def thermostat(self, thermostat):
        from .thermostats import _Thermostat

        if thermostat is not None and not isinstance(thermostat, _Thermostat):
            raise _lib.AzpError("ConstantVolume: thermostat must be None or one of azplugins_amd.thermostats, got %r" % (thermostat,))
        if self._thermostat is not None:
            self._thermostat._holders.discard(self)
        if thermostat is not None:
            thermostat._holders.add(self)
        self._thermostat = thermostat

    # -- the stepper of the NVE path; with a thermostat the thermostat steps --------
    _fusable = True
    _updaters_split = False  # (an updater changes types alone, which these kernels do not read)

    def _begin(self, sim):
        integ = sim.operations.integrator
        a = self._args = _lib.NVEArgs()
        a.box = sim.state.box.to_c()
        a.dt = integ.dt
        self._stream = _lib.raw_stream(sim.state.device)
        self._rot = None
        if integ.integrate_rotational_dof:
            if sim.domain is not None and not all(n in sim.domain.names for n in ("orientation", "angmom", "inertia")):
                raise _lib.AzpError("integrate_rotational_dof in a decomposed run: the domain must carry orientation, angmom "
                                    "and inertia (they migrate with the particles)")
            self._rot = _lib.NVERotArgs()
            self._rot.dt = integ.dt

    def _rotational_step(self, sim, one):
        st, rot, forces = sim.state, self._rot, sim.operations.integrator.forces
        torque = forces[0].torque_tensor  # the net torque, kept alive until the kernel is queued
        if len(forces) > 1:
            torque = torque.clone()
            for f in forces[1:]:
                torque += f.torque_tensor
        rot.d_orientation = st.orientation.data_ptr()
        rot.d_angmom = st.angmom.data_ptr()
        rot.d_inertia = st.inertia.data_ptr()
        rot.d_net_torque = torque.data_ptr()
        rot.N = st.N
        fn = _lib.lib().azp_integrate_nve_rot_step_one if one else _lib.lib().azp_integrate_nve_rot_step_two
        _lib.check(fn(C.byref(rot), self._stream), "azp_integrate_nve_rot_step")

    def _step_one(self, sim, timestep, fused):
        """Velocity Verlet (libazp kernels): v += a dt/2, x += v dt, wrap | forces | v += a dt/2; ``fused``: behind step
        two of the previous step, in one kernel."""
        _launch(self._args, sim.state, self._stream, "azp_integrate_nve_step_two_one" if fused else "azp_integrate_nve_step_one")
        if self._rot is not None:
            if fused:
                self._rotational_step(sim, False)  # (step two of the previous step: the torques are still its own)
            self._rotational_step(sim, True)

    def _step_two(self, sim, timestep):
        _launch(self._args, sim.state, self._stream, "azp_integrate_nve_step_two")
        if self._rot is not None:
            self._rotational_step(sim, False)


_AXES = ("x", "y", "z")


class ConstantPressure(_DeviceControlled):
    """``hoomd.md.methods.ConstantPressure`` on the three lengths of an orthorhombic box: a Martyna-Tobias-Klein barostat
    (NPH), with one of ``azplugins_amd.thermostats`` NPT. HOOMD-blue's source is not available to this project: the
    scheme is defined in ``include/azp.h`` and ``DESIGN.md`` 4.23 and runs in libazp (``csrc/barostat.hip``).

    ``S``: the target stress: a float (the pressure), a callable of the timestep (the ``variant`` classes included), or
    six values xx, yy, zz, yz, xz, xy whose last three are 0. ``tauS`` > 0: the barostat's time constant.
    ``couple``: ``"none"``, ``"xy"``, ``"xz"``, ``"yz"`` or ``"xyz"``: the coupled axes change at one rate.
    ``thermostat``: None or a ``Berendsen``, ``Bussi`` or ``MTTK``; it acts on the particles only, the box rates are not
    thermostatted. ``box_dof``: which of Lx, Ly, Lz (and, always False here, the tilts xz, yz, xy) are free.
    ``rescale_all`` has no effect (all particles are integrated), ``gamma`` must be 0.

    One rate nu_a per axis lives in a device-resident state that persists across runs: ``run(10); run(10)`` equals
    ``run(20)`` bit for bit. ``barostat_dof`` (the three nu), ``barostat_energy`` (W / 2 sum nu_a^2) and ``reference_kT``
    can be read between runs (reading synchronises); ``barostat_dof`` and ``reference_kT`` can be set. For hydrostatic S,
    K + U + S V + ``barostat_energy`` (+ the thermostat's ``energy``) is conserved up to the integrator's error. Without a
    thermostat the barostat's mass W = (Nf + 3) kT_ref tauS^2 takes kT_ref = 2 K / Nf from the first step of the first run.

    The box lives on the host: every step the host reads the three scale factors from the device (ONE HOST WAIT PER
    STEP) and sets the box through ``State.set_box``, so every neighbor list is rebuilt every step, as under an
    ``update.BoxResize`` that fires every step. While such a method is present the virial pass of every force runs
    every step (at most 8 forces).

    Refused: a filter other than ``All()``, rotational degrees of freedom, decomposed runs, tilted boxes, a free axis
    that is not periodic, tilt degrees of freedom, ``gamma`` != 0, fewer than 2 particles, a second method next to it."""

    _name = "ConstantPressure"
    _fusable = False
    _updaters_split = False

    def __init__(self, filter, S, tauS, couple, thermostat=None, box_dof=(True, True, True, False, False, False),
                 rescale_all=False, gamma=0.0):
        if filter is not None and not isinstance(filter, All):
            raise _lib.AzpError("ConstantPressure: only filter=All() is supported (the barostat scales every particle), got %r" % (filter,))
        self.filter = All() if filter is None else filter
        self.S = S
        tauS = float(tauS)
        if not (math.isfinite(tauS) and tauS > 0.0):
            raise _lib.AzpError("ConstantPressure: tauS must be > 0, got %r" % (tauS,))
        self.tauS = tauS
        if couple not in _lib.BAROSTAT_COUPLE:
            raise _lib.AzpError("ConstantPressure: couple must be one of %s, got %r" % (sorted(_lib.BAROSTAT_COUPLE), couple))
        self.couple = couple
        box_dof = tuple(bool(b) for b in box_dof)
        if len(box_dof) != 6:
            raise _lib.AzpError("ConstantPressure: box_dof takes six flags (Lx, Ly, Lz, xz, yz, xy), got %r" % (box_dof,))
        if any(box_dof[3:]):
            raise _lib.AzpError("ConstantPressure: tilt degrees of freedom are not supported (box_dof = %r): the box stays "
                                "orthorhombic" % (box_dof,))
        self.box_dof = box_dof
        if float(gamma) != 0.0:
            raise _lib.AzpError("ConstantPressure: gamma = %r: the Langevin piston is not supported, gamma must be 0" % (gamma,))
        self.gamma = 0.0
        self.rescale_all = bool(rescale_all)
        self._thermostat = None
        self.thermostat = thermostat
        self._pending = [0.0] * _lib.BAROSTAT_NSTATE
        self._row = None
        self._thermo = None
        self._first = True

    @property
    def S(self):
        return self._S

    @S.setter
    def S(self, S):
        if not callable(S):
            try:
                S = (float(S),) * 3 + (0.0,) * 3
            except TypeError:
                S = tuple(float(x) for x in S)
                if len(S) != 6:
                    raise _lib.AzpError("ConstantPressure: S is a float, a callable of the timestep or six values xx, yy, zz, "
                                        "yz, xz, xy; got %r" % (S,))
            if not all(math.isfinite(x) for x in S):
                raise _lib.AzpError("ConstantPressure: S must be finite, got %r" % (S,))
            if any(x != 0.0 for x in S[3:]):
                raise _lib.AzpError("ConstantPressure: shear stresses are not supported (S = %r): yz, xz and xy must be 0" % (S,))
        self._S = S

    def _S_at(self, timestep):
        """(S_xx, S_yy, S_zz) at ``timestep``."""
        if not callable(self._S):
            return self._S[:3]
        s = float(self._S(timestep))
        if not math.isfinite(s):
            raise _lib.AzpError("ConstantPressure: S must be finite, got %r at timestep %d" % (s, timestep))
        return (s, s, s)

    @property
    def thermostat(self):
        return self._thermostat

    @thermostat.setter
    def thermostat(self, thermostat):
        from .thermostats import _Thermostat

        if thermostat is not None and not isinstance(thermostat, _Thermostat):
            raise _lib.AzpError("ConstantPressure: thermostat must be None or one of azplugins_amd.thermostats, got %r" % (thermostat,))
        if self._thermostat is not None:
            self._thermostat._holders.discard(self)
        if thermostat is not None:
            thermostat._holders.add(self)
        self._thermostat = thermostat

    # -- device-resident state ---------------------------------------------------
    def _slots(self, k, n=1):
        """Slots k .. k + n - 1 of the state; reading synchronises."""
        if self._state is None:
            return tuple(self._pending[k:k + n])
        return tuple(self._state[k:k + n].tolist())

    def _set_slots(self, k, values, what):
        values = [float(v) for v in values]
        if not all(math.isfinite(v) for v in values):
            raise _lib.AzpError("ConstantPressure: %s must be finite, got %r" % (what, values))
        if self._state is None:
            self._pending[k:k + len(values)] = values
        else:
            import torch

            self._state[k:k + len(values)] = torch.tensor(values, dtype=torch.float64)

    @property
    def barostat_dof(self):
        """(nu_x, nu_y, nu_z): the rates of the three box lengths, d ln L_a / dt."""
        return self._slots(_lib.BAROSTAT_NU, 3)

    @barostat_dof.setter
    def barostat_dof(self, value):
        value = tuple(value)
        if len(value) != 3:
            raise _lib.AzpError("ConstantPressure: barostat_dof takes (nu_x, nu_y, nu_z), got %r" % (value,))
        self._set_slots(_lib.BAROSTAT_NU, value, "barostat_dof")

    @property
    def barostat_energy(self):
        """(W / 2)(nu_x^2 + nu_y^2 + nu_z^2) as of the last step run (0 before the first)."""
        return self._slots(_lib.BAROSTAT_ENERGY)[0]

    @property
    def reference_kT(self):
        """kT_ref of the barostat's mass W = (Nf + 3) kT_ref tauS^2 in a run without a thermostat: 2 K / Nf at the first
        step of the first run (0 before it), or what was set. With a thermostat its kT is used instead."""
        return self._slots(_lib.BAROSTAT_REF_KT)[0]

    @reference_kT.setter
    def reference_kT(self, value):
        if not float(value) >= 0.0:
            raise _lib.AzpError("ConstantPressure: reference_kT must be >= 0 (0: measure it at the next step), got %r" % (value,))
        self._set_slots(_lib.BAROSTAT_REF_KT, [value], "reference_kT")

    # -- the stepper -------------------------------------------
    def _check(self, sim, integ):
        """What ``ConstantPressure`` cannot do, each refused with its reason."""
        st = sim.state
        if len(integ.methods) != 1:
            raise _lib.AzpError("ConstantPressure must be the only method of the integrator (it scales every particle and the "
                                "box), got %r" % (integ.methods,))
        if not isinstance(self.filter, All):
            raise _lib.AzpError("ConstantPressure: only filter=All() is supported (the barostat scales every particle), got %r"
                                % (self.filter,))
        if integ.integrate_rotational_dof:
            raise _lib.AzpError("ConstantPressure: rotational degrees of freedom are not integrated (integrate_rotational_dof=True)")
        if sim.domain is not None:
            raise _lib.AzpError("ConstantPressure does not run decomposed (the domain's slabs are cut once, and the pressure "
                                "would need a collective every step)")
        if st.N < 2:
            raise _lib.AzpError("ConstantPressure: fewer than 2 particles leave no degree of freedom (Nf = 3 N - 3), N = %d" % st.N)
        box = st.box
        if box.is_triclinic:
            raise _lib.AzpError("ConstantPressure: %r is tilted: only orthorhombic boxes are supported" % (box,))
        for k in range(3):
            if self.box_dof[k] and not box.periodic[k]:
                raise _lib.AzpError("ConstantPressure: the box is not periodic along %s, which box_dof leaves free: a free axis "
                                    "must be periodic" % _AXES[k])
        if len(integ.forces) > _lib.THERMO_MAX_FORCES:
            raise _lib.AzpError("ConstantPressure sums the virials of at most %d forces, the integrator has %d"
                                % (_lib.THERMO_MAX_FORCES, len(integ.forces)))
        th = self._thermostat
        if th is not None:
            if th._kind == _lib.THERMOSTAT_BERENDSEN and th.tau < integ.dt:
                raise _lib.AzpError("%s: tau = %r is below dt = %r (the rescaling factor's radicand can turn negative)"
                                    % (th._name, th.tau, integ.dt))
            if any(m is not self for m in th._holders):
                raise _lib.AzpError("%s: one thermostat object is held by two methods (its state belongs to one run)" % th._name)

    def _begin(self, sim):
        import torch

        from .compute import ThermodynamicQuantities

        integ, st = sim.operations.integrator, sim.state
        self._check(sim, integ)
        dev = st.vel.device
        if self._state is None or self._state.device != dev:
            start = self._pending if self._state is None else self._state.cpu().tolist()
            self._state = torch.tensor(start, dtype=torch.float64, device=dev)
        if self._row is None or self._row.device != dev:
            self._row = torch.zeros(_lib.THERMO_NSUMS, dtype=torch.float64, device=dev)
        if self._thermo is None:
            self._thermo = ThermodynamicQuantities(All())  # (never in sim.operations.computes: its launch machinery alone)
        self._thermo._sim = sim
        a = self._args = _lib.BarostatArgs()
        a.d_state = self._state.data_ptr()
        a.d_sums = self._row.data_ptr()
        a.box = st.box.to_c()
        a.dt = integ.dt
        a.tauS = self.tauS
        a.ndof = float(3 * st.N - 3)
        a.couple = _lib.BAROSTAT_COUPLE[self.couple]
        a.box_dof = sum(1 << k for k in range(3) if self.box_dof[k])
        th = self._thermostat
        if th is not None:
            if th._kind == _lib.THERMOSTAT_BUSSI:
                sim._warn_if_seed_unset()
            if th._state is None or th._state.device != dev:
                start = th._pending if th._state is None else th._state.cpu().tolist()
                th._state = torch.tensor(start, dtype=torch.float64, device=dev)
            a.d_thermostat_state = th._state.data_ptr()
            a.thermostat_tau = th.tau
            a.thermostat_kind = th._kind
            a.thermostat_seed = int(sim.seed or 0) & 0xFFFF
            th._ndof = a.ndof
        self._stream = _lib.raw_stream(st.device)
        self._first = True  # (the first step opens from a sums pass of the state as it stands)

    def _advance(self, sim, timestep, phase):
        a = self._args
        a.S[:] = self._S_at(timestep)
        a.timestep = timestep
        a.phase = phase
        th = self._thermostat
        if th is not None:
            a.thermostat_kT = th._kT_at(timestep)
            if phase & _lib.BAROSTAT_OPEN:
                th._last_kT = a.thermostat_kT
        _launch(a, sim.state, self._stream, "azp_barostat_advance")

    def _step_one(self, sim, timestep, fused):
        from .state import Box

        st = sim.state
        if self._first:
            self._thermo._launch(self._row.data_ptr())
            self._first = False
        self._advance(sim, timestep, _lib.BAROSTAT_OPEN)
        # the one host read of the step: the box lives on the host
        host = self._state.tolist()
        if host[_lib.BAROSTAT_NONFINITE] != 0.0:
            raise _lib.AzpError("ConstantPressure: the barostat's state is not finite at timestep %d (nu = %r, K = %r, W = %r): "
                                "no kinetic energy to take reference_kT from, or the run has diverged"
                                % (timestep, host[_lib.BAROSTAT_NU:_lib.BAROSTAT_NU + 3], host[_lib.BAROSTAT_K], host[_lib.BAROSTAT_W]))
        lam = host[_lib.BAROSTAT_LAMBDA:_lib.BAROSTAT_LAMBDA + 3]
        box = st.box
        st.set_box(Box(lam[0] * box.Lx, lam[1] * box.Ly, lam[2] * box.Lz, periodic=box.periodic))
        _launch(self._args, st, self._stream, "azp_barostat_step_one")

    def _step_two(self, sim, timestep):
        _launch(self._args, sim.state, self._stream, "azp_barostat_step_two")
        self._thermo._launch(self._row.data_ptr())
        # (the close half belongs to the end of the step: S and kT of the timestep the next step opens at. Always a
        # launch of its own, at the end of a run too: run(a); run(b) is run(a + b) bit for bit)
        self._advance(sim, timestep + 1, _lib.BAROSTAT_CLOSE)

    def __repr__(self):
        return "ConstantPressure(S=%r, tauS=%r, couple=%r, thermostat=%r)" % (self._S, self.tauS, self.couple, self._thermostat)


class Integrator:
    """``hoomd.md.Integrator`` reduced: ``dt``, ``forces``, ``methods``,
    ``integrate_rotational_dof`` (orientations and angular momenta of particles with a
    non-zero moment of inertia are integrated with the net torque, HOOMD's default False).
    ``methods`` holds one ``ConstantVolume``, one ``ConstantPressure``, or one or more ``flow.Langevin`` /
    ``flow.Brownian`` with pairwise-disjoint filters (an ``All()`` filter stands alone)."""

    def __init__(self, dt, forces=None, methods=None, integrate_rotational_dof=False):
        self.dt = float(dt)
        self.forces = list(forces) if forces is not None else []
        self.methods = list(methods) if methods is not None else []
        self.integrate_rotational_dof = bool(integrate_rotational_dof)


class _Computes(list):
    """``sim.operations.computes``: a list whose members know their simulation (HOOMD attaches an operation when it
    joins the simulation's operations)."""

    def __init__(self, sim):
        super().__init__()
        self._sim = sim

    def _claim(self, op):
        from .compute import _Compute

        if not isinstance(op, _Compute):
            raise _lib.AzpError("sim.operations.computes holds computes (azplugins_amd.compute), got %r" % (op,))
        if op._sim is not None and op._sim is not self._sim and any(c is op for c in op._sim.operations.computes):
            raise _lib.AzpError("%s is already in the operations of another simulation" % type(op).__name__)
        op._sim = self._sim
        return op

    def append(self, op):
        if not any(c is op for c in self):
            super().append(self._claim(op))

    def insert(self, i, op):
        if not any(c is op for c in self):
            super().insert(i, self._claim(op))

    def extend(self, ops):
        for op in ops:
            self.append(op)

    def __iadd__(self, ops):
        self.extend(ops)
        return self

    def remove(self, op):
        for i, c in enumerate(self):
            if c is op:
                del self[i]
                op._sim = None
                return
        raise ValueError("%r is not in sim.operations.computes" % (op,))


class _Operations:
    def __init__(self, sim=None):
        self.integrator = None
        self.computes = _Computes(sim)
        # HOOMD's sim.operations.updaters: run ahead of the integrator's step at the timesteps their trigger fires
        # (azplugins_amd.update.TypeUpdater, azplugins_amd.evaporate.ParticleEvaporator)
        self.updaters = []
        # HOOMD's sim.operations.writers: run after the integrator's step at the timesteps their trigger fires
        # (azplugins_amd.compute.ThermodynamicRecorder, azplugins_amd.compute.RDFRecorder)
        self.writers = []
        # HOOMD puts a ParticleSorter into sim.operations.tuners by default; so does this
        # (remove it from the list, or set trigger_period = 0, to keep the initial order)
        from .sorter import ParticleSorter

        self.tuners = [ParticleSorter(trigger_period=200)]

    def add(self, op):
        """Add an updater, a writer or a compute (``hoomd.Operations.add``); a compute is attached while the simulation
        has a state."""
        from .compute import _Recorder
        from .update import _Updater

        for cls, ops in ((_Updater, self.updaters), (_Recorder, self.writers)):
            if isinstance(op, cls):
                if not any(u is op for u in ops):
                    ops.append(op)
                return
        self.computes.append(op)

    def remove(self, op):
        """Remove an updater, a writer or a compute; reading a removed compute's results raises
        ``compute.DataAccessError``."""
        from .compute import _Recorder
        from .update import _Updater

        for cls, ops, name in ((_Updater, self.updaters, "updaters"), (_Recorder, self.writers, "writers")):
            if isinstance(op, cls):
                for i, u in enumerate(ops):
                    if u is op:
                        del ops[i]
                        return
                raise ValueError("%r is not in sim.operations.%s" % (op, name))
        self.computes.remove(op)


class Simulation:
    def __init__(self, device="cuda:0", seed=None):
        self.device = device
        self.seed = seed
        self.state = None
        self.timestep = 0
        self.operations = _Operations(self)
        self._attached = []
        self.domain = None  # azplugins_amd.domain.DeviceDomain of a decomposed run (attach_domain)

    def attach_domain(self, domain):
        """Domain-decomposed run: ``domain`` (a rebuilt ``DeviceDomain``) owns the particle
        arrays. Every step the ghost rows of the arrays the forces read are exchanged; when
        any rank's distance check asks for a neighbor-list rebuild, all ranks migrate their
        particles and re-select their ghosts first (HOOMD: Communicator::migrateParticles /
        exchangeGhosts ahead of NeighborList::compute). A tilted box is refused: the domain's slabs are Cartesian."""
        if self.state.box.is_triclinic:
            raise _lib.AzpError("attach_domain: %r is tilted -- a domain cuts the box into Cartesian slabs, whose ghost layers "
                                "do not follow a tilted periodic face; run a tilted box on one device" % (self.state.box,))
        for kind, g in self.state.groups.items():
            if g.n and g.tags is None:
                raise _lib.AzpError("attach_domain: a %s needs its topology by tag (State.set_global_%ss) -- the index-based "
                                    "%s table of a single-domain state does not survive a migration"
                                    % ("bonded system" if kind == "bond" else "system with %ss" % kind, kind, kind))
        # every per-particle array that the integrator or a force touches must migrate with the particles
        # (an array left behind keeps its old size and order while N changes under it)
        need = ["pos", "vel", "tag", "image"]
        integ = self.operations.integrator
        if integ is not None:
            for f in integ.forces:
                need += [n for n in getattr(f, "_halo_fields", ()) if n not in need]
            if getattr(integ, "integrate_rotational_dof", False):
                need += ["orientation", "angmom", "inertia"]
        missing = [n for n in need if n not in domain.names]
        if missing:
            raise _lib.AzpError("attach_domain: the domain does not carry %s (DeviceDomain(arrays=...) must hold every array "
                                "the integrator and the forces use)" % ", ".join(missing))
        self.domain = domain
        domain.attach_state(self.state)
        self.operations.tuners.clear()  # the domain keeps its own interior | boundary | ghost order

    def _halo_fields(self):
        names = ["pos"]
        for f in self.operations.integrator.forces:
            for n in getattr(f, "_halo_fields", ()):
                if n not in names and n in self.domain.names:
                    names.append(n)
        return names

    def _wire_domain(self):
        """Point the neighbor lists of the attached forces at the domain's collective hooks."""
        dom = self.domain

        def before_rebuild(state):
            dom.rebuild()
            dom.attach_state(state)

        for f in self.operations.integrator.forces:
            nl = getattr(f, "nlist", None)
            if nl is not None:
                nl.reduce_flag = dom.all_reduce_flag
                nl.before_rebuild = before_rebuild

    def _warn_if_seed_unset(self):
        if self.seed is None:
            warnings.warn("Simulation.seed is not set, using default seed=0", RuntimeWarning)
            self.seed = 0

    def create_state_from_snapshot(self, snapshot):
        self.state = State(snapshot, self.device)
        return self.state

    @property
    def dt(self):
        integ = self.operations.integrator
        return integ.dt if integ is not None else 0.0

    def _attach_all(self):
        integ = self.operations.integrator
        if integ is None:
            raise _lib.AzpError("Simulation.operations.integrator is not set")
        if self.state is None:
            raise _lib.AzpError("Simulation has no state; call create_state_from_snapshot first")
        for f in integ.forces:
            if f not in self._attached or f._state is not self.state:
                f._attach(self)
                if f not in self._attached:
                    self._attached.append(f)
        if self._has_thermo() or self._barostat(integ) is not None:
            # (a ThermodynamicQuantities and a ConstantPressure read the per-particle virials: the virial pass of every
            # force runs every step)
            for f in integ.forces:
                f.compute_virial = True
            for c in self._thermo_computes():
                c._prepare()

    def _thermo_computes(self):
        from .compute import ThermodynamicQuantities

        return [c for c in self.operations.computes if isinstance(c, ThermodynamicQuantities)]

    @staticmethod
    def _barostat(integ):
        """The first ``ConstantPressure`` among the integrator's methods, or None."""
        return next((m for m in integ.methods if isinstance(m, ConstantPressure)), None)

    def _has_thermo(self):
        return bool(self.operations.computes) and bool(self._thermo_computes())

    def _check_writers(self):
        """A recorder reads its compute through this simulation's state: the compute has to be in ``computes``."""
        for w in self.operations.writers:
            if not any(c is w._compute for c in self.operations.computes):
                raise _lib.AzpError("%s: its %s is not in sim.operations.computes of this simulation"
                                    % (type(w).__name__, type(w._compute).__name__))
        integ = self.operations.integrator
        if integ is not None and len(integ.forces) > _lib.THERMO_MAX_FORCES and self._has_thermo():
            raise _lib.AzpError("ThermodynamicQuantities sums at most %d forces, the integrator has %d"
                                % (_lib.THERMO_MAX_FORCES, len(integ.forces)))

    def _writers_due(self):
        return [w for w in self.operations.writers if w.trigger(self.timestep)]

    def _run_writers(self, due):
        for w in due:
            w._record(self, self.timestep)

    def _compute_forces(self):
        import torch

        st = self.state
        forces = self.operations.integrator.forces
        if self.domain is not None:
            # decomposed runs: a neighbor-list rebuild migrates particles (N and every index change). Bring every list
            # up to date BEFORE any force buffer is sized or summed, so that all forces of this step see one order
            seen = []
            for f in forces:
                nl = getattr(f, "nlist", None)
                if nl is not None and all(nl is not s for s in seen):
                    seen.append(nl)
                    nl.compute(st)
            if len(seen) > 1:
                raise _lib.AzpError("decomposed runs support one neighbor list (a second list's rebuild would migrate "
                                    "particles under the first)")
        if len(forces) == 1:
            # a single force: its own array is the net force (no 32 MB zero + add per step)
            forces[0].compute(self.timestep)
            forces[0]._virial_evaluated = bool(forces[0].compute_virial)
            st.net_force = forces[0].force_tensor
            return
        if st.net_force.shape[0] != st.N or any(st.net_force is f.force_tensor for f in forces):
            st.net_force = torch.zeros((st.N, 4), dtype=torch.float64, device=st.device)
        for f in forces:
            f.compute(self.timestep)
            f._virial_evaluated = bool(f.compute_virial)
        # one pass over the forces' arrays (azp_sum_forces) instead of a zero + one read-modify-write per force
        for k0 in range(0, len(forces), 7):
            grp = forces[k0:k0 + 7]
            ptrs = ([st.net_force.data_ptr()] if k0 else []) + [f.force_tensor.data_ptr() for f in grp]
            arr = (C.c_void_p * len(ptrs))(*ptrs)
            _lib.check(_lib.lib().azp_sum_forces(st.N, len(ptrs), arr, st.net_force.data_ptr(), _lib.raw_stream(st.device)), "azp_sum_forces")

    def run(self, steps):
        """``steps`` steps of the integrator's methods (HOOMD IntegratorTwoStep::update): every stepper's step one at the
        step's timestep t, the forces at t + 1, every stepper's step two at t. The one loop of all paths."""
        from .minimize import FIRE

        self._check_writers()
        self._attach_all()
        integ = self.operations.integrator
        st = self.state
        # (refused even where nothing is stepped, and ahead of the forces: what the minimizer and the flow methods cannot do)
        fire = isinstance(integ, FIRE)
        if fire:
            integ._check(self)
        barostat = None if fire else self._barostat(integ)
        if barostat is not None:
            barostat._check(self, integ)
        flow_methods = [] if fire else self._check_flow_methods(integ)
        if self.domain is not None:
            self._wire_domain()
        self._compute_forces()
        if steps == 0 or not integ.methods:
            return
        # what moves the particles, each with the stepper interface: the minimizer, the flow methods, or
        # a ConstantPressure, or the one ConstantVolume (its thermostat where it has one)
        if fire:
            steppers = [integ]
        elif flow_methods:
            steppers = flow_methods
        elif barostat is not None:
            steppers = [barostat]
        elif len(integ.methods) != 1 or not isinstance(integ.methods[0], ConstantVolume):
            raise _lib.AzpError("Integrator.methods must hold exactly one ConstantVolume (all particles); got %r" % (integ.methods,))
        else:
            steppers = [integ.methods[0].thermostat or integ.methods[0]]
        for s in steppers:
            s._begin(self)
        # Inside a run nothing reads the velocities between step two of one step and step one of the next: where the
        # stepper can (_fusable) they are one kernel (same arithmetic, one pass over the arrays). Where a writer is due,
        # the full-step velocities of the previous step have to exist: its step two runs on its own (the same arithmetic,
        # bit for bit), the writer records, and this step starts with a plain step one. An updater that changes types
        # splits the fusion only for kernels that read them (_updaters_split: a flow method filtered by type); one that
        # changes the box (update.BoxResize) splits nothing: its kernel is queued ahead of the fused one, which reads the
        # box in its wrap alone, after step two's half kick
        fusable, updaters_split = steppers[0]._fusable, steppers[0]._updaters_split
        # (a bond force examines the "evaluator rejected its parameters" flag of step k when step k + 1 is queued, and
        # once more after the loop: no host round trip behind every launch)
        deferred = [f for f in integ.forces if hasattr(f, "defer_flag_check")]
        try:
            for f in deferred:
                f.defer_flag_check = True
            for k in range(steps):
                writers = self._writers_due() if k else []
                updaters = self._updaters_due()
                split = k > 0 and bool(not fusable or writers or (updaters_split and any(u._changes_types for u in updaters)))
                if split:
                    for s in steppers:
                        s._step_two(self, self.timestep - 1)
                self._run_writers(writers)  # (the state after self.timestep complete steps)
                self._run_updaters(updaters)
                for s in steppers:
                    s._step_one(self, self.timestep, fused=k > 0 and not split)
                if self.domain is not None:
                    self.domain.exchange(self._halo_fields())  # ghost rows follow their owners' particles
                st.position_generation += 1
                self.timestep += 1
                # re-index the particles between the position update and the force
                # evaluation: every per-particle array that survives the step is permuted,
                # the forces are recomputed in the new order
                # (also when a tile plan could not be compiled from the cells because the members of some tile have drifted
                # apart -- a DPD fluid diffuses a cell width in ~200 steps: sorting now costs 0.5 ms, the list-based rebuilds
                # that would follow until the sorter's next period 2.5 ms each; at most once per 20 steps)
                self._run_tuners(integ)
                self._compute_forces()
            for s in steppers:
                s._step_two(self, self.timestep - 1)
            self._run_writers(self._writers_due())
        finally:
            for f in deferred:
                f.defer_flag_check = False
        for f in deferred:
            f.check_flags(wait=True)

    def _check_thermostat(self, integ, method):
        """What a thermostatted ``ConstantVolume`` cannot do, each refused with its reason."""
        th = method.thermostat
        if not isinstance(method.filter, All):
            raise _lib.AzpError("%s: a thermostat needs filter=All() (it rescales with the kinetic energy of all particles), "
                                "got %r" % (th._name, method.filter))
        if integ.integrate_rotational_dof:
            raise _lib.AzpError("%s: rotational degrees of freedom are not thermostatted (integrate_rotational_dof=True)" % th._name)
        if self.domain is not None:
            raise _lib.AzpError("%s does not run decomposed (the kinetic energy would need a collective every step)" % th._name)
        if self.state.N < 2:
            raise _lib.AzpError("%s: fewer than 2 particles leave no degree of freedom (Nf = 3 N - 3), N = %d" % (th._name, self.state.N))
        if th._kind == _lib.THERMOSTAT_BERENDSEN and th.tau < integ.dt:
            raise _lib.AzpError("%s: tau = %r is below dt = %r (the rescaling factor's radicand can turn negative)"
                                % (th._name, th.tau, integ.dt))
        if any(m is not method for m in th._holders):
            raise _lib.AzpError("%s: one thermostat object is held by two methods (its state belongs to one run)" % th._name)

    def _updaters_due(self):
        return [u for u in self.operations.updaters if u.trigger(self.timestep)]

    def _run_updaters(self, due):
        """The updaters whose trigger fires at this timestep (HOOMD runs its updaters ahead of the integrator's
        step). Where one of them changes particle types (``_Updater._changes_types``), every neighbor list and tile plan
        is rebuilt before the next force evaluation (the reference: notifyParticleSort(), src/TypeUpdater.cc:86-87) --
        whether or not a type really changed, so that nothing is read back from the device."""
        for u in due:
            u._update(self, self.timestep)
        # (an updater that leaves the types alone -- update.BoxResize -- answers for its own generation counters)
        if any(u._changes_types for u in due):
            self.state.type_generation += 1

    def _run_tuners(self, integ):
        lists = [f.nlist for f in integ.forces if getattr(f, "nlist", None) is not None]
        wanted = any(nl.sort_wanted for nl in lists)
        for tuner in self.operations.tuners:
            due = tuner.trigger_period > 0 and self.timestep % tuner.trigger_period == 0
            on_demand = (wanted and tuner.trigger_period > 0
                         and (tuner.last_sort_step is None or self.timestep - tuner.last_sort_step >= 20))
            if (due or on_demand) and self.state.n_ghost == 0:
                tuner.sort(self)
                tuner.last_sort_step = self.timestep
                for nl in lists:
                    nl.particles_sorted()

    def _check_flow_methods(self, integ):
        """The flow methods of ``integ`` (empty if it has none), after checking that they can run together."""
        from .flow import _FlowMethod

        flow_methods = [m for m in integ.methods if isinstance(m, _FlowMethod)]
        if not flow_methods:
            return flow_methods
        if len(flow_methods) != len(integ.methods):
            raise _lib.AzpError("Integrator.methods: flow.Langevin / flow.Brownian cannot be mixed with other methods, got %r"
                                % (integ.methods,))
        if integ.integrate_rotational_dof:
            raise _lib.AzpError("flow.Langevin / flow.Brownian do not integrate rotational degrees of freedom "
                                "(integrate_rotational_dof=True)")
        if self.domain is not None:
            raise _lib.AzpError("flow.Langevin / flow.Brownian do not run decomposed (their accelerations do not migrate)")
        if any(any(m is o for o in flow_methods[:k]) for k, m in enumerate(flow_methods)):
            raise _lib.AzpError("Integrator.methods holds the same flow method twice")
        if len(flow_methods) > 1 and any(isinstance(m.filter, All) for m in flow_methods):
            raise _lib.AzpError("Integrator.methods: a flow method with filter All() must be the only method")
        seen = set()
        for m in flow_methods:
            if isinstance(m.filter, All):
                continue
            m.filter.mask(self.state.types)  # (rejects type names the state does not have)
            overlap = seen & set(m.filter.types)
            if overlap:
                raise _lib.AzpError("Integrator.methods: the filters of the flow methods overlap (types %s)" % sorted(overlap))
            seen |= set(m.filter.types)
        return flow_methods

    def kinetic_temperature(self):
        """Instantaneous kT = 2 KE / (3 N - 3) (HOOMD ThermodynamicQuantities)."""
        st = self.state
        v = st.vel[: st.N]
        ke = 0.5 * float((v[:, 3] * (v[:, :3] ** 2).sum(dim=1)).sum().item())
        return 2.0 * ke / (3 * st.N - 3)

    def rotational_kinetic_energy(self):
        """sum_k s_k^2 / (2 I_k) over the axes with I_k != 0, s = 1/2 conj(q) p the body-frame
        angular momentum (HOOMD ComputeThermo)."""
        import torch

        st = self.state
        q, p, I = st.orientation[: st.N], st.angmom[: st.N], st.inertia[: st.N]
        qs, qv = q[:, 0:1], q[:, 1:4]
        ps, pv = p[:, 0:1], p[:, 1:4]
        s_v = 0.5 * (qs * pv - ps * qv - torch.linalg.cross(qv, pv))  # vector part of conj(q) p / 2
        ke = torch.where(I != 0.0, s_v * s_v / torch.where(I != 0.0, I, torch.ones_like(I)), torch.zeros_like(I))
        return 0.5 * float(ke.sum().item())

    def thermalize_particle_momenta(self, kT, seed=12345):
        """Maxwell-Boltzmann velocities with zero total momentum."""
        import torch

        from .synthetic import normal

        st = self.state
        tag = np.arange(st.N, dtype=np.uint64)
        m = st.vel[: st.N, 3].cpu().numpy()
        v = np.stack([normal(seed, tag, c) for c in range(3)], axis=1) * np.sqrt(kT / m)[:, None]
        v -= (v * m[:, None]).sum(axis=0) / m.sum()
        st.vel[: st.N, :3] = torch.from_numpy(v).to(st.device)
