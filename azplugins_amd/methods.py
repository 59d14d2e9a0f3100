"""Integration methods under the names of ``hoomd.md.methods``: ``ConstantVolume`` (velocity Verlet; with one of
``azplugins_amd.thermostats`` NVT), ``ConstantPressure`` (a Martyna-Tobias-Klein barostat), ``Langevin`` and ``Brownian``
(translation and rotation, ``DESIGN.md`` 4.25), and what every stepper's
host side shares (``DESIGN.md`` 4.20): the launch helper ``_launch``, the owner of a device-resident control state
``_ControlState``, the partials buffer of the controlled-Verlet schemes, the refusals of the methods that move every
particle, and the base of the Langevin / Brownian family ``_StochasticMethod``. ``Simulation.run`` (``simulation.py``)
drives them; ``thermostats``, ``minimize`` and ``flow`` build on them."""

import ctypes as C
import math

import numpy as np

from . import _lib
from .filter import All, Type


def _launch(a, st, stream, *names):
    """Queue the libazp integration entries ``names`` with their argument struct ``a`` pointed at the state's arrays of
    this moment (they are replaced when particles migrate between ranks or are re-sorted), and at the state's box when
    ``box_generation`` has moved since the struct's box was written (``State.set_box``, ``update.BoxResize``); a fresh
    struct has no box yet. A struct with the fields ``d_accel`` and ``d_tag`` (the flow methods') gets them too."""
    generation = getattr(st, "box_generation", 0)  # (a stand-in state without the counter keeps its box)
    if getattr(a, "_box_generation", None) != generation:
        a.box = st.box.to_c()
        a._box_generation = generation
    a.d_pos = st.pos.data_ptr()
    a.d_vel = st.vel.data_ptr()
    a.d_net_force = st.net_force.data_ptr()
    a.d_image = st.image.data_ptr()
    a.N = st.N
    if hasattr(a, "d_accel"):
        a.d_accel = st.accel.data_ptr() if st.accel is not None else None
        a.d_tag = st.tag.data_ptr()
    lib = _lib.lib()
    for name in names:
        _lib.check(getattr(lib, name)(C.byref(a), stream), name)


def _net_torque(sim):
    """The net torque on the particles of ``sim``: the sum of the forces' ``torque_tensor`` (without forces a zero tensor,
    made once per state size); the caller keeps it until its kernel is queued."""
    st, forces = sim.state, sim.operations.integrator.forces
    if not forces:
        zero = getattr(st, "_zero_torque", None)
        if zero is None or zero.shape[0] != st.N:
            import torch

            zero = st._zero_torque = torch.zeros((st.N, 4), dtype=torch.float64, device=st.device)
        return zero
    torque = forces[0].torque_tensor
    if len(forces) > 1:
        torque = torque.clone()
        for f in forces[1:]:
            torque += f.torque_tensor
    return torque


class _ControlState:
    """The control state of a stepper whose step is controlled on the device (the thermostats, ``minimize.FIRE``,
    ``ConstantPressure``): a few float64 doubles that start from the host list ``start`` (editable until the first bind),
    live in ``tensor`` from the first run on, persist across runs and follow the particles to their device. ``name``
    leads the error messages."""

    def __init__(self, name, start):
        self._name = name
        self.start = list(start)
        self.tensor = None

    def bind(self, device):
        """Make the tensor from ``start`` (first run) or move it to ``device``; returns its data pointer."""
        if self.tensor is None or self.tensor.device != device:
            import torch

            self.tensor = torch.tensor(self.host(), dtype=torch.float64, device=device)
        return self.tensor.data_ptr()

    def host(self):
        """The whole state as a list; reading synchronises."""
        return list(self.start) if self.tensor is None else self.tensor.tolist()

    def get(self, k, n=1):
        """Slots k .. k + n - 1; reading synchronises."""
        return tuple(self.host()[k:k + n])

    def set(self, k, values, what):
        values = [float(v) for v in values]
        if not all(math.isfinite(v) for v in values):
            raise _lib.AzpError("%s: %s must be finite, got %r" % (self._name, what, values))
        if self.tensor is None:
            self.start[k:k + len(values)] = values
        else:
            import torch

            self.tensor[k:k + len(values)] = torch.tensor(values, dtype=torch.float64)

    def reset(self, values):
        """Write ``values`` over the whole state."""
        self.set(0, values, "the state")


class _DeviceControlled:
    """What the owners of a ``_ControlState`` (``self._control``) share: ``_state``, its tensor (None before the first run)."""

    @property
    def _state(self):
        return self._control.tensor


def _bind_partials(a, st, size_entry, partials):
    """The buffer that the sums of a controlled-Verlet scheme (``csrc/controlled_verlet.hpp``: the thermostats, FIRE)
    pass through: ``partials`` if it is on the state's device and holds what libazp's ``size_entry`` asks for N
    particles, else a new one; the argument struct ``a`` is pointed at it. Returns the buffer, which the caller keeps."""
    need = C.c_uint64(0)
    _lib.check(getattr(_lib.lib(), size_entry)(st.N, C.byref(need)), size_entry)
    if partials is None or partials.numel() * 8 < need.value or partials.device != st.vel.device:
        import torch

        partials = torch.zeros(int(need.value) // 8, dtype=torch.float64, device=st.vel.device)
    a.d_partials = partials.data_ptr()
    a.partials_bytes = partials.numel() * 8
    return partials


def _check_moves_all(name, sums, method, sim, integ):
    """What a method that moves every particle by one device-computed factor cannot do (a thermostatted
    ``ConstantVolume``, ``ConstantPressure``), each refused with its reason. ``name`` leads the messages, ``sums`` names
    what the method sums over all particles every step."""
    if not isinstance(method.filter, All):
        raise _lib.AzpError("%s: only filter=All() is supported (%s is summed over all particles), got %r" % (name, sums, method.filter))
    if integ.integrate_rotational_dof:
        raise _lib.AzpError("%s: rotational degrees of freedom are not supported (integrate_rotational_dof=True)" % name)
    if sim.domain is not None:
        raise _lib.AzpError("%s does not run decomposed (%s would need a collective every step)" % (name, sums))
    if sim.state.N < 2:
        raise _lib.AzpError("%s: fewer than 2 particles leave no degree of freedom (Nf = 3 N - 3), N = %d" % (name, sim.state.N))
    th = method.thermostat
    if th is not None:
        if th._kind == _lib.THERMOSTAT_BERENDSEN and th.tau < integ.dt:
            raise _lib.AzpError("%s: tau = %r is below dt = %r (the rescaling factor's radicand can turn negative)"
                                % (th._name, th.tau, integ.dt))
        if any(m is not method for m in th._holders):
            raise _lib.AzpError("%s: one thermostat object is held by two methods (its state belongs to one run)" % th._name)


class _HoldsThermostat:
    """``thermostat`` of ``ConstantVolume`` and ``ConstantPressure``: None or one of ``azplugins_amd.thermostats``, which
    knows the methods that hold it (one thermostat object belongs to one method)."""

    _thermostat = None

    @property
    def thermostat(self):
        return self._thermostat

    @thermostat.setter
    def thermostat(self, thermostat):
        from .thermostats import _Thermostat

        if thermostat is not None and not isinstance(thermostat, _Thermostat):
            raise _lib.AzpError("%s: thermostat must be None or one of azplugins_amd.thermostats, got %r"
                                % (type(self).__name__, thermostat))
        if self._thermostat is not None:
            self._thermostat._holders.discard(self)
        if thermostat is not None:
            thermostat._holders.add(self)
        self._thermostat = thermostat


class ConstantVolume(_HoldsThermostat):
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
        self.thermostat = thermostat

    # -- the stepper of the NVE path; with a thermostat the thermostat steps --------
    _fusable = True
    _updaters_split = False  # (an updater changes types alone, which these kernels do not read)

    def _begin(self, sim):
        integ = sim.operations.integrator
        a = self._args = _lib.NVEArgs()
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
        st, rot = sim.state, self._rot
        torque = _net_torque(sim)  # (kept alive until the kernel is queued)
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


class ConstantPressure(_HoldsThermostat, _DeviceControlled):
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
        self.thermostat = thermostat
        self._control = _ControlState("ConstantPressure", [0.0] * _lib.BAROSTAT_NSTATE)
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

    # -- device-resident state ---------------------------------------------------
    def _slots(self, k, n=1):
        return self._control.get(k, n)

    @property
    def barostat_dof(self):
        """(nu_x, nu_y, nu_z): the rates of the three box lengths, d ln L_a / dt."""
        return self._control.get(_lib.BAROSTAT_NU, 3)

    @barostat_dof.setter
    def barostat_dof(self, value):
        value = tuple(value)
        if len(value) != 3:
            raise _lib.AzpError("ConstantPressure: barostat_dof takes (nu_x, nu_y, nu_z), got %r" % (value,))
        self._control.set(_lib.BAROSTAT_NU, value, "barostat_dof")

    @property
    def barostat_energy(self):
        """(W / 2)(nu_x^2 + nu_y^2 + nu_z^2) as of the last step run (0 before the first)."""
        return self._control.get(_lib.BAROSTAT_ENERGY)[0]

    @property
    def reference_kT(self):
        """kT_ref of the barostat's mass W = (Nf + 3) kT_ref tauS^2 in a run without a thermostat: 2 K / Nf at the first
        step of the first run (0 before it), or what was set. With a thermostat its kT is used instead."""
        return self._control.get(_lib.BAROSTAT_REF_KT)[0]

    @reference_kT.setter
    def reference_kT(self, value):
        if not float(value) >= 0.0:
            raise _lib.AzpError("ConstantPressure: reference_kT must be >= 0 (0: measure it at the next step), got %r" % (value,))
        self._control.set(_lib.BAROSTAT_REF_KT, [value], "reference_kT")

    # -- the stepper -------------------------------------------
    def _check(self, sim, integ):
        """What ``ConstantPressure`` cannot do, each refused with its reason."""
        if len(integ.methods) != 1:
            raise _lib.AzpError("ConstantPressure must be the only method of the integrator (it scales every particle and the "
                                "box), got %r" % (integ.methods,))
        _check_moves_all("ConstantPressure", "the pressure", self, sim, integ)
        box = sim.state.box
        if box.is_triclinic:
            raise _lib.AzpError("ConstantPressure: %r is tilted: only orthorhombic boxes are supported" % (box,))
        for k in range(3):
            if self.box_dof[k] and not box.periodic[k]:
                raise _lib.AzpError("ConstantPressure: the box is not periodic along %s, which box_dof leaves free: a free axis "
                                    "must be periodic" % "xyz"[k])
        if len(integ.forces) > _lib.THERMO_MAX_FORCES:
            raise _lib.AzpError("ConstantPressure sums the virials of at most %d forces, the integrator has %d"
                                % (_lib.THERMO_MAX_FORCES, len(integ.forces)))

    def _begin(self, sim):
        import torch

        from .compute import ThermodynamicQuantities

        integ, st = sim.operations.integrator, sim.state
        self._check(sim, integ)
        dev = st.vel.device
        if self._row is None or self._row.device != dev:
            self._row = torch.zeros(_lib.THERMO_NSUMS, dtype=torch.float64, device=dev)
        if self._thermo is None:
            self._thermo = ThermodynamicQuantities(All())  # (never in sim.operations.computes: its launch machinery alone)
        self._thermo._sim = sim
        a = self._args = _lib.BarostatArgs()
        a.d_state = self._control.bind(dev)
        a.d_sums = self._row.data_ptr()
        a.dt = integ.dt
        a.tauS = self.tauS
        a.ndof = float(3 * st.N - 3)
        a.couple = _lib.BAROSTAT_COUPLE[self.couple]
        a.box_dof = sum(1 << k for k in range(3) if self.box_dof[k])
        th = self.thermostat
        if th is not None:
            a.d_thermostat_state = th._bind(sim)
            a.thermostat_tau = th.tau
            a.thermostat_kind = th._kind
            a.thermostat_seed = int(sim.seed or 0) & 0xFFFF
        self._stream = _lib.raw_stream(st.device)
        self._first = True  # (the first step opens from a sums pass of the state as it stands)

    def _advance(self, sim, timestep, phase):
        a = self._args
        a.S[:] = self._S_at(timestep)
        a.timestep = timestep
        a.phase = phase
        th = self.thermostat
        if th is not None:
            a.thermostat_kT = th._open_step(timestep) if phase & _lib.BAROSTAT_OPEN else th._kT_at(timestep)
        _launch(a, sim.state, self._stream, "azp_barostat_advance")

    def _step_one(self, sim, timestep, fused):
        from .state import Box

        st = sim.state
        if self._first:
            self._thermo._launch(self._row.data_ptr())
            self._first = False
        self._advance(sim, timestep, _lib.BAROSTAT_OPEN)
        # the one host read of the step: the box lives on the host
        host = self._control.host()
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


# ---------------------------------------------------------------------------
# the Langevin / Brownian family: flow.Langevin, flow.Brownian, Langevin, Brownian
# ---------------------------------------------------------------------------
def _finite(x, what):
    x = float(x)
    if not math.isfinite(x):
        raise _lib.AzpError("%s must be finite, got %r" % (what, x))
    return x


class _Gamma:
    """Per-type friction coefficients: ``method.gamma["A"] = 2.0``; types never set take the default. ``check`` validates
    a value and gives what is stored: a float (``gamma``) or a tuple of three (``gamma_r``, one per body axis)."""

    def __init__(self, default, check):
        self._check = check
        self._values = {}
        self.default = check(default)

    def __setitem__(self, types, value):
        value = self._check(value)
        for t in ([types] if isinstance(types, str) else list(types)):
            self._values[t] = value

    def __getitem__(self, t):
        return self._values.get(t, self.default)

    def table(self, type_names):
        """One row per type of ``type_names``: shape (ntypes,) or (ntypes, 3)."""
        return np.array([self[t] for t in type_names], dtype=np.float64)


class _StochasticMethod:
    """What the Langevin and Brownian methods share, with a flow field (``flow``) or with rotation (below): a filter
    ``All()`` or ``Type(...)``, ``kT`` evaluated on the host per step, per-type ``gamma``, and the stepper interface of
    DESIGN 4.20. Several of them may sit in ``Integrator.methods`` with pairwise-disjoint filters
    (``Simulation._check_flow_methods``)."""

    _name = None
    _uses_accel = False  # a Langevin method: step two stores what the next step one reads (State.accel, langevin_torque)
    _fusable = True
    # a method filtered by type reads the types when its kernel runs: where an updater is due, step two of the previous
    # step runs on its own ahead of the updater, as in HOOMD (the fused kernel is bit-identical to the two halves)
    _updaters_split = True

    def __init__(self, filter, kT, default_gamma):
        if not isinstance(filter, (All, Type)):
            raise _lib.AzpError("%s: filter must be All() or Type(...), got %r" % (self._name, filter))
        if not callable(kT):
            kT = _finite(kT, "%s kT" % self._name)
            if kT < 0.0:
                raise _lib.AzpError("%s: kT must be >= 0, got %r" % (self._name, kT))
        self.filter = filter
        self.kT = kT
        self.gamma = _Gamma(default_gamma, self._check_gamma)
        self._tables = None

    def _check_gamma(self, g):
        raise NotImplementedError

    def _kT(self, timestep):
        """kT at ``timestep``, evaluated on the host (passed to the kernel by value)."""
        return float(self.kT(timestep)) if callable(self.kT) else float(self.kT)

    def _gamma_tables(self, types):
        """The per-type tables the kernel reads, as numpy arrays in the order of its pointers."""
        return (self.gamma.table(types),)

    def _begin_tables(self, sim):
        """The seed warning; the accelerations of a first run; the gamma tables and the type mask on the device (made
        again when the types, a gamma or the filter changed). Returns (tables, mask or None)."""
        import torch

        st = sim.state
        sim._warn_if_seed_unset()
        if self._uses_accel and (st.accel is None or st.accel.shape[0] != st.n_max):
            # HOOMD computeAccelerations (prepRun): a = F_net / m on the first run of an integrator that needs it
            st.accel = torch.zeros((st.n_max, 4), dtype=torch.float64, device=st.device)
            st.accel[: st.N, :3] = st.net_force[: st.N, :3] / st.vel[: st.N, 3:4]
        tables = self._gamma_tables(st.types)
        key = (tuple(st.types), tuple(t.tobytes() for t in tables), self.filter)
        if self._tables is None or self._tables[0] != key:
            g = tuple(torch.from_numpy(t).to(st.device) for t in tables)
            m = None if isinstance(self.filter, All) else torch.from_numpy(self.filter.mask(st.types)).to(st.device)
            self._tables = (key, g, m)
        return self._tables[1:]

    def _at(self, timestep):
        """The argument struct at ``timestep`` (random numbers and kT)."""
        a = self._args
        a.timestep = int(timestep)
        a.kT = self._kT(timestep)
        return a


class _RotationalMethod(_StochasticMethod):
    """``Langevin`` and ``Brownian`` under the names of ``hoomd.md.methods``: translation as the flow methods at zero flow
    (bit for bit), and the rotation of particles with a moment of inertia where ``Integrator.integrate_rotational_dof`` is
    set (else the rotational arrays are not read). HOOMD-blue's source is not available to this project: the scheme is
    defined in ``include/azp.h`` and ``DESIGN.md`` 4.25 and runs in libazp (``csrc/langevin.hip``), one thread moving and
    rotating its particle in one pass."""

    def __init__(self, filter, kT, default_gamma=1.0, default_gamma_r=(1.0, 1.0, 1.0)):
        super().__init__(filter, kT, default_gamma)
        self.gamma_r = _Gamma(default_gamma_r, self._check_gamma_r)

    def _check_gamma_r(self, g):
        try:
            g = tuple(g)
        except TypeError:
            g = ()
        if len(g) != 3:
            raise _lib.AzpError("%s: gamma_r takes three values, one per body axis, got %r" % (self._name, g))
        return tuple(self._check_gamma(x) for x in g)

    def _gamma_tables(self, types):
        return (self.gamma.table(types), self.gamma_r.table(types).reshape(len(types), 3))

    def _begin(self, sim):
        """The argument struct of this run; with rotation, the Langevin torques of a first run (zeros)."""
        import torch

        st, integ = sim.state, sim.operations.integrator
        (g, g_r), m = self._begin_tables(sim)
        a = self._args = _lib.LangevinArgs()
        a.d_gamma = g.data_ptr()
        a.d_gamma_r = g_r.data_ptr()
        a.d_type_mask = m.data_ptr() if m is not None else None
        a.dt = integ.dt
        a.seed = int(sim.seed) & 0xFFFF
        a.ntypes = len(st.types)
        a.rotational = int(bool(integ.integrate_rotational_dof))
        if a.rotational and self._uses_accel and (st.langevin_torque is None or st.langevin_torque.shape[0] != st.n_max):
            st.langevin_torque = torch.zeros((st.n_max, 4), dtype=torch.float64, device=st.device)
        self._stream = _lib.raw_stream(st.device)

    def _queue(self, sim, timestep, name):
        """Queue entry ``name`` with the random numbers and kT of ``timestep``, pointed at the arrays of this moment."""
        a, st = self._at(timestep), sim.state
        torque = None
        if a.rotational:
            torque = _net_torque(sim)  # (kept alive until the kernel is queued)
            a.d_orientation = st.orientation.data_ptr()
            a.d_angmom = st.angmom.data_ptr()
            a.d_inertia = st.inertia.data_ptr()
            a.d_net_torque = torque.data_ptr()
            a.d_langevin_torque = st.langevin_torque.data_ptr() if self._uses_accel else None
        _launch(a, st, self._stream, name)


class Langevin(_RotationalMethod):
    """``hoomd.md.methods.Langevin``: velocity Verlet with the friction -gamma v and a uniform random force of variance
    2 gamma kT / dt per component in the acceleration (``flow.Langevin`` at zero flow), and for the rotation the NO_SQUISH
    step of ``ConstantVolume`` with the body-frame Langevin torque b_k = R_k - gamma_r,k S_k / I_k, var(R_k) =
    2 gamma_r,k kT / dt, computed in step two and used again by the next step one (``State.langevin_torque``).

    ``kT``: a float >= 0 or a callable of the timestep; 0 is the noiseless run. ``gamma[type]`` >= 0,
    ``gamma_r[type]`` three values >= 0. ``tally_reservoir_energy=True`` is refused: it would need a reduction every
    step. Does not run decomposed."""

    _name = "methods.Langevin"
    _uses_accel = True

    def __init__(self, filter, kT, tally_reservoir_energy=False, default_gamma=1.0, default_gamma_r=(1.0, 1.0, 1.0)):
        if tally_reservoir_energy:
            raise _lib.AzpError("methods.Langevin: tally_reservoir_energy=True is not supported (the reservoir energy would "
                                "need a reduction over all particles every step)")
        self.tally_reservoir_energy = False
        super().__init__(filter, kT, default_gamma, default_gamma_r)

    def _check_gamma(self, g):
        g = _finite(g, "methods.Langevin gamma")
        if g < 0.0:
            raise _lib.AzpError("methods.Langevin: gamma and gamma_r must be >= 0, got %r" % (g,))
        return g

    def _step_one(self, sim, timestep, fused):
        """Step one of the step starting at ``timestep`` (fused: preceded by step two of the previous step, whose
        random numbers and kT belong to ``timestep - 1``; step one itself draws nothing)."""
        if fused:
            self._queue(sim, timestep - 1, "azp_integrate_langevin_step_two_one")
        else:
            self._queue(sim, timestep, "azp_integrate_langevin_step_one")

    def _step_two(self, sim, timestep):
        self._queue(sim, timestep, "azp_integrate_langevin_step_two")


class Brownian(_RotationalMethod):
    """``hoomd.md.methods.Brownian``: x += (F + R) dt / gamma (``flow.Brownian`` at zero flow), and for the rotation the
    body-frame rotation vector dtheta_k = (torque_k + R_k) dt / gamma_r,k applied through the exponential map; velocities
    and angular momenta are not touched.

    ``kT``: a float >= 0 or a callable of the timestep; 0 is the noiseless run. ``gamma[type]`` > 0, ``gamma_r[type]``
    three values > 0 (the step divides by them). Does not run decomposed."""

    _name = "methods.Brownian"

    def _check_gamma(self, g):
        g = _finite(g, "methods.Brownian gamma")
        if not g > 0.0:
            raise _lib.AzpError("methods.Brownian: gamma and gamma_r must be > 0 (the step divides by them), got %r" % (g,))
        return g

    def _step_one(self, sim, timestep, fused):
        """The whole step starting at ``timestep``."""
        self._queue(sim, timestep, "azp_integrate_brownian_step")

    def _step_two(self, sim, timestep):
        pass  # Brownian dynamics has no second half
