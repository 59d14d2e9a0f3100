"""``hoomd.azplugins.flow`` (src/flow.py): the flow fields ``ConstantFlow`` and ``ParabolicFlow`` and the
integration methods that consume them, ``Langevin`` (``TwoStepLangevinFlow``) and ``Brownian``
(``TwoStepBrownianFlow``). The methods run in libazp (csrc/flow_methods.hip); ``Simulation.run`` drives them.

The fields are plain parameter holders (they pickle); ``_cpp()`` gives the ``_azplugins`` object with the
reference's constructor and properties, which also evaluates the field on the host."""

import math

import numpy as np

from . import _lib
from .filter import All, Type
from .methods import _launch


def _finite(x, what):
    x = float(x)
    if not math.isfinite(x):
        raise _lib.AzpError("%s must be finite, got %r" % (what, x))
    return x


class FlowField:
    """Base flow field."""

    def _c(self):
        """The ``azp_flow`` struct the kernels take."""
        raise NotImplementedError


class ConstantFlow(FlowField):
    """Constant flow u(r) = U, e.g. a backflow in bulk or a plug flow in a channel."""

    def __init__(self, velocity):
        self.velocity = velocity

    @property
    def velocity(self):
        return self._velocity

    @velocity.setter
    def velocity(self, velocity):
        v = tuple(velocity)
        if len(v) != 3:
            raise _lib.AzpError("ConstantFlow: velocity must have 3 components, got %r" % (velocity,))
        self._velocity = tuple(_finite(x, "ConstantFlow velocity") for x in v)

    def _cpp(self):
        return _lib.ext_module().ConstantFlow(self._velocity)

    def _c(self):
        f = _lib.Flow()
        f.kind = _lib.FLOW_CONSTANT
        for k in range(3):
            f.p[k] = self._velocity[k]
        return f

    def __eq__(self, other):
        return isinstance(other, ConstantFlow) and other._velocity == self._velocity

    def __repr__(self):
        return "ConstantFlow(velocity=%r)" % (self._velocity,)


class ParabolicFlow(FlowField):
    """Parabolic flow between parallel plates at y = +-separation/2: u_x(y) = 3/2 U (1 - (y / H)^2), H =
    separation / 2, along x with the gradient in y. The walls are the user's business (e.g. a
    two-plane ``wall.LJ93`` slit, or harmonic barriers)."""

    def __init__(self, mean_velocity, separation):
        self.mean_velocity = mean_velocity
        self.separation = separation

    @property
    def mean_velocity(self):
        return self._mean_velocity

    @mean_velocity.setter
    def mean_velocity(self, U):
        self._mean_velocity = _finite(U, "ParabolicFlow mean_velocity")

    @property
    def separation(self):
        return self._separation

    @separation.setter
    def separation(self, s):
        s = _finite(s, "ParabolicFlow separation")
        if not s > 0.0:
            raise _lib.AzpError("ParabolicFlow: separation must be > 0, got %r" % (s,))
        self._separation = s

    def _cpp(self):
        return _lib.ext_module().ParabolicFlow(self._mean_velocity, self._separation)

    def _c(self):
        # src/ParabolicFlow.h stores Umax = 1.5 U and L = separation / 2; the kernel evaluates Umax (1 - (y / L)^2)
        cpp = self._cpp()
        f = _lib.Flow()
        f.kind = _lib.FLOW_PARABOLIC
        f.p[0], f.p[1], f.p[2] = cpp.Umax, cpp.L, 0.0
        return f

    def __eq__(self, other):
        return isinstance(other, ParabolicFlow) and (other._mean_velocity, other._separation) == (
            self._mean_velocity, self._separation)

    def __repr__(self):
        return "ParabolicFlow(mean_velocity=%r, separation=%r)" % (self._mean_velocity, self._separation)


class _Gamma:
    """Per-type friction coefficients: ``method.gamma["A"] = 2.0``; types never set take the default."""

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
        return np.array([self[t] for t in type_names], dtype=np.float64)


class _FlowMethod:
    _name = None

    def __init__(self, filter, kT, flow_field, default_gamma=1.0, noiseless=False):
        if not isinstance(filter, (All, Type)):
            raise _lib.AzpError("%s: filter must be All() or Type(...), got %r" % (self._name, filter))
        if not isinstance(flow_field, FlowField):
            raise _lib.AzpError("%s: flow_field must be a ConstantFlow or a ParabolicFlow, got %r" % (self._name, flow_field))
        if not callable(kT):
            kT = _finite(kT, "%s kT" % self._name)
            if kT < 0.0:
                raise _lib.AzpError("%s: kT must be >= 0, got %r" % (self._name, kT))
        self.filter = filter
        self.kT = kT
        self.flow_field = flow_field
        self.gamma = _Gamma(default_gamma, self._check_gamma)
        self.noiseless = bool(noiseless)
        self._tables = None

    def _check_gamma(self, g):
        raise NotImplementedError

    def _kT(self, timestep):
        """kT at ``timestep``, evaluated on the host (passed to the kernel by value)."""
        return float(self.kT(timestep)) if callable(self.kT) else float(self.kT)

    # -- the stepper -----------------------------------------------
    _fusable = True
    # a method filtered by type reads the types when its kernel runs: where an updater is due, step two of the previous
    # step runs on its own ahead of the updater, as in HOOMD (the fused kernel is bit-identical to the two halves)
    _updaters_split = True

    def _begin(self, sim):
        """The seed warning; the accelerations of a first run; the gamma table and the type mask on the device; the
        argument struct of this run."""
        import torch

        st = sim.state
        sim._warn_if_seed_unset()
        if self._uses_accel and (st.accel is None or st.accel.shape[0] != st.n_max):
            # HOOMD computeAccelerations (prepRun): a = F_net / m on the first run of an integrator that needs it
            st.accel = torch.zeros((st.n_max, 4), dtype=torch.float64, device=st.device)
            st.accel[: st.N, :3] = st.net_force[: st.N, :3] / st.vel[: st.N, 3:4]
        key = (tuple(st.types), tuple(self.gamma.table(st.types)), self.filter)
        if self._tables is None or self._tables[0] != key:
            g = torch.from_numpy(self.gamma.table(st.types)).to(st.device)
            m = None if isinstance(self.filter, All) else torch.from_numpy(self.filter.mask(st.types)).to(st.device)
            self._tables = (key, g, m)
        _, g, m = self._tables
        a = _lib.FlowMethodArgs()
        a.d_gamma = g.data_ptr()
        a.d_type_mask = m.data_ptr() if m is not None else None
        a.dt = sim.operations.integrator.dt
        a.seed = int(sim.seed) & 0xFFFF
        a.noiseless = int(self.noiseless)
        a.ntypes = len(st.types)
        a.flow = self.flow_field._c()
        self._args = a
        self._stream = _lib.raw_stream(st.device)

    def _at(self, timestep):
        """The argument struct at ``timestep`` (random numbers and kT)."""
        a = self._args
        a.timestep = int(timestep)
        a.kT = self._kT(timestep)
        return a


class Langevin(_FlowMethod):
    """Langevin dynamics in a flow field (``TwoStepLangevinFlow``): velocity Verlet with the friction
    -gamma (v - u(r)) and a uniform random force of variance 2 gamma kT / dt per component added to the
    acceleration. ``gamma``: per type, >= 0. ``kT``: a float or a callable of the timestep."""

    _name = "flow.Langevin"
    _uses_accel = True

    def _check_gamma(self, g):
        g = _finite(g, "flow.Langevin gamma")
        if g < 0.0:
            raise _lib.AzpError("flow.Langevin: gamma must be >= 0, got %r" % (g,))
        return g

    def _step_one(self, sim, timestep, fused):
        """Step one of the step starting at ``timestep`` (fused: preceded by step two of the previous step, whose
        random numbers and kT belong to ``timestep - 1``; step one itself draws nothing)."""
        if fused:
            _launch(self._at(timestep - 1), sim.state, self._stream, "azp_integrate_langevin_flow_step_two_one")
        else:
            _launch(self._at(timestep), sim.state, self._stream, "azp_integrate_langevin_flow_step_one")

    def _step_two(self, sim, timestep):
        _launch(self._at(timestep), sim.state, self._stream, "azp_integrate_langevin_flow_step_two")


class Brownian(_FlowMethod):
    """Brownian dynamics in a flow field (``TwoStepBrownianFlow``): x += (u(x) + (F + R) / gamma) dt with a
    uniform random force of variance 2 gamma kT / dt per component; velocities are not touched. ``gamma``: per
    type, > 0. ``kT``: a float or a callable of the timestep."""

    _name = "flow.Brownian"
    _uses_accel = False

    def _check_gamma(self, g):
        g = _finite(g, "flow.Brownian gamma")
        if not g > 0.0:
            raise _lib.AzpError("flow.Brownian: gamma must be > 0 (the step divides by it), got %r" % (g,))
        return g

    def _step_one(self, sim, timestep, fused):
        """The whole step starting at ``timestep``."""
        _launch(self._at(timestep), sim.state, self._stream, "azp_integrate_brownian_flow_step")

    def _step_two(self, sim, timestep):
        pass  # Brownian dynamics has no second half
