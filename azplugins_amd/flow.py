"""``hoomd.azplugins.flow`` (src/flow.py): the flow fields ``ConstantFlow`` and ``ParabolicFlow`` and the
integration methods that consume them, ``Langevin`` (``TwoStepLangevinFlow``) and ``Brownian``
(``TwoStepBrownianFlow``). The methods run in libazp (csrc/flow_methods.hip); ``Simulation.run`` drives them.

The fields are plain parameter holders (they pickle); ``_cpp()`` gives the ``_azplugins`` object with the
reference's constructor and properties, which also evaluates the field on the host."""

from . import _lib
from .methods import _finite, _launch, _StochasticMethod


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


class _FlowMethod(_StochasticMethod):
    def __init__(self, filter, kT, flow_field, default_gamma=1.0, noiseless=False):
        if not isinstance(flow_field, FlowField):
            raise _lib.AzpError("%s: flow_field must be a ConstantFlow or a ParabolicFlow, got %r" % (self._name, flow_field))
        super().__init__(filter, kT, default_gamma)
        self.flow_field = flow_field
        self.noiseless = bool(noiseless)

    # -- the stepper -----------------------------------------------
    def _begin(self, sim):
        """The seed warning, the accelerations of a first run and the device tables (``_begin_tables``); the argument
        struct of this run."""
        st = sim.state
        (g,), m = self._begin_tables(sim)
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
