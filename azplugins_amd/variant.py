"""``hoomd.azplugins.variant``: quantities that change with the timestep. ``SphereArea`` is the radius of a droplet
whose surface area shrinks at a constant rate (src/VariantSphereArea.{h,cc}); it is a callable of the timestep, which
is what ``external.SphericalHarmonicBarrier(location=...)`` takes.

The scalar variants of ``hoomd.variant`` are here too (``Constant``, ``Ramp``, ``Cycle``, ``Power``: callables of the
timestep with ``min`` and ``max``), and ``variant.box`` (azplugins_amd/variant_box.py) holds the box variants that
``update.BoxResize`` takes."""

import math

from . import _lib


def _finite(name, **values):
    out = []
    for key, v in values.items():
        v = float(v)
        if not math.isfinite(v):
            raise _lib.AzpError("%s: %s must be finite, got %r" % (name, key, v))
        out.append(v)
    return out


def _steps(name, positive=(), **values):
    out = []
    for key, v in values.items():
        if isinstance(v, bool) or int(v) != v or int(v) < (1 if key in positive else 0):
            raise _lib.AzpError("%s: %s must be a%s integer number of timesteps, got %r"
                                % (name, key, " positive" if key in positive else " non-negative", v))
        out.append(int(v))
    return out


class _Scalar:
    """A scalar variant: ``v(timestep)``, ``min`` and ``max`` over all timesteps, equality by parameters."""

    _fields = ()

    def _values(self):
        return tuple(getattr(self, f) for f in self._fields)

    def __eq__(self, other):
        return type(other) is type(self) and other._values() == self._values()

    def __hash__(self):
        return hash((type(self).__name__,) + self._values())

    def __repr__(self):
        return "%s(%s)" % (type(self).__name__, ", ".join("%s=%r" % (f, getattr(self, f)) for f in self._fields))


class Constant(_Scalar):
    """``hoomd.variant.Constant``: ``value`` at every timestep."""

    _fields = ("value",)

    def __init__(self, value):
        (self.value,) = _finite("Constant", value=value)

    def __call__(self, timestep):
        return self.value

    min = max = property(lambda self: self.value)


class Ramp(_Scalar):
    """``hoomd.variant.Ramp``: ``A`` up to ``t_start``, ``A (1 - s) + B s`` with ``s = (t - t_start) / t_ramp`` during
    the ``t_ramp`` steps that follow, ``B`` afterwards."""

    _fields = ("A", "B", "t_start", "t_ramp")

    def __init__(self, A, B, t_start, t_ramp):
        self.A, self.B = _finite("Ramp", A=A, B=B)
        self.t_start, self.t_ramp = _steps("Ramp", positive=("t_ramp",), t_start=t_start, t_ramp=t_ramp)

    def __call__(self, timestep):
        t = int(timestep)
        if t < self.t_start:
            return self.A
        if t < self.t_start + self.t_ramp:
            s = (t - self.t_start) / self.t_ramp
            return self.A * (1.0 - s) + self.B * s
        return self.B

    min = property(lambda self: min(self.A, self.B))
    max = property(lambda self: max(self.A, self.B))


class Cycle(_Scalar):
    """``hoomd.variant.Cycle``: ``A`` up to ``t_start``, then periodically ``A`` for ``t_A`` steps, a linear ramp to
    ``B`` over ``t_AB``, ``B`` for ``t_B`` and a linear ramp back to ``A`` over ``t_BA``."""

    _fields = ("A", "B", "t_start", "t_A", "t_AB", "t_B", "t_BA")

    def __init__(self, A, B, t_start, t_A, t_AB, t_B, t_BA):
        self.A, self.B = _finite("Cycle", A=A, B=B)
        self.t_start, self.t_A, self.t_AB, self.t_B, self.t_BA = _steps(
            "Cycle", positive=("t_AB", "t_BA"), t_start=t_start, t_A=t_A, t_AB=t_AB, t_B=t_B, t_BA=t_BA)

    def __call__(self, timestep):
        t = int(timestep)
        if t < self.t_start:
            return self.A
        d = (t - self.t_start) % (self.t_A + self.t_AB + self.t_B + self.t_BA)
        if d < self.t_A:
            return self.A
        if d < self.t_A + self.t_AB:
            s = (d - self.t_A) / self.t_AB
            return self.B * s + self.A * (1.0 - s)
        if d < self.t_A + self.t_AB + self.t_B:
            return self.B
        s = (d - (self.t_A + self.t_AB + self.t_B)) / self.t_BA
        return self.A * s + self.B * (1.0 - s)

    min = property(lambda self: min(self.A, self.B))
    max = property(lambda self: max(self.A, self.B))


class Power(_Scalar):
    """``hoomd.variant.Power``: ``A`` up to ``t_start``, ``(A^(1/power) (1 - s) + B^(1/power) s)^power`` with
    ``s = (t - t_start) / t_ramp`` during the ``t_ramp`` steps that follow, ``B`` afterwards. ``A``, ``B`` >= 0."""

    _fields = ("A", "B", "power", "t_start", "t_ramp")

    def __init__(self, A, B, power, t_start, t_ramp):
        self.A, self.B, self.power = _finite("Power", A=A, B=B, power=power)
        if self.power == 0.0 or self.A < 0.0 or self.B < 0.0:
            raise _lib.AzpError("Power: power must not be 0 and A, B must not be negative, got A=%r, B=%r, power=%r" % (A, B, power))
        self.t_start, self.t_ramp = _steps("Power", positive=("t_ramp",), t_start=t_start, t_ramp=t_ramp)

    def __call__(self, timestep):
        t = int(timestep)
        if t < self.t_start:
            return self.A
        if t < self.t_start + self.t_ramp:
            s = (t - self.t_start) / self.t_ramp
            inv = 1.0 / self.power
            return (self.B ** inv * s + self.A ** inv * (1.0 - s)) ** self.power
        return self.B

    min = property(lambda self: min(self.A, self.B))
    max = property(lambda self: max(self.A, self.B))


class SphereArea:
    """R(t) = sqrt(R0^2 - alpha t / (4 pi)): a sphere of initial radius ``R0`` whose area drops by ``alpha`` per
    timestep; 0 once ``alpha t / (4 pi) >= R0^2`` (src/VariantSphereArea.cc:18-41)."""

    def __init__(self, R0, alpha):
        self.R0 = float(R0)
        self.alpha = float(alpha)
        if not (math.isfinite(self.R0) and math.isfinite(self.alpha)):
            raise _lib.AzpError("SphereArea: R0 and alpha must be finite, got %r, %r" % (R0, alpha))

    def __call__(self, timestep):
        R0_sq = self.R0 * self.R0
        drsq = self.alpha / (4.0 * math.pi) * timestep
        if drsq >= R0_sq:  # the droplet cannot shrink below zero
            return 0.0
        return math.sqrt(R0_sq - drsq)

    def __eq__(self, other):
        return isinstance(other, SphereArea) and (other.R0, other.alpha) == (self.R0, self.alpha)

    def __repr__(self):
        return "SphereArea(R0=%r, alpha=%r)" % (self.R0, self.alpha)


from . import variant_box as box  # noqa: E402  (``variant.box``, as ``hoomd.variant.box``)
