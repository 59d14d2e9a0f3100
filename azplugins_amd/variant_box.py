"""``variant.box`` (``hoomd.variant.box``): boxes that change with the timestep, callables of the timestep that return
a ``state.Box``. ``update.BoxResize`` takes one. The periodic flags of a box variant are those of its initial box."""

import math

from . import _lib
from .state import Box

_FIELDS = ("Lx", "Ly", "Lz", "xy", "xz", "yz")


def _numbers(box):
    return tuple(getattr(box, f) for f in _FIELDS)


class BoxVariant:
    """Base of the box variants: ``v(timestep)`` is a ``state.Box``."""

    def __call__(self, timestep):
        raise NotImplementedError

    def __ne__(self, other):
        return not self == other

    __hash__ = object.__hash__


class Constant(BoxVariant):
    """``hoomd.variant.box.Constant``: ``box`` at every timestep."""

    def __init__(self, box):
        self.box = Box.from_box(box)

    def __call__(self, timestep):
        return self.box

    def __eq__(self, other):
        return isinstance(other, Constant) and other.box == self.box

    def __repr__(self):
        return "variant.box.Constant(%r)" % (self.box,)


class Interpolate(BoxVariant):
    """``hoomd.variant.box.Interpolate``: between ``initial_box`` and ``final_box`` as the scalar ``variant`` goes from
    its ``min`` to its ``max``: with ``s = (variant(t) - min) / (max - min)`` (0 where ``max == min``) each of Lx, Ly,
    Lz, xy, xz, yz is ``a (1 - s) + b s``. The two boxes must have the same periodic flags."""

    def __init__(self, initial_box, final_box, variant):
        self.initial_box, self.final_box = Box.from_box(initial_box), Box.from_box(final_box)
        if self.initial_box.periodic != self.final_box.periodic:
            raise _lib.AzpError("variant.box.Interpolate: the periodic flags of the two boxes differ (%r, %r): a box resize "
                                "cannot change them" % (self.initial_box.periodic, self.final_box.periodic))
        if not (callable(variant) and hasattr(variant, "min") and hasattr(variant, "max")):
            raise _lib.AzpError("variant.box.Interpolate: variant must be a scalar variant (azplugins_amd.variant), got %r" % (variant,))
        self.variant = variant

    def scale(self, timestep):
        """s in [0, 1] at ``timestep``."""
        lo, hi = float(self.variant.min), float(self.variant.max)
        if hi == lo:
            return 0.0
        return (float(self.variant(timestep)) - lo) / (hi - lo)

    def __call__(self, timestep):
        s = self.scale(timestep)
        a, b = _numbers(self.initial_box), _numbers(self.final_box)
        return Box(*[x * (1.0 - s) + y * s for x, y in zip(a, b)], periodic=self.initial_box.periodic)

    def __eq__(self, other):
        return (isinstance(other, Interpolate) and other.initial_box == self.initial_box and other.final_box == self.final_box
                and other.variant == self.variant)

    def __repr__(self):
        return "variant.box.Interpolate(%r, %r, %r)" % (self.initial_box, self.final_box, self.variant)


class InverseVolumeRamp(BoxVariant):
    """``hoomd.variant.box.InverseVolumeRamp``: 1 / V goes linearly in the timestep from 1 / V0 (the volume of
    ``initial_box``) at ``t_start`` to 1 / ``final_volume`` at ``t_start + t_ramp`` and is constant outside the ramp (the
    density of a fixed number of particles rises linearly). The three edges are scaled by (V / V0)^(1/3); the tilt factors
    do not change. 3-D boxes only."""

    def __init__(self, initial_box, final_volume, t_start, t_ramp):
        self.initial_box = Box.from_box(initial_box)
        self.final_volume = float(final_volume)
        v0 = self.initial_box.volume
        if not (math.isfinite(self.final_volume) and self.final_volume > 0.0 and math.isfinite(v0) and v0 > 0.0):
            raise _lib.AzpError("variant.box.InverseVolumeRamp: the volumes must be positive and finite (a 3-D box), got "
                                "%r and %r" % (v0, final_volume))
        for name, v, least in (("t_start", t_start, 0), ("t_ramp", t_ramp, 1)):
            if isinstance(v, bool) or int(v) != v or int(v) < least:
                raise _lib.AzpError("variant.box.InverseVolumeRamp: %s must be an integer >= %d, got %r" % (name, least, v))
        self.t_start, self.t_ramp = int(t_start), int(t_ramp)

    def volume(self, timestep):
        """V at ``timestep``."""
        t = int(timestep)
        v0 = self.initial_box.volume
        if t <= self.t_start:
            return v0
        if t >= self.t_start + self.t_ramp:
            return self.final_volume
        s = (t - self.t_start) / self.t_ramp
        return 1.0 / ((1.0 - s) / v0 + s / self.final_volume)

    def __call__(self, timestep):
        b = self.initial_box
        f = (self.volume(timestep) / b.volume) ** (1.0 / 3.0)
        return Box(b.Lx * f, b.Ly * f, b.Lz * f, b.xy, b.xz, b.yz, periodic=b.periodic)

    def __eq__(self, other):
        return (isinstance(other, InverseVolumeRamp) and other.initial_box == self.initial_box
                and (other.final_volume, other.t_start, other.t_ramp) == (self.final_volume, self.t_start, self.t_ramp))

    def __repr__(self):
        return "variant.box.InverseVolumeRamp(%r, final_volume=%r, t_start=%r, t_ramp=%r)" % (
            self.initial_box, self.final_volume, self.t_start, self.t_ramp)


__all__ = ["BoxVariant", "Constant", "Interpolate", "InverseVolumeRamp"]
