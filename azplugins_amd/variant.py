"""``hoomd.azplugins.variant``: quantities that change with the timestep. ``SphereArea`` is the radius of a droplet
whose surface area shrinks at a constant rate (src/VariantSphereArea.{h,cc}); it is a callable of the timestep, which
is what ``external.SphericalHarmonicBarrier(location=...)`` takes."""

import math

from . import _lib


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
