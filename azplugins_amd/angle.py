"""Angle potentials: harmonic, cosine-squared and tabulated bending on libazp's gfx950 angle kernel
(``csrc/angle_forces.hip``).

The reference holds no angle code (with HOOMD-blue, bending stiffness comes from ``hoomd.md.angle`` next to the
plugin), so the semantics are DEFINED HERE and in ``include/azp.h``: HOOMD's documented
``md.angle.Harmonic`` and ``md.angle.CosineSquared`` conventions.

An angle has members ``a, b, c`` with ``b`` the vertex (``Snapshot.angles.group``). With ``dab = r_a - r_b`` and
``dcb = r_c - r_b`` (minimum image), ``c = dab.dcb / (|dab||dcb|)`` clamped to [-1, 1] and
``s = max(sqrt(1 - c^2), 1e-3)`` (HOOMD's floor):

* ``Harmonic``: ``U = 1/2 k (theta - t0)^2`` with ``theta = acos(c)``, ``dU/dc = -k (theta - t0) / s``;
* ``CosineSquared``: ``U = 1/2 k (c - cos t0)^2``, ``dU/dc = k (c - cos t0)``;
* ``Table``: ``U`` and the torque ``tau = -dU/dtheta`` sampled at equal steps of ``theta = acos(c)`` over [0, pi] and
  interpolated linearly, ``dU/dc = tau / s``.

``F_a = -dU/dc (dcb / (|dab||dcb|) - c dab / |dab|^2)``, ``F_c`` likewise with a and c exchanged, ``F_b = -F_a - F_c``.
Every member gets a third of ``U`` and, with ``compute_virial``, a third of ``dab (x) F_a + dcb (x) F_c``. Coincident
members (``|dab|`` or ``|dcb|`` equal to 0) are undefined. Angles add no neighbor-list exclusions by themselves:
``nlist.Cell(exclusions=("bond", "angle"))`` or ``"1-3"`` does.

Out of scope: impropers, an ``_azplugins`` class."""

import ctypes as C
import math

import numpy as np

from . import _lib
from .bonded import BondedForce, BondedTable
from .force import BondedTableTypeParameter, TypeParameter


class _AngleParameter(TypeParameter):
    """``TypeParameter`` whose values are also range-checked when they are set."""

    def _validate(self, value):
        out = super()._validate(value)
        if not math.isfinite(out["k"]):
            raise ValueError("%s: k must be finite, got %r" % (self.name, out["k"]))
        if not 0.0 <= out["t0"] <= math.pi:  # (false for a NaN too)
            raise ValueError("%s: t0 must lie in [0, pi], got %r" % (self.name, out["t0"]))
        return out


class Angle(BondedForce):
    """Reduced ``hoomd.md.angle.Angle``: per-angle-type ``params``. ``block_size``: 0 (256) or 64, 128, 256."""

    _kind = "angle"
    _make = None
    _unpack_entry = None
    _schema = dict(k=float, t0=float)
    _parameter = _AngleParameter
    _param_doubles = 2
    _cpp_class_name = None  # the reference's module.cc registers no angle class

    def _pack(self, d):
        """One type's dict folded into its two doubles by libazp."""
        out = np.zeros(2)
        getattr(_lib.lib(), self._make)(d["k"], d["t0"], out.ctypes.data)
        return out

    def _unpack(self, raw):
        raw = np.ascontiguousarray(raw, dtype=np.float64)
        k, t0 = C.c_double(), C.c_double()
        getattr(_lib.lib(), self._unpack_entry)(raw.ctypes.data, C.byref(k), C.byref(t0))
        return dict(k=k.value, t0=t0.value)


class Harmonic(Angle):
    """Harmonic angle potential ``U = 1/2 k (theta - t0)^2`` (HOOMD ``md.angle.Harmonic``).
    ``params[type] = dict(k, t0)``, ``k`` finite, ``0 <= t0 <= pi`` (radians)."""

    _entry = "azp_angle_forces_harmonic"
    _make = "azp_angle_harmonic_params_make"
    _unpack_entry = "azp_angle_harmonic_params_unpack"


class CosineSquared(Angle):
    """Cosine-squared angle potential ``U = 1/2 k (cos theta - cos t0)^2`` (HOOMD ``md.angle.CosineSquared``).
    ``params[type] = dict(k, t0)``, ``k`` finite, ``0 <= t0 <= pi`` (radians); ``cos t0`` is folded on the host."""

    _entry = "azp_angle_forces_cosine_squared"
    _make = "azp_angle_cossq_params_make"
    _unpack_entry = "azp_angle_cossq_params_unpack"


class Table(BondedTable, Angle):
    """Tabulated angle potential (``hoomd.md.angle.Table``'s name; the reference has none, the semantics are defined in
    ``include/azp.h`` and DESIGN 4.26). ``params[type] = dict(U=array, tau=array)``: ``width = len(U) >= 2`` samples of
    the energy and of the torque ``tau = -dU/dtheta`` at ``theta_k = k pi / (width - 1)``, both end points included,
    interpolated linearly in between. ``width`` is per type. [0, pi] is the whole domain of ``theta``: no angle is out
    of bounds. ``tau`` is what the user supplies, not a derivative of the interpolated ``U``: the energy is conserved
    to the accuracy of the table, not to rounding."""

    _entry = "azp_angle_forces_table"
    _schema = dict(U=np.ndarray, tau=np.ndarray)
    _parameter = BondedTableTypeParameter
    _param_doubles = 4
    _domain = (0.0, math.pi)


__all__ = ["Angle", "Harmonic", "CosineSquared", "Table"]
