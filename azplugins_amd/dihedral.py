"""Dihedral potentials: periodic, OPLS and tabulated torsions on libazp's gfx950 dihedral kernel
(``csrc/dihedral_forces.hip``).

The reference holds no dihedral code (with HOOMD-blue, torsions come from ``hoomd.md.dihedral`` next to the plugin), so
the semantics are DEFINED HERE and in ``include/azp.h``, under ``md.dihedral``'s class names and
parameter keys.

A dihedral has members ``a, b, c, d`` (``Snapshot.dihedrals.group``). With ``b1 = r_b - r_a``, ``b2 = r_c - r_b``,
``b3 = r_d - r_c`` (minimum image), ``n1 = b1 x b2`` and ``n2 = b2 x b3``, the angle is
``phi = atan2(|b2| (b1 . n2), n1 . n2)`` in (-pi, pi]: IUPAC, cis (``a`` eclipsing ``d``) is 0 and trans is pi.

* ``Periodic``: ``U = 1/2 k (1 + d cos(n phi - phi0))``;
* ``OPLS``: ``U = 1/2 [k1 (1 + cos phi) + k2 (1 - cos 2 phi) + k3 (1 + cos 3 phi) + k4 (1 - cos 4 phi)]``;
* ``Table``: ``U`` and the torque ``tau = -dU/dphi`` sampled at equal steps of ``phi`` over [-pi, pi] and interpolated
  linearly.

``F_m = -U'(phi) g_m`` with the gradient of ``phi`` in the Blondel-Karplus form, which has no ``1 / sin phi``:
``g_a = -(|b2| / |n1|^2) n1``, ``g_d = (|b2| / |n2|^2) n2``, ``g_b = -(1 + s) g_a + t g_d``,
``g_c = -(1 + t) g_d + s g_a`` with ``s = b1 . b2 / |b2|^2`` and ``t = b3 . b2 / |b2|^2``. Every member gets a quarter
of ``U`` and, with ``compute_virial``, a quarter of ``(-b1) (x) F_a + b2 (x) F_c + (b2 + b3) (x) F_d`` (zero trace).
``a, b, c`` or ``b, c, d`` collinear (``|n1|`` or ``|n2|`` equal to 0) and coincident members are undefined. Dihedrals
add no neighbor-list exclusions by themselves: ``nlist.Cell(exclusions=("bond", "1-3", "1-4"))`` excludes the 1-4
pairs and ``special_pair.LJ`` puts them back scaled.

Out of scope: impropers, ``special_pair.Coulomb`` (no charges), an ``_azplugins`` class."""

import ctypes as C
import math

import numpy as np

from . import _lib
from .bonded import BondedForce, BondedTable
from .force import BondedTableTypeParameter, TypeParameter


class Dihedral(BondedForce):
    """Reduced ``hoomd.md.dihedral.Dihedral``: per-dihedral-type ``params``. ``block_size``: 0 (256) or 64, 128, 256.
    One type's parameter row is 32 bytes, handled as four float64 words."""

    _kind = "dihedral"
    _param_doubles = 4


class _PeriodicParameter(TypeParameter):
    """``TypeParameter`` whose values are also range-checked when they are set."""

    def _validate(self, value):
        out = super()._validate(value)
        for key in ("k", "phi0"):
            if not math.isfinite(out[key]):
                raise ValueError("%s: %s must be finite, got %r" % (self.name, key, out[key]))
        if out["d"] not in (1.0, -1.0):
            raise ValueError("%s: d must be +1 or -1, got %r" % (self.name, out["d"]))
        if not (out["n"] >= 1.0 and out["n"] == int(out["n"])):  # (false for a NaN too)
            raise ValueError("%s: n must be an integer >= 1, got %r" % (self.name, out["n"]))
        out["d"], out["n"] = int(out["d"]), int(out["n"])
        return out


class _OPLSParameter(TypeParameter):
    def _validate(self, value):
        out = super()._validate(value)
        for key, v in out.items():
            if not math.isfinite(v):
                raise ValueError("%s: %s must be finite, got %r" % (self.name, key, v))
        return out


class Periodic(Dihedral):
    """Periodic torsion ``U = 1/2 k (1 + d cos(n phi - phi0))`` (HOOMD ``md.dihedral.Periodic``).
    ``params[type] = dict(k, d, n, phi0)``: ``k`` and ``phi0`` (radians) finite, ``d`` +1 or -1, ``n`` an integer >= 1;
    ``cos phi0`` and ``sin phi0`` are folded on the host."""

    _entry = "azp_dihedral_forces_periodic"
    _schema = dict(k=float, d=float, n=float, phi0=float)
    _parameter = _PeriodicParameter

    def _pack(self, d):
        out = np.zeros(4)
        _lib.lib().azp_dihedral_periodic_params_make(d["k"], d["d"], d["n"], d["phi0"], out.ctypes.data)
        return out

    def _unpack(self, raw):
        raw = np.ascontiguousarray(raw, dtype=np.float64)
        k, phi0, d, n = C.c_double(), C.c_double(), C.c_int(), C.c_uint()
        _lib.lib().azp_dihedral_periodic_params_unpack(raw.ctypes.data, C.byref(k), C.byref(d), C.byref(n), C.byref(phi0))
        return dict(k=k.value, d=d.value, n=n.value, phi0=phi0.value)


class OPLS(Dihedral):
    """OPLS torsion ``U = 1/2 [k1 (1 + cos phi) + k2 (1 - cos 2 phi) + k3 (1 + cos 3 phi) + k4 (1 - cos 4 phi)]``
    (HOOMD ``md.dihedral.OPLS``). ``params[type] = dict(k1, k2, k3, k4)``, all finite."""

    _entry = "azp_dihedral_forces_opls"
    _schema = dict(k1=float, k2=float, k3=float, k4=float)
    _parameter = _OPLSParameter

    def _pack(self, d):
        out = np.zeros(4)
        _lib.lib().azp_dihedral_opls_params_make(d["k1"], d["k2"], d["k3"], d["k4"], out.ctypes.data)
        return out

    def _unpack(self, raw):
        raw = np.ascontiguousarray(raw, dtype=np.float64)
        k = [C.c_double() for _ in range(4)]
        _lib.lib().azp_dihedral_opls_params_unpack(raw.ctypes.data, *[C.byref(x) for x in k])
        return dict(k1=k[0].value, k2=k[1].value, k3=k[2].value, k4=k[3].value)


class Table(BondedTable, Dihedral):
    """Tabulated torsion (``hoomd.md.dihedral.Table``'s name; the reference has none, the semantics are defined in
    ``include/azp.h`` and DESIGN 4.26). ``params[type] = dict(U=array, tau=array)``: ``width = len(U) >= 2`` samples of
    the energy and of the torque ``tau = -dU/dphi`` at ``phi_k = -pi + 2 pi k / (width - 1)``, both end points
    included, interpolated linearly in between. ``width`` is per type.

    Periodicity is not enforced: ``U[0]`` may differ from ``U[-1]``. A planar trans dihedral reads the end its
    ``sin phi`` names: ``sin phi = +0`` is ``phi = +pi`` and reads ``U[-1]``, ``tau[-1]``; ``sin phi = -0`` is
    ``phi = -pi`` and reads ``U[0]``, ``tau[0]``. A table that is meant to be periodic stores equal ends. The rows are
    kept over ``phi + pi`` in [0, 2 pi]."""

    _entry = "azp_dihedral_forces_table"
    _schema = dict(U=np.ndarray, tau=np.ndarray)
    _parameter = BondedTableTypeParameter
    _domain = (0.0, 2.0 * math.pi)


__all__ = ["Dihedral", "Periodic", "OPLS", "Table"]
