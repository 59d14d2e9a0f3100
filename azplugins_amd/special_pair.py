"""Special pair potentials: interactions between listed pairs of particles (``Snapshot.pairs``, HOOMD's
``hoomd.md.special_pair``) on libazp's gfx950 special-pair kernel (``csrc/special_pair_forces.hip``).

A force field that excludes the 1-4 pairs of its chains from the non-bonded interactions
(``nlist.Cell(exclusions=("bond", "1-3", "1-4"))``) usually puts them back with scaled parameters: OPLS with half the
Lennard-Jones energy. Those pairs are listed as special pairs, with a type each, and evaluated here.

The reference holds no such code, so the semantics are DEFINED HERE and in ``include/azp.h``, under
``md.special_pair``'s class name and parameter keys. With ``r`` the minimum-image distance of the two members:

* ``LJ``: ``U = 4 epsilon [(sigma / r)^12 - (sigma / r)^6]`` for ``r < r_cut``, 0 otherwise. There is no shift: ``U``
  jumps at ``r_cut``.

Each member gets the force on itself, half of ``U`` and, with ``compute_virial``, half of the pair's virial: one lane
per particle and no atomics, like a bond; ``compute.ThermodynamicQuantities`` sums it like any other force. Special
pairs exclude nothing by themselves: name ``"special_pair"`` (or ``"1-4"``) in the neighbor list's ``exclusions``.

Out of scope: ``special_pair.Coulomb`` (a ``State`` has no charges), an ``_azplugins`` class."""

import ctypes as C
import math

import numpy as np

from . import _lib
from .bonded import BondedForce
from .force import TypeParameter


class _LJParameter(TypeParameter):
    """``TypeParameter`` whose values are also range-checked when they are set."""

    def _validate(self, value):
        out = super()._validate(value)
        for key in ("epsilon", "sigma"):
            if not math.isfinite(out[key]):
                raise ValueError("%s: %s must be finite, got %r" % (self.name, key, out[key]))
        if out["sigma"] < 0.0:
            raise ValueError("%s: sigma must not be negative, got %r" % (self.name, out["sigma"]))
        return out


class _CutoffParameter(TypeParameter):
    """``r_cut[type] = float``: one finite, non-negative cutoff per special-pair type."""

    def _validate(self, value):
        value = float(value)
        if not (math.isfinite(value) and value >= 0.0):
            raise ValueError("%s must be finite and >= 0, got %r" % (self.name, value))
        return value

    def __getitem__(self, key):
        k = self._key(key)
        if k not in self._data:
            raise KeyError("%s[%r] is not set" % (self.name, key))
        return self._data[k]


class SpecialPair(BondedForce):
    """Reduced ``hoomd.md.special_pair.SpecialPair``: per-pair-type ``params`` and ``r_cut``. ``block_size``: 0 (256)
    or 64, 128, 256."""

    _kind = "pair"
    _args_struct = "PairGroupArgs"
    _param_doubles = 4

    def __init__(self):
        super().__init__()
        self.r_cut = _CutoffParameter("r_cut", {}, 1, self._mark_dirty)

    def _build_tables(self):
        for t in self._types():
            if self.r_cut.get_raw(t) is None:
                raise _lib.AzpError("%s.r_cut[%r] is not set" % (type(self).__name__, t))
        super()._build_tables()

    def _rows(self, types, values):
        raw = np.zeros((max(len(types), 1), self._param_doubles))
        for i, (t, d) in enumerate(zip(types, values)):
            raw[i] = self._pack(dict(d, r_cut=self.r_cut[t]))
        return raw


class LJ(SpecialPair):
    """Lennard-Jones special pair ``U = 4 epsilon [(sigma / r)^12 - (sigma / r)^6]`` for ``r < r_cut``, 0 otherwise, not
    shifted (HOOMD ``md.special_pair.LJ``). ``params[type] = dict(epsilon, sigma)`` (finite, ``sigma >= 0``) and
    ``r_cut[type] = float``; both must be set for every special-pair type of the state."""

    _entry = "azp_special_pair_forces_lj"
    _schema = dict(epsilon=float, sigma=float)
    _parameter = _LJParameter

    def _pack(self, d):
        out = np.zeros(4)
        _lib.lib().azp_special_pair_lj_params_make(d["epsilon"], d["sigma"], d["r_cut"], out.ctypes.data)
        return out

    def _unpack(self, raw):
        raw = np.ascontiguousarray(raw, dtype=np.float64)
        v = [C.c_double() for _ in range(3)]
        _lib.lib().azp_special_pair_lj_params_unpack(raw.ctypes.data, *[C.byref(x) for x in v])
        return dict(epsilon=v[0].value, sigma=v[1].value, r_cut=v[2].value)


__all__ = ["SpecialPair", "LJ"]
