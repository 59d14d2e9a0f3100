"""The base of the bond, angle and dihedral force classes: per-type ``params``, the parameter rows on the device and
the launch over the ``State``'s per-particle table of that kind (``csrc/bonded_kernel.hpp``)."""

import ctypes as C

import numpy as np

from . import _lib
from .force import Force, TypeParameter


def table_param_rows(who, device, types, tables, refused):
    """The device side of a tabulated bonded potential (``bond.Table``, ``angle.Table``, ``dihedral.Table``), from one
    ``(lo, hi, U, F)`` per type -- samples at both ends of ``[lo, hi]`` and at equal steps in between, ``lo >= 0``.
    ``azp_table_pack(closed = 1)`` makes each type's rows; the rows of all types go into ONE device tensor (32-byte
    aligned, one spare row at the end) and each type's ``azp_table_params`` points at its first row. Returns that
    tensor, which the caller keeps alive, and the structs as float64 words (``len(types)`` x 4). ``refused``: what to
    say of a table the library does not take."""
    import torch

    packed = []
    for t, (lo, hi, U, F) in zip(types, tables):
        rows = _lib.table_pack(lo, hi, U, F, closed=True)
        if rows is None:
            raise _lib.AzpError("%s.params[%r]: %s" % (who, t, refused))
        packed.append(rows)
    dev_rows = torch.from_numpy(np.concatenate(packed + [np.zeros((1, 4))])).to(device)
    assert dev_rows.data_ptr() % 32 == 0
    entries, first = [], 0
    for (lo, hi, _, _), rows in zip(tables, packed):
        entries.append((lo, hi, dev_rows.data_ptr() + 32 * first, len(rows)))
        first += len(rows)
    return dev_rows, _lib.table_params_rows(entries)


class BondedTable:
    """Mixin of ``angle.Table`` and ``dihedral.Table``: ``params[type] = dict(U=array, tau=array)`` over the whole
    domain ``_domain`` of the angle (what the kernel's evaluator reads the table over, starting at 0), through
    ``table_param_rows``. There is no ``_azplugins`` class behind it: ``params[...]`` hands back what was set."""

    _domain = None  # (0, upper limit of the table coordinate)

    def _rows(self, types, values):
        lo, hi = self._domain
        self._table_rows, params = table_param_rows(type(self).__name__, self._state.device, types,
                                                    [(lo, hi, d["U"], d["tau"]) for d in values],
                                                    "needs at least 2 finite samples in U and tau")
        return params


class BondedForce(Force):
    """``params[type] = dict(...)`` per group type; ``block_size``: 0 (256) or 64, 128, 256.

    A kind declares ``_kind`` ("bond", "angle", "dihedral" or "pair": the ``State`` group it reads, its ``_lib`` argument struct
    and that struct's table, count and type-number fields all carry the name) and ``_param_doubles``; a potential
    declares ``_entry``, ``_schema``, ``_pack`` and ``_unpack`` and, to range-check what is set, ``_parameter``."""

    _kind = None
    _args_struct = None    # the ``_lib`` struct where it is not ``<Kind>Args`` (special pairs: ``PairArgs`` is taken)
    _entry = None
    _schema = None
    _parameter = TypeParameter
    _param_doubles = None  # one type's parameter row in float64 words
    _readback = None       # (Bond: params[...] reads back what the C++ object holds)

    def __init__(self):
        super().__init__()
        self.params = self._parameter("params", self._schema, 1, self._mark_dirty, self._readback)
        self._tables = None
        self.block_size = 0

    def _mark_dirty(self):
        self._tables = None

    def _attach(self, sim):
        super()._attach(sim)
        self._tables = None

    def _pack(self, d):
        """One type's dict folded into its parameter row by libazp (``_param_doubles`` float64 words)."""
        raise NotImplementedError

    def _unpack(self, raw):
        raise NotImplementedError

    def _types(self):
        return getattr(self._state, self._kind + "_types")

    def _rows(self, types, values):
        raw = np.zeros((max(len(types), 1), self._param_doubles))
        for i, d in enumerate(values):
            raw[i] = self._pack(d)
        return raw

    def _build_tables(self):
        import torch

        types = self._types()
        values = [self.params.get_raw(t) for t in types]
        for t, d in zip(types, values):
            if d is None:
                raise _lib.AzpError("%s.params[%r] is not set" % (type(self).__name__, t))
        self._tables = torch.from_numpy(self._rows(types, values)).to(self._state.device)

    def _launch(self, args, stream):
        fn = getattr(_lib.lib(), self._entry)
        _lib.check(fn(C.byref(args), self._tables.data_ptr(), stream), self._entry)

    def compute(self, timestep=None):
        self._require()
        st = self._state
        kind = self._kind
        self._ensure_buffers()
        n_types = max(len(self._types()), 1)
        if self._tables is None or self._tables.shape[0] != n_types:
            self._build_tables()
        tab = getattr(st, kind + "_table")()
        a = getattr(_lib, self._args_struct or kind.capitalize() + "Args")()
        a.d_force = self._force.data_ptr()
        a.d_virial = self._virial.data_ptr()
        a.virial_pitch = st.N
        a.N = st.N
        a.n_max = st.n_max
        a.d_pos = st.pos.data_ptr()
        a.box = st.box.to_c()
        setattr(a, "d_gpu_%slist" % kind, tab["table"].data_ptr())
        if "bond_pos" in tab:
            setattr(a, "d_gpu_%s_pos" % kind, tab["bond_pos"].data_ptr())
        setattr(a, "d_gpu_n_%ss" % kind, tab["n_%ss" % kind].data_ptr())
        a.pitch = tab["pitch"]
        setattr(a, "n_%s_types" % kind, n_types)
        a.compute_virial = 1 if self.compute_virial else 0
        a.block_size = self.block_size
        self._launch(a, _lib.raw_stream(st.device))
