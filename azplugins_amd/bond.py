"""Bond potentials: drop-in mirror of ``hoomd.azplugins.bond`` (reference
``src/bond.py``) on libazp's gfx950 bond kernel."""

import ctypes as C

import numpy as np

from . import _lib
from .bonded import BondedForce, table_param_rows
from .force import TableTypeParameter


class Bond(BondedForce):
    """Reduced ``hoomd.md.bond.Bond``: per-bond-type ``params``. Its own, around the shared launch: the ``_azplugins``
    C++ object as the source of the parameter bytes and of what ``params[...]`` reads back, and the flag word of an
    evaluator that rejected its parameters."""

    _kind = "bond"
    _cpp_class_name = None
    _param_doubles = 4

    def _readback(self, key):
        """After attaching, ``params[...]`` returns what the C++ object holds (HOOMD:
        getParams -> asDict; src/pytest/test_bond.py:223)."""
        if not self._attached or key not in self.params._data:
            return None
        self._sync_cpp()
        return dict(self._cpp.getParams(key))

    def _attach(self, sim):
        import torch

        super()._attach(sim)
        self._cpp = None
        self._flags = torch.zeros(1, dtype=torch.int32, device=self._state.device)

    def _sync_cpp(self):
        """The ``_azplugins`` C++ object (class name + "GPU") with the current parameters."""
        types = list(self._state.bond_types) or ["A-A"]
        if getattr(self, "_cpp", None) is None:
            self._cpp = getattr(_lib.ext_module(), self._cpp_class_name + "GPU")(types)
        for t in self._state.bond_types:
            d = self.params.get_raw(t)
            if d is not None:
                self._cpp.setParams(t, d)

    def _rows(self, types, values):
        self._sync_cpp()
        raw = np.frombuffer(self._cpp.params_bytes(), dtype=np.float64).reshape(max(len(types), 1), -1).copy()
        assert raw.shape[1] == self._param_doubles
        return raw

    def _build_tables(self):
        super()._build_tables()
        self._flags.zero_()  # (new parameters: the sticky "rejected" flag starts over, on the device and on the host)
        self._flag_pending = None
        if getattr(self, "_flag_host", None) is not None:
            getattr(self, "_flag_side").synchronize()
            self._flag_host.zero_()

    def _launch(self, args, stream):
        import torch

        # The evaluator's "rejected its parameters" flag (HOOMD: "bond.<name>: bond out of bounds") is sticky on the
        # device (the kernel only ever sets it) and travels to the host on a side stream behind each launch; it is
        # LOOKED AT when the next launch is queued, by which time it has long arrived -- a readback right behind
        # the launch would idle the GPU for a host round trip every step. check_flags() looks now.
        self.check_flags(wait=False)
        fn = getattr(_lib.lib(), self._entry)
        _lib.check(fn(C.byref(args), self._tables.data_ptr(), self._flags.data_ptr(), stream), self._entry)
        if getattr(self, "_flag_side", None) is None:
            self._flag_side = torch.cuda.Stream(device=self._state.device)
            self._flag_host = torch.zeros(1, dtype=torch.int32).pin_memory()
        done = torch.cuda.Event()
        done.record()
        with torch.cuda.stream(self._flag_side):
            self._flag_side.wait_event(done)
            self._flag_host.copy_(self._flags, non_blocking=True)
        self._flag_pending = torch.cuda.Event()
        self._flag_pending.record(self._flag_side)
        if not self.defer_flag_check:
            self.check_flags(wait=True)

    defer_flag_check = False  # True inside Simulation.run: the flag of step k is examined when step k + 1 is queued

    def check_flags(self, wait=True):
        """Raise if an evaluator rejected its parameters in a launch whose flag has reached the host
        (``wait=True``: of every launch so far)."""
        ev = getattr(self, "_flag_pending", None)
        if ev is None:
            return
        if wait:
            ev.synchronize()
        elif not ev.query():
            return
        if int(self._flag_host[0]) != 0:
            # HOOMD: "bond.<name>: bond out of bounds" when the evaluator returns false
            raise _lib.AzpError("bond.%s: bond out of bounds (evaluator rejected its parameters)" % type(self).__name__)


class DoubleWell(Bond):
    """Double well bond potential (reference ``src/bond.py:13-65``)."""

    _cpp_class_name = "PotentialBondDoubleWell"
    _entry = "azp_bond_forces_double_well"
    _schema = dict(r_0=float, r_1=float, U_1=float, U_tilt=float)

    def _pack(self, d):
        out = np.zeros(4)
        _lib.lib().azp_dw_params_make(d["r_0"], d["r_1"], d["U_1"], d["U_tilt"], out.ctypes.data)
        return out

    def _unpack(self, raw):
        v = [C.c_double() for _ in range(4)]
        _lib.lib().azp_dw_params_unpack(raw.ctypes.data, *[C.byref(x) for x in v])
        return dict(r_0=v[0].value, r_1=v[1].value, U_1=v[2].value, U_tilt=v[3].value)


class Quartic(Bond):
    """Quartic bond potential (reference ``src/bond.py:68-157``; ``delta``
    defaults to 0, ``src/bond.py:153``)."""

    _cpp_class_name = "PotentialBondQuartic"
    _entry = "azp_bond_forces_quartic"
    _schema = dict(k=float, r_0=float, b_1=float, b_2=float, U_0=float, sigma=float, epsilon=float, delta=0.0)
    _param_doubles = 8

    def _pack(self, d):
        out = np.zeros(8)
        _lib.lib().azp_quartic_params_make(d["k"], d["r_0"], d["b_1"], d["b_2"], d["U_0"], d["sigma"], d["epsilon"],
                                           d["delta"], out.ctypes.data)
        return out

    def _unpack(self, raw):
        v = [C.c_double() for _ in range(8)]
        _lib.lib().azp_quartic_params_unpack(raw.ctypes.data, *[C.byref(x) for x in v])
        keys = ("k", "r_0", "b_1", "b_2", "U_0", "sigma", "epsilon", "delta")
        return {k: x.value for k, x in zip(keys, v)}


class Table(Bond):
    """Tabulated bond potential (``hoomd.md.bond.Table``'s name; the reference has none, the semantics are defined in
    ``include/azp.h`` and DESIGN 4.21). ``params[type] = dict(r_min=float, r_max=float, U=array, F=array)``:
    ``width = len(U) >= 2`` samples of the energy and of ``F = -dU/dr`` at ``r_min + k (r_max - r_min) / (width - 1)``,
    both end points included, interpolated linearly in between. A bond shorter than ``r_min`` or of length ``r_max`` or
    more is an error ("bond out of bounds"), found by the kernel before it reads the table.

    There is no ``_azplugins`` class behind it: the tables of all bond types live in one device tensor this object owns."""

    _entry = "azp_bond_forces_table"
    _schema = dict(r_min=float, r_max=float, U=np.ndarray, F=np.ndarray)
    _parameter = TableTypeParameter

    def _readback(self, key):
        return None  # (params[...] hands back what was set: there is no C++ object that could hold anything else)

    def _rows(self, types, values):
        self._table_rows, params = table_param_rows(type(self).__name__, self._state.device, types,
                                                    [(d["r_min"], d["r_max"], d["U"], d["F"]) for d in values],
                                                    "needs 0 <= r_min < r_max and at least 2 finite samples in U and F")
        return params


__all__ = ["DoubleWell", "Quartic", "Table"]
