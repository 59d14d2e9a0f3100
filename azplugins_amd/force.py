"""Common base of the force classes: per-type parameter dictionaries and the
per-particle result arrays HOOMD's ``Force`` exposes (``forces``, ``energies``,
``torques``, ``virials``, ``energy``)."""

import numpy as np

from . import _lib


class TypeParameter:
    """``hoomd.data.typeparam.TypeParameter`` + ``TypeParameterDict`` reduced to
    what the reference's pair/bond classes use: a dict keyed by a type name
    (``len_keys=1``) or an unordered pair of type names (``len_keys=2``) whose
    values are validated against a schema ``{key: type | default}``."""

    def __init__(self, name, schema, len_keys, on_change=None, readback=None):
        self.name = name
        self.schema = dict(schema)
        self.len_keys = len_keys
        self._data = {}
        self._on_change = on_change
        self._readback = readback

    def _key(self, key):
        if self.len_keys == 1:
            if not isinstance(key, str):
                raise KeyError("%s keys are single type names, got %r" % (self.name, key))
            return key
        if not (isinstance(key, (tuple, list)) and len(key) == 2 and all(isinstance(k, str) for k in key)):
            raise KeyError("%s keys are pairs of type names, got %r" % (self.name, key))
        return tuple(sorted(key))

    def _validate(self, value):
        if not isinstance(self.schema, dict) or not self.schema:
            return value
        if not isinstance(value, dict):
            raise TypeError("%s values must be dicts" % self.name)
        unknown = set(value) - set(self.schema)
        if unknown:
            raise ValueError("%s: unknown keys %s (expected %s)" % (self.name, sorted(unknown), sorted(self.schema)))
        out = {}
        for k, spec in self.schema.items():
            if k in value:
                typ = spec if isinstance(spec, type) else type(spec)
                try:
                    out[k] = typ(value[k])
                except (TypeError, ValueError):
                    raise TypeError("%s[%r] must be convertible to %s" % (self.name, k, typ.__name__))
            elif isinstance(spec, type):
                raise ValueError("%s: missing required key %r" % (self.name, k))
            else:
                out[k] = spec
        return out

    def __setitem__(self, key, value):
        self._data[self._key(key)] = self._validate(value)
        if self._on_change:
            self._on_change()

    def __getitem__(self, key):
        k = self._key(key)
        if self._readback is not None:
            rb = self._readback(k)
            if rb is not None:
                return _ParamView(self, k, rb)
        if k not in self._data:
            # HOOMD hands out a (partially filled) dict for a type that has no
            # parameters yet, e.g. ``barrier.params["A"].update(...)``
            return _ParamView(self, k, {})
        return _ParamView(self, k, self._data[k]) if isinstance(self._data[k], dict) else self._data[k]

    def __contains__(self, key):
        return self._key(key) in self._data

    def keys(self):
        return self._data.keys()

    def get_raw(self, key, default=None):
        return self._data.get(self._key(key), default)


class _ParamView(dict):
    """dict returned by ``params[key]``; ``update`` / item assignment write through
    (with validation), as HOOMD's TypeParameterDict entries do."""

    def __init__(self, owner, key, values):
        super().__init__(values)
        self._owner = owner
        self._key_ = key

    def update(self, *args, **kwargs):
        merged = dict(self)
        merged.update(*args, **kwargs)
        self._owner[self._key_] = merged
        super().update(self._owner._data[self._owner._key(self._key_)])

    def __setitem__(self, k, v):
        self.update({k: v})


class TableTypeParameter(TypeParameter):
    """``params`` of the tabulated potentials (``pair.Table``, ``bond.Table``): ``r_min``, for bonds ``r_max``, and the
    samples ``U`` and ``F = -dU/dr`` as equally long one-dimensional arrays. What can be judged when a value is set
    raises ``ValueError`` there: unequal lengths, too few samples, non-finite entries, a range that is empty, and, for
    pairs, a table for ``(b, a)`` that differs from the one set for ``(a, b)`` (both orders name the same rows)."""

    def __init__(self, name, schema, len_keys, on_change=None, readback=None):
        super().__init__(name, schema, len_keys, on_change, readback)
        self.closed = "r_max" in self.schema   # bond form: both end points stored
        self.r_end = None                      # pairs: key -> r_cut, or None while it is not known
        self._set_as = {}                      # the order of the type names each pair's table was set with

    def _validate(self, value):
        if not isinstance(value, dict):
            raise TypeError("%s values must be dicts" % self.name)
        if set(value) != set(self.schema):
            raise ValueError("%s: expected the keys %s, got %s" % (self.name, sorted(self.schema), sorted(value)))
        out = {k: float(value[k]) for k in self.schema if k not in ("U", "F")}
        for k in ("U", "F"):
            out[k] = np.array(value[k], dtype=np.float64)
            if out[k].ndim != 1:
                raise ValueError("%s: %s must be a one-dimensional array" % (self.name, k))
        if out["U"].shape != out["F"].shape:
            raise ValueError("%s: U and F differ in length (%d, %d)" % (self.name, len(out["U"]), len(out["F"])))
        least = 2 if self.closed else 1
        if len(out["U"]) < least:
            raise ValueError("%s: a table needs at least %d samples, got %d" % (self.name, least, len(out["U"])))
        if not (np.isfinite(out["U"]).all() and np.isfinite(out["F"]).all()):
            raise ValueError("%s: U and F must be finite" % self.name)
        if not (np.isfinite(out["r_min"]) and out["r_min"] >= 0.0):
            raise ValueError("%s: r_min must be finite and >= 0, got %r" % (self.name, out["r_min"]))
        if self.closed and not (np.isfinite(out["r_max"]) and out["r_max"] > out["r_min"]):
            raise ValueError("%s: r_max must be finite and > r_min, got %r" % (self.name, out["r_max"]))
        return out

    @staticmethod
    def _same(a, b):
        return all(np.array_equal(a[k], b[k]) for k in a)

    def __setitem__(self, key, value):
        k = self._key(key)
        v = self._validate(value)
        r_end = self.r_end(k) if self.r_end is not None else None
        if r_end is not None and r_end > 0.0 and not v["r_min"] < r_end:
            raise ValueError("%s[%r]: r_min = %g is not below r_cut = %g" % (self.name, key, v["r_min"], r_end))
        as_set = tuple(key) if self.len_keys == 2 else key
        if k in self._data and self._set_as[k] != as_set and not self._same(v, self._data[k]):
            raise ValueError("%s[%r] differs from the table set for %r: both name the same rows" % (self.name, key, self._set_as[k]))
        self._data[k] = v
        self._set_as[k] = as_set
        if self._on_change:
            self._on_change()

    def __getitem__(self, key):
        """What was set, the arrays as copies: a table is replaced as a whole, not edited in place."""
        k = self._key(key)
        if k not in self._data:
            raise KeyError("%s[%r] is not set" % (self.name, key))
        return {name: (v.copy() if isinstance(v, np.ndarray) else v) for name, v in self._data[k].items()}


class BondedTableTypeParameter(TypeParameter):
    """``params`` of the tabulated angle and dihedral potentials (``angle.Table``, ``dihedral.Table``):
    ``dict(U=array, tau=array)``, the energy and the torque ``tau = -dU/d(angle)`` as equally long one-dimensional
    arrays of at least 2 samples over the whole domain of the angle, both end points included. There is no range to
    give. Raises ``ValueError`` where the value is set: other keys than ``U`` and ``tau``, arrays that are not
    one-dimensional, unequal lengths, fewer than 2 samples, non-finite entries."""

    def _validate(self, value):
        if not isinstance(value, dict):
            raise TypeError("%s values must be dicts" % self.name)
        if set(value) != {"U", "tau"}:
            raise ValueError("%s: expected the keys ['U', 'tau'], got %s" % (self.name, sorted(value)))
        try:
            out = {k: np.array(value[k], dtype=np.float64) for k in ("U", "tau")}
        except (TypeError, ValueError):
            raise ValueError("%s: U and tau must be arrays of numbers" % self.name)
        for k, v in out.items():
            if v.ndim != 1:
                raise ValueError("%s: %s must be a one-dimensional array" % (self.name, k))
        if out["U"].shape != out["tau"].shape:
            raise ValueError("%s: U and tau differ in length (%d, %d)" % (self.name, len(out["U"]), len(out["tau"])))
        if len(out["U"]) < 2:
            raise ValueError("%s: a table needs at least 2 samples, got %d" % (self.name, len(out["U"])))
        if not (np.isfinite(out["U"]).all() and np.isfinite(out["tau"]).all()):
            raise ValueError("%s: U and tau must be finite" % self.name)
        return out

    def __getitem__(self, key):
        """What was set, the arrays as copies: a table is replaced as a whole, not edited in place."""
        k = self._key(key)
        if k not in self._data:
            raise KeyError("%s[%r] is not set" % (self.name, key))
        return {name: v.copy() for name, v in self._data[k].items()}


class ScalarTypeParameter(TypeParameter):
    """Per-type-pair scalar (``r_cut`` / ``r_on``) with a default."""

    def __init__(self, name, default, on_change=None):
        super().__init__(name, {}, 2, on_change)
        self.default = default

    def _validate(self, value):
        return float(value)

    def __getitem__(self, key):
        k = self._key(key)
        if k in self._data:
            return self._data[k]
        if self.default is None:
            raise KeyError("%s[%r] is not set and there is no default" % (self.name, key))
        return float(self.default)


class Force:
    """Holds the result buffers of one force compute (HOOMD ``ForceCompute``):
    force (N,4) = (fx, fy, fz, energy), virial (6, N), torque (N,4)."""

    def __init__(self):
        self._state = None
        self._force = None
        self._virial = None
        self._torque = None
        self.compute_virial = False

    @property
    def _attached(self):
        return self._state is not None

    def _attach(self, sim):
        import torch

        self._sim = sim
        self._state = sim.state
        N = self._state.N
        dev = self._state.device
        self._force = torch.zeros((N, 4), dtype=torch.float64, device=dev)
        self._torque = torch.zeros((N, 4), dtype=torch.float64, device=dev)
        self._virial = torch.zeros((6, N), dtype=torch.float64, device=dev)
        self._dirty = True

    def _require(self):
        if not self._attached:
            raise _lib.AzpError("%s is not attached to a simulation; call sim.run(0) first" % type(self).__name__)

    def _ensure_buffers(self):
        """Result buffers follow the number of local particles (it changes when particles
        migrate between the ranks of a decomposed run)."""
        import torch

        N = self._state.N
        if self._force.shape[0] != N:
            dev = self._state.device
            self._force = torch.zeros((N, 4), dtype=torch.float64, device=dev)
            self._torque = torch.zeros((N, 4), dtype=torch.float64, device=dev)
            self._virial = torch.zeros((6, N), dtype=torch.float64, device=dev)

    def compute(self, timestep=None):
        self._require()
        raise NotImplementedError

    # -- HOOMD Force properties ---------------------------------------------
    @property
    def forces(self):
        self._require()
        return self._force[:, :3].cpu().numpy()

    @property
    def energies(self):
        self._require()
        return self._force[:, 3].cpu().numpy()

    @property
    def energy(self):
        self._require()
        return float(self._force[:, 3].sum().item())

    @property
    def torques(self):
        self._require()
        return self._torque[:, :3].cpu().numpy()

    @property
    def virials(self):
        self._require()
        if not self.compute_virial:
            return None
        return self._virial.t().cpu().numpy()

    # device views, for integrators and benchmarks
    @property
    def force_tensor(self):
        return self._force

    @property
    def torque_tensor(self):
        return self._torque
