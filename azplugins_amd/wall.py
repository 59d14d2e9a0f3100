"""Wall potentials: the LJ 9-3 and colloid walls of the reference's legacy wall evaluators
(``src/WallEvaluatorLJ93.h``, ``src/WallEvaluatorColloid.h``, instantiated in ``src/WallPotentials.h``) on planes,
spheres and cylinders, on libazp's wall kernels (``csrc/wall_forces.hip``).

The reference's two headers define only ``V(r)``. The loop over the walls, the geometries and the extrapolated mode
belong to HOOMD's wall code, whose source this project does not have: everything but ``V(r)`` is DEFINED HERE
(and in ``include/azp.h``), not taken from HOOMD.

Every geometry yields a signed distance ``d`` to its surface and a unit vector ``u``, the direction in which ``d``
grows (given by the formula, whichever side the particle is on). The active side is ``d > 0``. ``x`` is the particle
position wrapped into the box as the barrier kernels wrap it; walls are not periodic (no minimum image).

With ``c = r_cut`` and ``e = r_extrap`` of the particle's type, one wall contributes

* standard mode (``e == 0``): ``E = V(d) - shift``, ``F = -V'(d) u`` if ``0 < d < c`` (strict at ``c``), else nothing
  (also for ``d <= 0``);
* extrapolated mode (``0 < e < c``): as above for ``d >= e``; for ``d < e``, behind the wall included,
  ``E = V(e) - shift + F_e (e - d)`` and ``F = F_e u`` with ``F_e = -V'(e)``: energy and force are continuous at ``e``.

``shift`` is ``V(r_cut)`` in mode ``"shift"`` and 0 in mode ``"none"``. The walls' contributions are added in list
order; the outputs are overwritten for all N particles.

The per-particle virial is ZERO: the reference's headers do not define one and ``HarmonicBarrier`` sets the precedent.
The virial buffer is written with zeros whenever ``compute_virial`` is set (``ThermodynamicQuantities`` turns it on),
so the pressure of a system with walls lacks the wall term.

Out of scope: moving walls, a wall virial, HOOMD's ``open`` flag, per-particle diameters, an ``_azplugins`` class."""

import ctypes as C
import math

import numpy as np

from . import _lib
from .force import Force, TypeParameter


def _vec3(name, v):
    try:
        out = tuple(float(c) for c in v)
    except TypeError:
        raise ValueError("%s must be three numbers, got %r" % (name, v))
    if len(out) != 3 or not all(math.isfinite(c) for c in out):
        raise ValueError("%s must be three finite numbers, got %r" % (name, v))
    return out


def _unit(name, v):
    v = _vec3(name, v)
    n = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    if n == 0.0:
        raise ValueError("%s must not be the zero vector" % name)
    return (v[0] / n, v[1] / n, v[2] / n)


def _radius(r):
    r = float(r)
    if not (math.isfinite(r) and r > 0.0):
        raise ValueError("radius must be positive and finite, got %r" % (r,))
    return r


class _Geometry:
    """Plain parameter holder: equal when the parameters are equal, picklable."""

    _fields = ()

    def __eq__(self, other):
        return type(other) is type(self) and all(getattr(self, f) == getattr(other, f) for f in self._fields)

    def __hash__(self):
        return hash((type(self).__name__,) + tuple(getattr(self, f) for f in self._fields))

    def __repr__(self):
        return "%s(%s)" % (type(self).__name__, ", ".join("%s=%r" % (f, getattr(self, f)) for f in self._fields))


class Plane(_Geometry):
    """``d = n.(x - origin)``, ``u = n``; ``normal`` is normalised here (a zero normal raises ``ValueError``)."""

    _fields = ("origin", "normal")

    def __init__(self, origin=(0.0, 0.0, 0.0), normal=(0.0, 0.0, 1.0)):
        self.origin = _vec3("origin", origin)
        self.normal = _unit("normal", normal)

    def _c(self):
        return _lib.Wall(_lib.WALL_PLANE, 0, self.origin, self.normal, 0.0)


class Sphere(_Geometry):
    """``rho = |x - origin|``. Inside: ``d = R - rho``, ``u = -(x - origin) / rho``; outside: ``d = rho - R``,
    ``u = (x - origin) / rho``. At ``rho == 0`` ``u = 0``: the energy counts, the force does not."""

    _fields = ("radius", "origin", "inside")

    def __init__(self, radius, origin=(0.0, 0.0, 0.0), inside=True):
        self.radius = _radius(radius)
        self.origin = _vec3("origin", origin)
        self.inside = bool(inside)

    def _c(self):
        return _lib.Wall(_lib.WALL_SPHERE, int(self.inside), self.origin, (0.0, 0.0, 1.0), self.radius)


class Cylinder(_Geometry):
    """``s = (x - origin) - ((x - origin).a) a``, ``rho = |s|``, then as the sphere with ``s`` in place of
    ``x - origin``; ``axis`` is normalised here."""

    _fields = ("radius", "origin", "axis", "inside")

    def __init__(self, radius, origin=(0.0, 0.0, 0.0), axis=(0.0, 0.0, 1.0), inside=True):
        self.radius = _radius(radius)
        self.origin = _vec3("origin", origin)
        self.axis = _unit("axis", axis)
        self.inside = bool(inside)

    def _c(self):
        return _lib.Wall(_lib.WALL_CYLINDER, int(self.inside), self.origin, self.axis, self.radius)


class _WallParameter(TypeParameter):
    """``TypeParameter`` whose values are also checked by the potential (ranges, not only keys and types)."""

    def __init__(self, name, schema, check, on_change):
        super().__init__(name, schema, 1, on_change)
        self._check = check

    def _validate(self, value):
        out = super()._validate(value)
        self._check(out)
        return out


class _WallPotential(Force):
    """Common part of the two wall potentials: the wall list, the mode, the per-type rows and the two launches."""

    _schema = None
    _entry = None
    _net_entry = None
    _make = None
    _cpp_class_name = None  # the reference's module.cc registers no wall class

    def __init__(self, walls, mode="shift"):
        super().__init__()
        walls = list(walls)
        if not 1 <= len(walls) <= _lib.WALL_MAX:
            raise ValueError("%s takes 1 to %d walls, got %d" % (type(self).__name__, _lib.WALL_MAX, len(walls)))
        for w in walls:
            if not isinstance(w, _Geometry):
                raise TypeError("walls must be Plane, Sphere or Cylinder objects, got %r" % (w,))
        self._walls = tuple(walls)
        self._mode = None
        self.mode = mode
        self.params = _WallParameter("params", self._schema, self._check_params, self._mark_dirty)
        self._tables = None
        self._net = None  # (out, scratch) of wall_forces

    @property
    def walls(self):
        return self._walls

    @property
    def mode(self):
        return self._mode

    @mode.setter
    def mode(self, value):
        if value not in ("none", "shift"):
            raise ValueError("%s: mode must be 'none' or 'shift', got %r" % (type(self).__name__, value))
        self._mode = value
        self._tables = None

    def _mark_dirty(self):
        self._tables = None

    def _attach(self, sim):
        super()._attach(sim)
        self._tables = None

    @staticmethod
    def _check_cut(d):
        if not (d["r_cut"] >= 0.0 and d["r_extrap"] >= 0.0):
            raise ValueError("params: r_cut and r_extrap must not be negative")
        if d["r_cut"] > 0.0 and d["r_extrap"] >= d["r_cut"]:
            raise ValueError("params: r_extrap (%g) must be smaller than r_cut (%g)" % (d["r_extrap"], d["r_cut"]))

    def _check_params(self, d):
        self._check_cut(d)

    def _row_args(self, d):
        raise NotImplementedError

    def _row(self, d):
        """One type's dict folded into its parameter row by libazp (coefficients, r_cut, r_extrap, shift, V(e), F_e)."""
        row = (C.c_double * _lib.WALL_PARAM_DOUBLES)()
        shift = 1 if self._mode == "shift" else 0
        _lib.check(getattr(_lib.lib(), self._make)(*(self._row_args(d) + [d["r_cut"], d["r_extrap"], shift, row])), self._make)
        return list(row)

    def _args(self):
        import torch

        st = self._state
        if self._tables is None:
            raw = np.zeros((len(st.types), _lib.WALL_PARAM_DOUBLES))
            for i, t in enumerate(st.types):
                d = self.params.get_raw(t)
                if d is None:
                    raise _lib.AzpError("%s.params[%r] is not set" % (type(self).__name__, t))
                raw[i] = self._row(d)
            self._tables = torch.from_numpy(raw).to(st.device)
        a = _lib.WallArgs()
        a.N = st.N
        a.ntypes = len(st.types)
        a.d_pos = st.pos.data_ptr()
        a.box = st.box.to_c()
        a.d_params = self._tables.data_ptr()
        a.n_walls = len(self._walls)
        for k, w in enumerate(self._walls):
            a.walls[k] = w._c()
        return a

    def compute(self, timestep=None):
        self._require()
        st = self._state
        self._ensure_buffers()
        a = self._args()
        a.d_force = self._force.data_ptr()
        # (zeros, written every call that a virial is asked for: the thermodynamic sums read this buffer)
        a.d_virial = self._virial.data_ptr() if self.compute_virial else None
        a.virial_pitch = st.N
        _lib.check(getattr(_lib.lib(), self._entry)(C.byref(a), _lib.raw_stream(st.device)), self._entry)

    @property
    def wall_forces(self):
        """``(n_walls, 3)``: row ``w`` is the force the particles exert on wall ``w``, ``-sum_i F_i^(w)``, at the
        current state (the observable behind a substrate pressure). Summed on the device in a fixed order: two reads
        of one state agree bit for bit. On a decomposed run the ranks' sums are added over the domain's group."""
        import torch

        from .compute import _all_reduce_sum

        self._require()
        st = self._state
        a = self._args()
        lib = _lib.lib()
        need = C.c_uint64(0)
        _lib.check(lib.azp_wall_net_forces_scratch_size(C.byref(a), C.byref(need)), "azp_wall_net_forces_scratch_size")
        if self._net is None or self._net[1].numel() < need.value or self._net[0].device != st.pos.device:
            self._net = (torch.empty((len(self._walls), 4), dtype=torch.float64, device=st.device),
                         torch.empty(max(int(need.value), 8), dtype=torch.uint8, device=st.device))
        out, scratch = self._net
        _lib.check(getattr(lib, self._net_entry)(C.byref(a), out.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                                 _lib.raw_stream(st.device)), self._net_entry)
        dom = self._sim.domain
        if dom is not None:
            out = _all_reduce_sum(dom, out.clone())
        return out[:, :3].cpu().numpy()


class LJ93(_WallPotential):
    """Lennard-Jones 9-3 wall (reference ``src/WallEvaluatorLJ93.h``): ``V(r) = epsilon [(2/15) (sigma/r)^9 -
    (sigma/r)^3]``. ``params[type] = dict(epsilon, sigma, r_cut, r_extrap=0.0)``; a type with ``epsilon == 0`` or
    ``r_cut == 0`` feels nothing. ``walls``: 1 to 16 geometries; ``mode``: ``"none"`` or ``"shift"``. Semantics of
    the cutoff, the extrapolated mode and the (zero) virial: see the module docstring."""

    _schema = dict(epsilon=float, sigma=float, r_cut=float, r_extrap=0.0)
    _entry = "azp_wall_forces_lj93"
    _net_entry = "azp_wall_net_forces_lj93"
    _make = "azp_wall_lj93_params_make"

    def _row_args(self, d):
        return [d["epsilon"], d["sigma"]]


class Colloid(_WallPotential):
    """Colloid (integrated Lennard-Jones) wall (reference ``src/WallEvaluatorColloid.h``): ``V(z) = C1 [(7a - z) /
    (z - a)^7 + (7a + z) / (z + a)^7] - C2 [2az / (z^2 - a^2) + ln((z - a) / (z + a))]``, ``C1 = A sigma^6 / 7560``,
    ``C2 = A / 6``. ``params[type] = dict(A, sigma, a, r_cut, r_extrap=0.0)``: the radius ``a`` is a per-type
    parameter (``State`` carries no diameters), as ``pair.Colloid`` takes ``a_1`` and ``a_2``. A type with
    ``A == 0``, ``a <= 0`` or ``r_cut == 0`` feels nothing; otherwise ``r_cut > a`` and, if set, ``r_extrap > a``.

    In standard mode a particle with ``0 < d <= a`` (its surface touching or inside the wall) gets a NON-FINITE
    energy and force, as in the reference. Set ``r_extrap`` (a little above ``a``) to keep such particles finite."""

    _schema = dict(A=float, sigma=float, a=float, r_cut=float, r_extrap=0.0)
    _entry = "azp_wall_forces_colloid"
    _net_entry = "azp_wall_net_forces_colloid"
    _make = "azp_wall_colloid_params_make"

    def _check_params(self, d):
        self._check_cut(d)
        if d["A"] == 0.0 or not d["a"] > 0.0 or d["r_cut"] == 0.0:
            return
        if d["r_cut"] <= d["a"]:
            raise ValueError("params: r_cut (%g) must be larger than the radius a (%g)" % (d["r_cut"], d["a"]))
        if 0.0 < d["r_extrap"] <= d["a"]:
            raise ValueError("params: r_extrap (%g) must be larger than the radius a (%g)" % (d["r_extrap"], d["a"]))

    def _row_args(self, d):
        return [d["A"], d["sigma"], d["a"]]


__all__ = ["Plane", "Sphere", "Cylinder", "LJ93", "Colloid"]
