"""Pair potentials: drop-in mirror of ``hoomd.azplugins.pair`` (reference
``src/pair.py``) driving libazp's gfx950 kernels through the C ABI.

Class names, constructor arguments, parameter keys, accepted ``mode`` values and
the parameter round trip follow the reference (file:line in each class). What
the reference delegates to HOOMD's ``hoomd.md.pair.Pair`` -- ``r_cut`` / ``r_on``
type parameters, ``mode``, attaching -- is restated here in reduced form.
"""

import ctypes as C

import numpy as np

from . import _lib
from .force import Force, ScalarTypeParameter, TableTypeParameter, TypeParameter

_SHIFT = {"none": 0, "shift": 1, "xplor": 2}


class Pair(Force):
    """Reduced ``hoomd.md.pair.Pair``: neighbor list, per-type-pair ``params``,
    ``r_cut``, ``r_on`` and ``mode``."""

    _cpp_class_name = None          # name the reference registers in _azplugins
    _entry = None                   # libazp entry point
    _planned_entry = None           # tile-plan entry point (isotropic pairs)
    _plan_balance = False           # plans from cells: rows to lanes by in-range length (expensive, ragged pair blocks)
    _schema = {}
    _param_doubles = 4              # size of the raw param struct in doubles
    _accepted_modes = ("none", "shift", "xplor")
    _halo_fields = ("pos",)         # per-particle arrays whose ghost rows the kernel reads (decomposed runs)

    def __init__(self, nlist, default_r_cut=None, default_r_on=0.0, mode="none"):
        super().__init__()
        if mode not in self._accepted_modes:
            raise ValueError("mode must be one of %s, got %r" % (self._accepted_modes, mode))
        self.nlist = nlist
        self._mode = mode
        self.params = TypeParameter("params", self._schema, 2, self._mark_dirty, self._readback)
        self.r_cut = ScalarTypeParameter("r_cut", default_r_cut, self._r_cut_changed)
        self.r_on = ScalarTypeParameter("r_on", default_r_on, self._mark_dirty)
        self.threads_per_particle = 0   # 0 = library heuristic (HOOMD autotunes this)
        self.block_size = 0
        self.use_plan = True            # LDS-staged tile kernel when the neighbor list can be tiled
        self.use_displacement_bound = True  # let it stop rows early while particles have barely moved (exact)
        # ... by the displacements of each tile's own particles instead of the global maximum: pays when a few
        # particles move much farther than the rest; on a liquid in equilibrium it costs 1 %, so opt-in
        self.use_local_displacement = False
        self.plan_bank_order = None     # None: bank-aware rows only for long-lived lists (below); True / False: always / never
        self.use_fused_plan = True      # sole consumer of its list: compile the plan straight from the binned particles
        self.use_speculative_launch = True  # queue the force kernel behind the list's distance check (_compute_speculative)
        self._plan = None               # _lib.PairPlan (created by the first compile)
        self._plan_builds = None        # _plan_key() the plan was compiled for (None: recompile at the next launch)
        self._plan_valid = False
        self._plan_ids = None           # (list_id, head_id) of a plan compiled from the cells: the plan is its own list
        self._plan_disp0 = None         # displacement bound of the list's positions when the plan was compiled
        self._calls_since_plan = None   # force calls the plan on hand has served (None: no plan compiled yet)
        self._spec_cache = None         # (signature, box struct, pair args) of the last speculative launch
        self._fused_refused_types = None  # type count whose table the tile kernel could not hold (no fused plan)
        self._tables = None
        self._cpp = None            # the _azplugins C++ object (created on attach)
        self._cpp_synced = False
        nlist.add_consumer(self)

    # -- mode ----------------------------------------------------------------
    @property
    def mode(self):
        return self._mode

    @mode.setter
    def mode(self, m):
        if m not in self._accepted_modes:
            raise ValueError("mode must be one of %s, got %r" % (self._accepted_modes, m))
        self._mode = m
        self._mark_dirty()

    def _mark_dirty(self):
        self._tables = None
        self._cpp_synced = False
        # the tile plan orders and classifies rows against the cutoffs / inner radii it was
        # built with: recompile it with the new tables
        self._plan_builds = None

    def _r_cut_changed(self):
        """HOOMD rebuilds the neighbor list when a consumer's r_cut matrix changes: the
        list on hand was built for the old r_cut + buffer."""
        self._mark_dirty()
        self.nlist.consumers_changed()

    # -- raw parameter structs (host side of the C ABI) ------------------------
    def _pack(self, d):
        raise NotImplementedError

    def _unpack(self, raw):
        raise NotImplementedError

    def _readback(self, key):
        """After attaching, ``params[...]`` returns what the C++ side holds
        (HOOMD: getParams -> asDict), as the reference tests check
        (src/pytest/test_pair.py:349)."""
        if not self._attached or key not in self.params._data:
            return None
        self._sync_cpp()
        return dict(self._cpp.getParams(*key))

    def _make_cpp(self):
        """The ``_azplugins`` class of this potential for a GPU device: ``_cpp_class_name +
        "GPU"`` (hoomd's _attach_hook; the conservative DPD potential only has a CPU class)."""
        ext = _lib.ext_module()
        cls = getattr(ext, self._cpp_class_name + "GPU", None) or getattr(ext, self._cpp_class_name)
        return cls(list(self._state.types))

    def _sync_cpp(self):
        """Push the Python-side type parameters into the C++ object (setParams / setRCut /
        setROn / mode), as HOOMD's TypeParameter machinery does on attach and on every change."""
        if self._cpp is None:
            self._cpp = self._make_cpp()
            self._cpp_synced = False
        if self._cpp_synced:
            return
        types = self._state.types
        for i, a in enumerate(types):
            for b in types[i:]:
                d = self.params.get_raw((a, b))
                if d is not None:
                    self._cpp.setParams(a, b, d)
                self._cpp.setRCut(a, b, self.r_cut[(a, b)])
                self._cpp.setROn(a, b, self.r_on[(a, b)])
        self._cpp.mode = self._mode
        self._cpp_synced = True

    def _r_cut_matrix(self):
        self._require()
        types = self._state.types
        T = len(types)
        rc = np.zeros((T, T))
        for i, a in enumerate(types):
            for j, b in enumerate(types):
                rc[i, j] = self.r_cut[(a, b)]
        return rc

    def _attach(self, sim):
        super()._attach(sim)
        self._tables = None
        self._cpp = None
        self._cpp_synced = False

    def _build_tables(self):
        """Device tables from the C++ object's host tables (param_type structs, r_cut^2, r_on^2)."""
        import torch

        types = self._state.types
        T = len(types)
        for a in types:
            for b in types:
                if self.params.get_raw((a, b)) is None:
                    raise _lib.AzpError("%s.params[(%r, %r)] is not set" % (type(self).__name__, a, b))
        self._sync_cpp()
        raw = np.frombuffer(self._cpp.params_bytes(), dtype=np.float64).reshape(T * T, -1).copy()
        assert raw.shape[1] == self._param_doubles
        rc = np.asarray(self._cpp.rcutsq())
        ro = np.asarray(self._cpp.ronsq())
        dev = self._state.device
        self._spec_cache = None  # (argument structs kept by _compute_speculative point into the old tables)
        self._tables = dict(
            params=torch.from_numpy(raw).to(dev), rcutsq=torch.from_numpy(rc).to(dev), ronsq=torch.from_numpy(ro).to(dev)
        )
        # optional row-ordering hint for the tile plan (azp_pair_args.d_rinnersq)
        inner = np.zeros(T * T)
        for i, a in enumerate(types):
            for j, b in enumerate(types):
                inner[i * T + j] = self._inner_radius(self.params.get_raw((a, b))) ** 2
        if inner.any():
            self._tables["rinnersq"] = torch.from_numpy(inner).to(dev)

    def _inner_radius(self, d):
        """Radius inside which the potential takes a (rare) short-range branch; the
        tile plan lists such pairs first. 0 = no such branch."""
        return 0.0

    def takes_plan_from_cells(self):
        """The neighbor list's question at a build, when this potential is its sole consumer: may the list skip its
        HOOMD-format rows (fused mode)? Yes when the tile plan is compiled straight from the cells."""
        st = self._state
        refused = st is not None and self._fused_refused_types == len(st.types)  # (the types' table did not fit)
        return bool(self.use_plan and self._planned_entry and self.threads_per_particle in (0, 1) and self.use_fused_plan
                    and not refused)

    def _pair_args(self, particle_range=None):
        """azp_pair_args for the current state and ``particle_range`` (first, count): the list's HOOMD-format rows, or
        while the list is in fused mode the ids of the plan compiled from its cells (placeholders until that compile)."""
        st, nl = self._state, self.nlist
        a = _lib.PairArgs()
        a.d_force = self._force.data_ptr()
        a.d_virial = self._virial.data_ptr()
        a.virial_pitch = st.N
        a.N = st.N
        a.n_max = st.n_max
        a.d_pos = st.pos.data_ptr()
        a.box = st.box.to_c()
        a.d_n_neigh = nl.n_neigh.data_ptr()
        if nl.fused_active:
            ids = self._plan_ids if self._plan_builds == self._plan_key() else None
            a.d_nlist, a.d_head_list = ids if ids else (nl.n_neigh.data_ptr(), nl.n_neigh.data_ptr())
        else:
            a.d_nlist, a.d_head_list, a.size_nlist = nl.nlist.data_ptr(), nl.head_list.data_ptr(), nl.size
        a.d_rcutsq = self._tables["rcutsq"].data_ptr()
        a.d_ronsq = self._tables["ronsq"].data_ptr()
        if "rinnersq" in self._tables:
            a.d_rinnersq = self._tables["rinnersq"].data_ptr()
        a.ntypes = len(st.types)
        a.shift_mode = _SHIFT[self._mode]
        a.compute_virial = 1 if self.compute_virial else 0
        a.block_size = self.block_size
        a.threads_per_particle = self.threads_per_particle
        if not self.use_plan:
            a.flags = _lib.PAIR_FLAG_NO_AUTO_PLAN  # use_plan = False means the generic kernel, not libazp's own plan cache
        a.r_list_max = nl.r_list_max
        # displacement of any particle since the PLAN was built <= displacement since the list was
        # built (now) + the same quantity at the time the plan was built (0 in the usual flow)
        bound = nl.displacement_bound(st)
        d0 = self._plan_disp0
        if bound is not None and d0 is not None and self.use_displacement_bound:
            a.has_displacement_bound, a.displacement_bound = 1, bound + d0
            darr = nl.displacements(st) if self.use_local_displacement else None
            if darr is not None and darr.shape[0] == st.n_max:
                a.d_displacement, a.displacement_bound_extra = darr.data_ptr(), d0
        if particle_range is not None:
            a.range_first, a.range_count = int(particle_range[0]), int(particle_range[1])
        return a

    def compute(self, timestep=None, particle_range=None):
        """Evaluate the forces. ``particle_range=(first, count)`` restricts the
        launch to a sub-range of the local particles (domain-decomposed runs compute
        the interior while the halo exchange is in flight)."""
        self._require()
        st = self._state
        if particle_range is None and self._compute_speculative(timestep):
            return
        self.nlist.compute(st)
        self._ensure_buffers()  # after the list: a rebuild of a decomposed run migrates particles
        if self._tables is None:
            self._build_tables()
        entry, args = self._prepare_launch(_lib.raw_stream(st.device), timestep, particle_range)
        rc = getattr(_lib.lib(), entry)(*args)
        if rc == _lib.ERROR_TOO_MANY_TYPES and self._plan_ids is not None:
            # the tile kernel cannot hold the per-type-pair table beside its staged slots, and a plan compiled from the
            # cells has no list for the generic kernel: cannot run fused. The list leaves fused mode as after a failed
            # compile; the planned entry runs the generic kernel on the plan compiled from the list.
            self._fused_refused_types = len(st.types)
            self.nlist.leave_fused_mode()
            entry, args = self._prepare_launch(_lib.raw_stream(st.device), timestep, particle_range)
            rc = getattr(_lib.lib(), entry)(*args)
        _lib.check(rc, entry)

    def _compute_speculative(self, timestep):
        """The common MD step -- the list was built earlier, the particles have moved, the plan is current: queue the
        neighbor list's distance check AND the force kernel behind it before asking for the check's result. The
        kernel reads the displacement bound from the check's device words and leaves at once if the check asks for
        a rebuild (azp_pair_args.d_stale_flag); the host then waits for the check alone while the GPU is already
        computing forces, instead of idling it for a readback and a launch every step. Returns False when the
        ordinary path has to run (first call, rebuild, no plan, decomposed run)."""
        nl, st = self.nlist, self._state
        if not (self.use_speculative_launch and self.use_plan and self._planned_entry is not None and self.use_displacement_bound
                and self._plan_valid and self._tables is not None and self._plan_disp0 is not None
                and self._plan_builds == self._plan_key() and self._force.shape[0] == st.N and nl.allows_speculative_launch(st)):
            return False
        token = nl.begin_check(st)
        # the argument struct of the previous step, while nothing it points to has moved (the host side of a step has to
        # stay shorter than NVE + distance check on the GPU, ~50 us at N = 2^20, or the force kernel waits for its launch)
        boxc = st.box.to_c()
        sig = (self._plan_builds, self._force.data_ptr(), self._virial.data_ptr(), st.pos.data_ptr(), nl.n_neigh.data_ptr(), id(self._tables),
               self._mode, self.compute_virial, self._plan_disp0, st.N, st.n_max, self.block_size)
        cache = self._spec_cache
        if cache is not None and cache[0] == sig and cache[1] is boxc:
            a = cache[2]
        else:
            self._list_mode_for_launch(True)
            a = self._pair_args()
            a.has_displacement_bound, a.displacement_bound, a.d_displacement = 0, 0.0, None
            a.displacement_bound_extra = self._plan_disp0
            self._spec_cache = (sig, boxc, a)
        a.d_stale_flag, a.d_displacement_sq_bits = token["flag_ptr"], token["bits_ptr"]
        entry, args = self._prepare_launch(_lib.raw_stream(st.device), timestep, a=a)
        _lib.check(getattr(_lib.lib(), entry)(*args), entry)
        if nl.end_check(token):
            return False  # rebuild: the kernel left without writing; the ordinary path takes over (it has the verdict)
        return True

    def _prepare_launch(self, stream, timestep, particle_range=None, a=None):
        """The launch for the current state: the libazp entry point and its arguments -- the tile plan's handle for the
        planned entry points, this potential's argument struct, the parameter table, ``stream``. Without ``a`` the pair
        args are filled for ``particle_range`` and the plan step runs; ``a``: pair args for the plan on hand, which the
        caller has found current (the speculative path)."""
        planned = self.use_plan and self._planned_entry is not None
        if a is None:
            self._list_mode_for_launch(planned)
            a = self._pair_args(particle_range)
            if planned:
                self._plan_step(a, stream)
        args, params = C.byref(self._wrap_args(a, timestep)), self._tables["params"].data_ptr()
        if not planned:
            return self._entry, (args, params, stream)
        self._calls_since_plan += 1
        return self._planned_entry, (self._plan.handle, args, params, stream)

    def _list_mode_for_launch(self, planned):
        """Before a launch's pair args: a launch that does not take its plan from the cells needs the HOOMD-format list,
        and a plan that was compiled from the cells (its own list) is recompiled once the list has left fused mode."""
        nl = self.nlist
        if nl.fused_active and not (planned and self.use_fused_plan):
            nl.leave_fused_mode()
        if self._plan_ids is not None and not nl.fused_active:
            self._plan_ids = self._plan_builds = None

    def _plan_step(self, a, stream):
        """Compile the tile plan when the neighbor list was rebuilt since the last compile -- from the list's cells in
        fused mode, else (or when that compile fails) from its HOOMD-format rows -- and fill in the list ids and the
        displacement fields of ``a`` for this launch."""
        key = self._plan_key()
        if self._plan_builds == key:
            return
        if self._plan is None:
            self._plan = _lib.PairPlan()
        nl = self.nlist
        first, count = a.range_first, a.range_count
        a.range_first = a.range_count = 0  # (a plan covers all local particles)
        if nl.fused_active:
            # the plan straight from the binned particles: no u32 list, no hash set, one kernel
            self._plan.set_balance(self._plan_balance)
            info = nl.compile_plan(self._plan, a, stream)
            self._plan_valid = bool(info["valid"])
            if info["valid"]:
                self._plan_ids = (info["list_id"], info["head_id"])
                a.d_nlist, a.d_head_list = self._plan_ids
                self._plan_builds = key
                self._calls_since_plan = 0
                # row classes were cut at the positions the LIST was built from, whenever this compile runs
                self._plan_disp0 = 0.0
                b = nl.displacement_bound(self._state)
                known = b is not None and self.use_displacement_bound
                a.has_displacement_bound, a.displacement_bound = (1, b) if known else (0, 0.0)
                a.displacement_bound_extra = 0.0
            else:
                a.d_nlist, a.d_head_list, a.size_nlist = nl.nlist.data_ptr(), nl.head_list.data_ptr(), nl.size
        if self._plan_builds != key:
            # bank-aware rows pay off only for lists that live long (include/azp.h): keep them
            # for the first build and whenever the previous list served >= 50 force calls
            calls = self._calls_since_plan
            self._plan.set_bank_order((calls is None or calls >= 50) if self.plan_bank_order is None else self.plan_bank_order)
            self._calls_since_plan = 0
            self._plan.build(a, stream)
            self._plan_valid = bool(self._plan.info()["valid"])
            self._plan_builds = key
            self._plan_disp0 = nl.displacement_bound(self._state)
            # this launch sees exactly the positions the plan was built from
            a.has_displacement_bound, a.displacement_bound = (1 if self.use_displacement_bound else 0), 0.0
            a.d_displacement = None  # (those refer to the positions the LIST was built from)
        a.range_first, a.range_count = first, count

    def _plan_key(self):
        return (id(self.nlist), self.nlist.num_builds, self.threads_per_particle)

    def _wrap_args(self, a, timestep):
        """The argument struct of this potential's entry points around the common pair args."""
        return a

    @property
    def plan_info(self):
        return self._plan.info() if self._plan is not None else None


class Colloid(Pair):
    """Colloid pair potential (reference ``src/pair.py:14-118``)."""

    _cpp_class_name = "PotentialPairColloid"
    _entry = "azp_pair_forces_colloid"
    _planned_entry = "azp_pair_forces_planned_colloid"
    _schema = dict(A=float, a_1=float, a_2=float, sigma=float)

    def _pack(self, d):
        out = np.zeros(4)
        _lib.lib().azp_colloid_params_make(d["A"], d["a_1"], d["a_2"], d["sigma"], out.ctypes.data)
        return out

    def _unpack(self, raw):
        v = [C.c_double() for _ in range(4)]
        _lib.lib().azp_colloid_params_unpack(raw.ctypes.data, *[C.byref(x) for x in v])
        return dict(A=v[0].value, a_1=v[1].value, a_2=v[2].value, sigma=v[3].value)


class ExpandedYukawa(Pair):
    """Expanded Yukawa pair potential (reference ``src/pair.py:242-297``)."""

    _cpp_class_name = "PotentialPairExpandedYukawa"
    _entry = "azp_pair_forces_expanded_yukawa"
    _planned_entry = "azp_pair_forces_planned_expanded_yukawa"
    _schema = dict(epsilon=float, kappa=float, delta=float)

    def _pack(self, d):
        return np.array([d["epsilon"], d["kappa"], d["delta"], 0.0])

    def _unpack(self, raw):
        return dict(epsilon=float(raw[0]), kappa=float(raw[1]), delta=float(raw[2]))


class Hertz(Pair):
    """Hertz pair potential (reference ``src/pair.py:300-351``)."""

    _cpp_class_name = "PotentialPairHertz"
    _entry = "azp_pair_forces_hertz"
    _planned_entry = "azp_pair_forces_planned_hertz"
    _schema = dict(epsilon=float)
    _param_doubles = 1

    def _pack(self, d):
        return np.array([d["epsilon"]])

    def _unpack(self, raw):
        return dict(epsilon=float(raw[0]))


class PerturbedLennardJones(Pair):
    """Perturbed Lennard-Jones pair potential (reference ``src/pair.py:354-426``)."""

    _cpp_class_name = "PotentialPairPerturbedLennardJones"
    _entry = "azp_pair_forces_perturbed_lennard_jones"
    _planned_entry = "azp_pair_forces_planned_perturbed_lennard_jones"
    _schema = dict(epsilon=float, sigma=float, attraction_scale_factor=float)

    def _pack(self, d):
        out = np.zeros(4)
        _lib.lib().azp_plj_params_make(d["epsilon"], d["sigma"], d["attraction_scale_factor"], out.ctypes.data)
        return out

    def _unpack(self, raw):
        v = [C.c_double() for _ in range(3)]
        _lib.lib().azp_plj_params_unpack(raw.ctypes.data, *[C.byref(x) for x in v])
        return dict(epsilon=v[0].value, sigma=v[1].value, attraction_scale_factor=v[2].value)

    def _inner_radius(self, d):
        # the WCA core (r < 2^(1/6) sigma), plus the distance a pair can close before
        # the next neighbor-list rebuild
        # (+ 1e-3: the tile kernel drops its core test beyond the first chunks of a row only while
        # r_wca + 2 x displacement bound clears this radius by the plan's single-precision margin)
        return 2.0 ** (1.0 / 6.0) * d["sigma"] + self.nlist.buffer + 1e-3


class DPDGeneralWeight(Pair):
    """DPD thermostat with generalized weight function (reference
    ``src/pair.py:121-239``). ``kT`` may be a float or a callable of the
    timestep (HOOMD ``Variant``). ``mode`` is always ``"none"``."""

    _cpp_class_name = "PotentialPairDPDThermoGeneralWeight"
    _halo_fields = ("pos", "vel")   # (ghost tags change only when the ghosts are re-selected)
    _entry = "azp_dpd_forces_general_weight"
    _planned_entry = "azp_dpd_forces_planned_general_weight"
    _plan_balance = True
    _schema = dict(A=float, gamma=float, s=float)
    _accepted_modes = ("none",)

    def __init__(self, nlist, kT, default_r_cut=None):
        super().__init__(nlist, default_r_cut=default_r_cut, default_r_on=0.0, mode="none")
        self.kT = kT

    def _pack(self, d):
        return np.array([d["A"], d["gamma"], d["s"], 0.0])

    def _unpack(self, raw):
        return dict(A=float(raw[0]), gamma=float(raw[1]), s=float(raw[2]))

    def _attach(self, sim):
        # DPD uses RNGs: warn if the seed was not set (src/pair.py:236-239)
        sim._warn_if_seed_unset()
        super()._attach(sim)

    def _wrap_args(self, a, timestep):
        st = self._state
        d = _lib.DPDArgs()
        d.pair = a
        d.d_vel = st.vel.data_ptr()
        d.d_tag = st.tag.data_ptr()
        ts = self._sim.timestep if timestep is None else timestep
        d.timestep = int(ts)
        d.deltaT = float(self._sim.dt)
        d.T = float(self.kT(ts)) if callable(self.kT) else float(self.kT)
        d.seed = int(self._sim.seed) & 0xFFFF
        return d


class DPDConservativeGeneralWeight(Pair):
    """Conservative part only: the reference also registers
    ``PotentialPairConservativeGeneralWeight``
    (src/export_PotentialPairDPDThermo.cc.inc:33-35)."""

    _cpp_class_name = "PotentialPairConservativeGeneralWeight"
    _entry = "azp_pair_forces_dpd_conservative"
    _planned_entry = "azp_pair_forces_planned_dpd_conservative"
    _schema = dict(A=float, gamma=float, s=float)
    _accepted_modes = ("none",)

    def __init__(self, nlist, default_r_cut=None):
        super().__init__(nlist, default_r_cut=default_r_cut, default_r_on=0.0, mode="none")

    _pack = DPDGeneralWeight._pack
    _unpack = DPDGeneralWeight._unpack


class TwoPatchMorse(Pair):
    """Two-patch Morse anisotropic pair potential (reference
    ``src/pair.py:429-525``; HOOMD ``AnisotropicPair``: no ``r_on``, modes
    ``"none"`` / ``"shift"``)."""

    _cpp_class_name = "AnisoPotentialPairTwoPatchMorse"
    _halo_fields = ("pos", "orientation")
    _entry = "azp_aniso_forces_two_patch_morse"
    _planned_entry = "azp_aniso_forces_planned_two_patch_morse"
    _plan_balance = True
    _schema = dict(M_d=float, M_r=float, r_eq=float, omega=float, alpha=float, repulsion=bool)
    _param_doubles = 6
    _accepted_modes = ("none", "shift")

    def __init__(self, nlist, default_r_cut=None, mode="none"):
        super().__init__(nlist, default_r_cut=default_r_cut, default_r_on=0.0, mode=mode)

    def _pack(self, d):
        out = np.zeros(6)
        _lib.lib().azp_tpm_params_make(d["M_d"], d["M_r"], d["r_eq"], d["omega"], d["alpha"], int(d["repulsion"]),
                                       out.ctypes.data)
        return out

    def _unpack(self, raw):
        v = [C.c_double() for _ in range(5)]
        rep = C.c_int()
        _lib.lib().azp_tpm_params_unpack(raw.ctypes.data, *[C.byref(x) for x in v], C.byref(rep))
        return dict(M_d=v[0].value, M_r=v[1].value, r_eq=v[2].value, omega=v[3].value, alpha=v[4].value,
                    repulsion=bool(rep.value))

    def _wrap_args(self, a, timestep):
        st = self._state
        g = _lib.AnisoArgs()
        g.pair = a
        g.d_orientation = st.orientation.data_ptr()
        g.d_torque = self._torque.data_ptr()
        return g


class Table(Pair):
    """Tabulated pair potential (``hoomd.md.pair.Table``'s name; the reference has none, the semantics are defined in
    ``include/azp.h`` and DESIGN 4.21). ``params[(a, b)] = dict(r_min=float, U=array, F=array)``: ``width = len(U)``
    samples of the energy and of ``F = -dU/dr`` at ``r_min + k (r_cut - r_min) / width``; between them both are
    interpolated linearly, toward zero at ``r_cut`` in the last interval. Pairs closer than ``r_min`` or beyond
    ``r_cut`` contribute nothing. ``mode`` is always ``"none"``.

    There is no ``_azplugins`` class behind it: the tables of all type pairs live in one device tensor this object owns,
    ``(a, b)`` and ``(b, a)`` share their rows, and the parameter struct of a pair points at them."""

    _entry = "azp_pair_forces_table"
    _planned_entry = "azp_pair_forces_planned_table"
    _schema = dict(r_min=float, U=np.ndarray, F=np.ndarray)
    _accepted_modes = ("none",)

    def __init__(self, nlist, default_r_cut=None, default_r_on=0.0, mode="none"):
        super().__init__(nlist, default_r_cut=default_r_cut, default_r_on=default_r_on, mode=mode)
        self.params = TableTypeParameter("params", self._schema, 2, self._mark_dirty, self._readback)
        self.params.r_end = self._r_cut_if_known

    def _r_cut_if_known(self, key):
        try:
            return self.r_cut[key]
        except KeyError:
            return None

    def _readback(self, key):
        return None  # (params[...] hands back what was set: there is no C++ object that could hold anything else)

    def _build_tables(self):
        """Pack every type pair's samples for its current ``r_cut`` (``dr = (r_cut - r_min) / width``, so a changed
        ``r_cut`` repacks) into one device tensor and point the parameter structs at it."""
        import torch

        types = self._state.types
        T = len(types)
        dev = self._state.device
        name = type(self).__name__
        packed, first = {}, 0
        for i, a in enumerate(types):
            for b in types[i:]:
                d = self.params.get_raw((a, b))
                if d is None:
                    raise _lib.AzpError("%s.params[(%r, %r)] is not set" % (name, a, b))
                rc = self.r_cut[(a, b)]
                if rc == 0.0:
                    continue  # never evaluated: no rows
                rows = _lib.table_pack(d["r_min"], rc, d["U"], d["F"], closed=False)
                if rows is None:
                    raise _lib.AzpError("%s.params[(%r, %r)]: needs 0 <= r_min < r_cut and finite U, F of equal length "
                                        "(r_min = %g, r_cut = %g)" % (name, a, b, d["r_min"], rc))
                packed[(a, b)] = (first, rows)
                first += len(rows)
        all_rows = np.concatenate([rows for _, rows in packed.values()] + [np.zeros((1, 4))])
        d_rows = torch.from_numpy(all_rows).to(dev)
        assert d_rows.data_ptr() % 32 == 0
        entries, rc2, ro2 = [], np.zeros(T * T), np.zeros(T * T)
        for i, a in enumerate(types):
            for j, b in enumerate(types):
                key = (a, b) if i <= j else (b, a)
                rc2[i * T + j] = self.r_cut[key] ** 2
                ro2[i * T + j] = self.r_on[key] ** 2
                if key in packed:
                    at, rows = packed[key]
                    entries.append((self.params.get_raw(key)["r_min"], self.r_cut[key], d_rows.data_ptr() + 32 * at, len(rows)))
                else:
                    entries.append((0.0, 0.0, 0, 0))
        # argument structs kept by _compute_speculative and the plan's row classes refer to the old tensors and cutoffs
        self._spec_cache = None
        self._plan_builds = None
        self._tables = dict(params=torch.from_numpy(_lib.table_params_rows(entries)).to(dev), rcutsq=torch.from_numpy(rc2).to(dev),
                            ronsq=torch.from_numpy(ro2).to(dev), rows=d_rows)


__all__ = ["Colloid", "DPDGeneralWeight", "DPDConservativeGeneralWeight", "ExpandedYukawa", "Hertz",
           "PerturbedLennardJones", "Table", "TwoPatchMorse"]
