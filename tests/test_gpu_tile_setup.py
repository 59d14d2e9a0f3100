"""The tile kernel's per-tile set-up and its core / tail phases (pair_tiled.hpp).

The staging has two forms, chosen per launch (orthorhombic box periodic along every axis with the
r_list_max hint, or anything else), the row words and the words of a speculative launch are loaded
ahead of the staging, and split-energy instances walk the rows in a core phase and a tail phase
when the caller's displacement bound allows it. Same helpers and tolerances as
test_gpu_parity.py::test_planned_pair_parity and ::test_planned_after_particles_moved.
"""

import ctypes as C
import itertools

import numpy as np
import pytest

import helpers as H
from azplugins_amd import _lib
from azplugins_amd import synthetic as syn
from test_gpu_parity import assert_close, assert_per_particle

pytestmark = pytest.mark.gpu

NAME = "PerturbedLennardJones"
ENTRY = "azp_pair_forces_planned_perturbed_lennard_jones"
R_CUT, R_BUFF = 3.0, 0.4
R_WCA = 2.0 ** (1.0 / 6.0)   # sigma = 1
R_INNER = R_WCA + 0.33       # inner radius hint: the second lattice shell (1.52 +- jitter) straddles it
MARGIN = 1e-4                # what both plan compilers keep for their single-precision class test (plan_core_reach_sq)


def _launch(plan, a, p, t):
    import torch

    t["force"].fill_(float("nan"))
    t["virial"].fill_(float("nan"))
    status = getattr(_lib.lib(), ENTRY)(plan.handle, C.byref(a), p.data_ptr(), H._stream())
    torch.cuda.synchronize()
    return status


BOXES = [("ortho", p) for p in itertools.product((1, 0), repeat=3)] + [("triclinic", (1, 1, 1))]


@pytest.mark.parametrize("kind,periodic", BOXES, ids=["%s-%d%d%d" % ((k,) + p) for k, p in BOXES])
def test_box_flags(oracle, kind, periodic):
    """Every periodicity combination of an orthorhombic box and one triclinic box, each with the
    r_list_max hint (staged images trusted where the tile is compact) and without it: forces,
    energies and virial of the planned kernel against the oracle. 8,000 particles, 32 tiles."""
    cfg = syn.config_plj_sc(20)
    L = cfg["L"]
    tilt = (0.1, -0.05, 0.07) if kind == "triclinic" else (0.0, 0.0, 0.0)
    pos = syn.pos4(cfg["xyz"])
    box = oracle.make_box(L, tilt, periodic)
    params = oracle.pack_pair_params(NAME, cfg["params"])
    nl = oracle.build_nlist(pos, box, R_CUT + R_BUFF)
    f_ref, v_ref = oracle.pair_forces(NAME, pos, box, nl, params, R_CUT, mode="shift", virial=True, nthreads=8)
    for hint in (R_CUT + R_BUFF, 0.0):
        info = {}
        f_gpu, v_gpu = H.gpu_pair_forces(NAME, pos, (L, tilt, periodic), nl, params, R_CUT, mode="shift", virial=True, planned=True,
                                         plan_info=info, r_list_max=hint)
        assert info["valid"] == 1, info
        assert_close(f_gpu[:, :3], f_ref[:, :3], what="force, hint %g" % hint)
        assert_close(f_gpu[:, 3], f_ref[:, 3], what="energy, hint %g" % hint)
        assert_close(v_gpu, v_ref, what="virial, hint %g" % hint)
        assert_per_particle(f_gpu, f_ref)


@pytest.fixture(scope="module")
def core_case(oracle):
    """A plan built with the inner-radius hint, and a listed pair that lay just outside row class core then."""
    cfg = syn.config_plj_sc(20)
    L = cfg["L"]
    xyz = cfg["xyz"]
    pos = syn.pos4(xyz)
    box = oracle.make_box(L)
    nl = oracle.build_nlist(pos, box, R_CUT + R_BUFF)
    n_neigh, head, nlist = nl
    half = 0.5 * float(np.min(L))
    # a pair of interior particles (no wrapping between them) between R_INNER + 0.01 and R_INNER + 0.05 apart
    pair = None
    for i in np.nonzero(np.abs(xyz).max(axis=1) < half - 5.0)[0]:
        js = nlist[int(head[i]):int(head[i]) + int(n_neigh[i])].astype(np.int64)
        d = np.linalg.norm(xyz[js] - xyz[i], axis=1)
        ok = np.nonzero((d > R_INNER + 0.01) & (d < R_INNER + 0.05))[0]
        if ok.size:
            pair = (int(i), int(js[ok[0]]), float(d[ok[0]]))
            break
    assert pair is not None
    # ... and a pair of row class near (just inside the cutoff, beyond the plan's sure radius): its entries sit behind every core and sure entry of
    # their rows. Lower bound of their row positions: the neighbors closer than r_cut - r_buff - 0.01 (core or sure for
    # certain); upper bound of any slice's core-class count: the most neighbors any particle has within R_INNER + 0.001
    deep, behind = None, 0
    for i in np.nonzero(np.abs(xyz).max(axis=1) < half - 5.0)[0]:
        js = nlist[int(head[i]):int(head[i]) + int(n_neigh[i])].astype(np.int64)
        d = np.linalg.norm(xyz[js] - xyz[i], axis=1)
        ok = np.nonzero((d > R_CUT - 0.15) & (d < R_CUT - 0.05))[0]
        if ok.size and np.abs(xyz[js[ok[0]]]).max() < half - 5.0:
            j = int(js[ok[0]])
            dj = np.linalg.norm(xyz[nlist[int(head[j]):int(head[j]) + int(n_neigh[j])].astype(np.int64)] - xyz[j], axis=1)
            behind = min(int((d < R_CUT - R_BUFF - 0.01).sum()), int((dj < R_CUT - R_BUFF - 0.01).sum()))
            deep = (int(i), j, float(d[ok[0]]))
            break
    assert deep is not None
    # (all particles, periodic images included: count within the list, which reaches farther than R_INNER)
    owner = np.repeat(np.arange(len(n_neigh)), n_neigh.astype(np.int64))
    order = np.argsort(head.astype(np.int64), kind="stable")
    assert np.array_equal(order, np.arange(len(head)))  # rows stored in particle order
    dx = xyz[nlist.astype(np.int64)] - xyz[owner]
    dx -= L * np.rint(dx / L)
    core_most = int(np.bincount(owner, weights=(np.linalg.norm(dx, axis=1) < R_INNER + 1e-3), minlength=len(n_neigh)).max())
    # every slice's core phase ends at 8 * Kcore <= core_most + 7 entries: the deep pair's entries lie in the tail phase
    assert behind >= core_most + 7, (behind, core_most)
    return dict(cfg=cfg, pos=pos, box=box, nl=nl, pair=pair, deep=deep)


def _close_in(case, each, which="pair"):
    """Positions with the chosen pair moved towards each other by `each` per particle."""
    i, j, d = case[which]
    moved = case["pos"].copy()
    u = (moved[j, :3] - moved[i, :3]) / d
    moved[i, :3] += each * u
    moved[j, :3] -= each * u
    return moved


@pytest.mark.parametrize("mode", ["none", "shift"])
def test_core_phase_not_taken_when_a_pair_enters_the_core(oracle, core_case, mode):
    """A pair filed outside row class core moves into the WCA core. The bound that covers the move is
    too large for the tail phase (2 b exceeds the gap between the two radii), and so is no bound at
    all: the blended form must be found for that pair. A third launch sits one shell width inside
    the condition, the pair moved as far as that bound allows and still outside the WCA core: the
    tail phase is taken and must agree as well."""
    import torch

    cfg, nl, box = core_case["cfg"], core_case["nl"], core_case["box"]
    L = cfg["L"]
    params = oracle.pack_pair_params(NAME, cfg["params"])
    i, j, d = core_case["deep"]
    # (one lane per particle: the instances that have the two phases)
    a, t = H.gpu_pair_args(core_case["pos"], (L,), nl, 1, R_CUT, 0.0, mode, False, tpp=1, r_list_max=R_CUT + R_BUFF)
    ri = H._dev(np.array([R_INNER ** 2]))
    a.d_rinnersq = ri.data_ptr()
    p = H._dev(np.atleast_2d(params).astype(np.float64))
    plan = _lib.PairPlan()
    plan.build(a, H._stream())
    info = plan.info()
    assert info["valid"] == 1 and info["threads_per_particle"] == 1
    assert info["core_radius"] == pytest.approx(R_INNER - MARGIN, abs=1e-6) and d > info["sure_radius"] + 0.01
    # the rows reach well beyond the core phase (mean chunks: core class, ..., whole rows): there is a tail phase
    chunks = plan.phase_chunks()
    assert chunks[0] + 2 < chunks[2]

    # into the core: a pair of row class near, whose entries lie in the tail phase of both rows (core_case), ends 1.0
    # apart (< 2^(1/6)). The move is far beyond r_buff / 2; list and plan stay those of the build, for the oracle too.
    each = 0.5 * (d - 1.0)
    assert 2.0 * each > R_INNER - R_WCA and d - 2.0 * each < R_WCA
    moved = _close_in(core_case, each, "deep")
    f_ref = oracle.pair_forces(NAME, moved, box, nl, params, R_CUT, 0.0, mode, nthreads=8)
    t["pos"].copy_(torch.from_numpy(moved))
    for known, bound in ((1, each * (1 + 1e-12)), (0, 0.0)):
        a.has_displacement_bound, a.displacement_bound = known, bound
        assert _launch(plan, a, p, t) == 0
        f_gpu = t["force"].cpu().numpy()
        assert_close(f_gpu, f_ref, what="bound %g known %d" % (bound, known))
        assert_per_particle(f_gpu, f_ref)
    assert abs(f_ref[i, 3]) > 0 and np.linalg.norm(f_ref[i, :3]) > 10.0  # the core pair dominates its particles' forces

    # one shell width inside the condition sqrt(wca_rsq) + 2 b (1 + 1e-9) + m <= r_inner: the tail phase is taken (the
    # condition holds and the rows have one, above); the pair that lay just outside the core class closes in by 2 b
    i, j, d = core_case["pair"]
    w = R_BUFF / 16.0
    b = 0.5 * (R_INNER - R_WCA - MARGIN - w)
    assert R_WCA + 2.0 * b * (1 + 1e-9) + MARGIN <= R_INNER and d - 2.0 * b > R_WCA
    moved = _close_in(core_case, b)
    f_ref = oracle.pair_forces(NAME, moved, box, nl, params, R_CUT, 0.0, mode, nthreads=8)
    t["pos"].copy_(torch.from_numpy(moved))
    a.has_displacement_bound, a.displacement_bound = 1, b * (1 + 1e-12)
    assert _launch(plan, a, p, t) == 0
    f_gpu = t["force"].cpu().numpy()
    assert_close(f_gpu, f_ref, what="inside the condition")
    assert_per_particle(f_gpu, f_ref)


@pytest.mark.parametrize("mode", ["none", "shift"])
def test_core_phase_taken_or_not_same_bits(oracle, core_case, mode):
    """The same plan and positions launched with a bound that satisfies the condition and with no
    displacement information: the force arrays are equal as 64-bit words (the tail phase only skips
    a test whose outcome is known). bench.py --full verifies the same at full size."""
    import torch

    cfg, nl = core_case["cfg"], core_case["nl"]
    L = cfg["L"]
    params = oracle.pack_pair_params(NAME, cfg["params"])
    a, t = H.gpu_pair_args(core_case["pos"], (L,), nl, 1, R_CUT, 0.0, mode, False, tpp=1, r_list_max=R_CUT + R_BUFF)
    ri = H._dev(np.array([R_INNER ** 2]))
    a.d_rinnersq = ri.data_ptr()
    p = H._dev(np.atleast_2d(params).astype(np.float64))
    plan = _lib.PairPlan()
    plan.build(a, H._stream())
    assert plan.info()["valid"] == 1 and plan.info()["threads_per_particle"] == 1
    # every particle moves by up to b = 0.1: 2 b = 0.2 is below the gap of 0.33 - m, and half of the buffer is used
    b = 0.1
    tag = np.arange(core_case["pos"].shape[0], dtype=np.uint64)
    v = np.stack([syn.normal(5, tag, c) for c in range(3)], axis=1)
    v *= (b * syn.u01(6, tag, 0) ** (1.0 / 3.0) / np.linalg.norm(v, axis=1))[:, None]
    moved = core_case["pos"].copy()
    moved[:, :3] = syn.wrap(moved[:, :3] + v, L)
    t["pos"].copy_(torch.from_numpy(moved))
    out = {}
    for label, known, bound in (("phases", 1, b * (1 + 1e-12)), ("whole rows", 0, 0.0)):
        a.has_displacement_bound, a.displacement_bound = known, bound
        assert _launch(plan, a, p, t) == 0
        out[label] = t["force"].cpu().numpy().copy()
    assert np.isfinite(out["phases"]).all()
    assert np.array_equal(out["phases"].view(np.uint64), out["whole rows"].view(np.uint64))


def test_sub_range_launch(oracle):
    """8,000 + 37 particles; a launch over a sub-range whose tile count (20) is no multiple of 8:
    the rows of the covered tiles against the oracle, every other row untouched."""
    cfg = syn.config_plj_sc(21)
    L = cfg["L"]
    n = 8037
    pos = syn.pos4(cfg["xyz"][:n])
    box = oracle.make_box(L)
    params = oracle.pack_pair_params(NAME, cfg["params"])
    nl = oracle.build_nlist(pos, box, R_CUT + R_BUFF)
    f_ref = oracle.pair_forces(NAME, pos, box, nl, params, R_CUT, mode="shift", nthreads=8)
    a, t = H.gpu_pair_args(pos, (L,), nl, 1, R_CUT, 0.0, "shift", False, r_list_max=R_CUT + R_BUFF)
    p = H._dev(np.atleast_2d(params).astype(np.float64))
    plan = _lib.PairPlan()
    plan.build(a, H._stream())
    info = plan.info()
    assert info["valid"] == 1
    tile = info["tile_size"]
    # whole range first (N is no multiple of the tile)
    assert _launch(plan, a, p, t) == 0
    f_all = t["force"].cpu().numpy()
    assert_close(f_all, f_ref)
    first, count = 300, 5000
    a.range_first, a.range_count = first, count
    assert _launch(plan, a, p, t) == 0
    f_gpu = t["force"].cpu().numpy()
    lo, hi = (first // tile) * tile, min(-(-(first + count) // tile) * tile, n)
    assert ((hi - lo + tile - 1) // tile) % 8 != 0
    assert np.array_equal(f_gpu[lo:hi], f_all[lo:hi])
    assert np.isnan(f_gpu[:lo]).all() and np.isnan(f_gpu[hi:]).all()


def test_stale_exits_leave_the_output_untouched(oracle):
    """A launch whose d_stale_flag is set leaves at once: the pre-filled force array is unchanged and
    the call reports success, as before. The HOOMD-signature entry on a plan that turned out stale (the
    list rewritten in place) recompiles and returns the forces of the new list."""
    import torch

    cfg = syn.config_plj_sc(20)
    L = cfg["L"]
    pos = syn.pos4(cfg["xyz"])
    box = oracle.make_box(L)
    params = oracle.pack_pair_params(NAME, cfg["params"])
    nl = oracle.build_nlist(pos, box, R_CUT + R_BUFF)
    a, t = H.gpu_pair_args(pos, (L,), nl, 1, R_CUT, 0.0, "shift", False, r_list_max=R_CUT + R_BUFF)
    p = H._dev(np.atleast_2d(params).astype(np.float64))
    plan = _lib.PairPlan()
    plan.build(a, H._stream())
    assert plan.info()["valid"] == 1
    flag = torch.ones(1, dtype=torch.int32, device="cuda:0")
    bits = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    a.d_stale_flag, a.d_displacement_sq_bits = flag.data_ptr(), bits.data_ptr()
    t["force"].fill_(-7.25)
    status = getattr(_lib.lib(), ENTRY)(plan.handle, C.byref(a), p.data_ptr(), H._stream())
    torch.cuda.synchronize()
    assert status == 0
    assert bool((t["force"] == -7.25).all())
    # the flag cleared, displacement 0: the launch computes
    flag.zero_()
    assert _launch(plan, a, p, t) == 0
    f_ref = oracle.pair_forces(NAME, pos, box, nl, params, R_CUT, mode="shift", nthreads=8)
    assert_close(t["force"].cpu().numpy(), f_ref)

    # plan cache behind the HOOMD-signature entry: second call on a list that was rewritten in place
    lib = _lib.lib()
    lib.azp_pair_auto_plan_clear()
    a2, t2 = H.gpu_pair_args(pos, (L,), nl, 1, R_CUT, 0.0, "shift", False, r_list_max=R_CUT + R_BUFF, auto_plan=True)
    entry = getattr(lib, H.ENTRY[NAME])
    assert entry(C.byref(a2), p.data_ptr(), H._stream()) == 0
    torch.cuda.synchronize()
    assert_close(t2["force"].cpu().numpy(), f_ref)
    compiles = _lib.auto_plan_stats()["compiles"]
    # a shorter list (cut at r_cut + 0.2) written into the same buffers: the cached plan is stale
    nl_b = oracle.build_nlist(pos, box, R_CUT + 0.2)
    assert nl_b[2].size <= nl[2].size
    t2["n_neigh"].copy_(H._dev(nl_b[0], np.uint32))
    t2["head"].copy_(H._dev(nl_b[1], np.uint64))
    t2["nlist"][:nl_b[2].size].copy_(H._dev(nl_b[2], np.uint32))
    t2["force"].fill_(float("nan"))
    assert entry(C.byref(a2), p.data_ptr(), H._stream()) == 0
    torch.cuda.synchronize()
    f_ref_b = oracle.pair_forces(NAME, pos, box, nl_b, params, R_CUT, mode="shift", nthreads=8)
    assert_close(t2["force"].cpu().numpy(), f_ref_b)
    assert _lib.auto_plan_stats()["compiles"] == compiles + 1  # the speculative launch left, the plan was compiled again
    lib.azp_pair_auto_plan_clear()
