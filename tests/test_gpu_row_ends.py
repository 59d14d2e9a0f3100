"""Row ends of the tile plan counted in batches of 4 entries (half chunks), csrc/pair_plan*.hip, pair_tiled.hpp, xtiled.hpp.

A plan keeps, per slice (one wave of the force kernel) and per buffer shell, the number of BATCHES a wave has to walk; the
tile kernel runs count / 2 whole iterations and, for an odd count, one half iteration peeled off behind its loop. What
must hold: for every shell count a displacement bound can select, forces and energies are bit for bit those of the
whole-row launch on the same (moved) positions, and agree with the oracle on the moved positions with the old list --
for both plan compilers (from the cell list: what ``nlist.Cell.fused`` runs; from a HOOMD-format list: what runs with
it off), for slices with odd and with even counts, a count of 1 included, for the instances that do not take the
PerturbedLJ split path (two types, xplor, virial) and for the DPD / TwoPatchMorse kernels, which walk whole chunks
derived from the same counts.
"""
import ctypes as C

import numpy as np
import pytest

import helpers as H
from azplugins_amd import _lib
from azplugins_amd import synthetic as syn
from test_gpu_parity import PAIR_PARAMS, assert_close

pytestmark = pytest.mark.gpu

PLJ = "PerturbedLennardJones"
ENTRY = "azp_pair_forces_planned_perturbed_lennard_jones"


def _shells():
    return int(_lib.lib().azp_pair_plan_shells())


def _bound_for(n, w):
    """A displacement bound that selects exactly n shells of width w (n w >= 2 bound > (n - 1) w); the margin covers a
    width that differs from the expected one in its last single-precision bit."""
    return 0.5 * n * w * (1.0 - 1e-6)


def _moved(xyz, L, amp, seed):
    """Every particle displaced by at most amp, every second one by exactly amp (it sits ON the bound)."""
    n = xyz.shape[0]
    tag = np.arange(n, dtype=np.uint64)
    v = np.stack([syn.normal(seed, tag, c) for c in range(3)], axis=1)
    v *= (amp * syn.u01(seed, tag, 9) ** (1.0 / 3.0) / np.linalg.norm(v, axis=1))[:, None]
    v[::2] *= (amp / np.maximum(np.linalg.norm(v[::2], axis=1), 1e-300))[:, None]
    return syn.wrap(xyz + v, L)


def _blocked(cfg, n_side, block):
    """Memory order by blocks of block[0] x block[1] x block[2] lattice sites (256 sites: one tile is one compact block)."""
    a = cfg["L"][0] / n_side
    ijk = np.floor((cfg["xyz"] + 0.5 * cfg["L"]) / a + 1e-9).astype(np.int64) % n_side
    # (the jitter of 0.1 a around the site centres keeps every particle inside its own site)
    b = np.asarray(block)
    nb = n_side // b
    outer = ((ijk[:, 2] // b[2]) * nb[1] + ijk[:, 1] // b[1]) * nb[0] + ijk[:, 0] // b[0]
    inner = ((ijk[:, 2] % b[2]) * b[1] + ijk[:, 1] % b[1]) * b[0] + ijk[:, 0] % b[0]
    return cfg["xyz"][np.lexsort((inner, outer))]


def _thin_layers():
    """Square layers two lattice constants apart, r_cut between the first and the second in-plane neighbor distance:
    four entries in range per row (one batch), a few diagonal neighbors in the outer buffer shells."""
    nx, nz = 8, 32
    ix, iy, iz = np.meshgrid(np.arange(nx), np.arange(nx), np.arange(nz), indexing="ij")
    order = np.lexsort((ix.ravel(), iy.ravel(), iz.ravel()))
    L = np.array([float(nx), float(nx), 2.0 * nz])
    xyz = (np.stack([ix.ravel()[order], iy.ravel()[order], 2.0 * iz.ravel()[order]], axis=1) + 0.5) - 0.5 * L
    tag = np.arange(xyz.shape[0], dtype=np.uint64)
    xyz = xyz + 0.02 * (np.stack([syn.u01(41, tag, c) for c in range(3)], axis=1) - 0.5)
    return dict(xyz=syn.wrap(xyz, L), L=L, params=dict(epsilon=1.0, sigma=0.9, attraction_scale_factor=0.5), r_cut=1.2, r_buff=0.2)


def _workload(name):
    if name == "plj_sc20":
        return syn.config_plj_sc(20)
    if name == "north_star8":
        return syn.config_north_star(8)
    if name == "plj_sc32_blocked":
        # tiles narrow against the box (8 x 8 x 4 sites, L = 32 sites): the kernel trusts the staged images -- the loop
        # without the per-pair minimum image, which the two small boxes above never take
        cfg = syn.config_plj_sc(32)
        cfg["xyz"] = _blocked(cfg, 32, (8, 8, 4))
        return cfg
    assert name == "thin_layers"
    return _thin_layers()


_REF = {}


def _reference(oracle, name, shells):
    """Per workload, computed once: the oracle's list at the build positions and, for each shell count in ``shells``,
    (bound, moved positions, oracle forces on the moved positions with the OLD list)."""
    if name not in _REF:
        cfg = _workload(name)
        S = _shells()
        w = float(np.float32(cfg["r_buff"] / S))  # the plan publishes its width in single precision
        pos0 = syn.pos4(cfg["xyz"])
        box = oracle.make_box(cfg["L"])
        nl = oracle.build_nlist(pos0, box, cfg["r_cut"] + cfg["r_buff"])
        _REF[name] = dict(cfg=cfg, w=w, pos0=pos0, box=box, nl=nl, params=oracle.pack_pair_params(PLJ, cfg["params"]), steps={})
    ref = _REF[name]
    cfg = ref["cfg"]
    for n in shells:
        if n not in ref["steps"]:
            bound = _bound_for(n, ref["w"])
            moved = syn.pos4(_moved(cfg["xyz"], cfg["L"], bound, seed=300 + n))
            f = oracle.pair_forces(PLJ, moved, ref["box"], ref["nl"], ref["params"], cfg["r_cut"], 0.0, "shift", nthreads=8)
            ref["steps"][n] = (bound, moved, f)
    return ref


def _plan(compiler, pos, L, nl, r_cut, r_buff, ntypes=1, mode="shift", r_on=0.0, virial=False, r_inner=None):
    """A plan compiled at ``pos`` by one of the two compilers, and pair arguments bound to it."""
    rc = np.broadcast_to(np.asarray(r_cut, dtype=np.float64), (ntypes, ntypes))
    hint = float(rc.max() + 2 * r_buff)
    keep = None
    plan = _lib.PairPlan()
    if compiler == "cells":
        cells, keep = H.gpu_cells(pos, (L,), np.where(rc > 0, rc + r_buff, 0.0), ntypes)
        n = pos.shape[0]
        dummy = (np.zeros(n, np.uint32), np.zeros(n, np.uint64), np.zeros(1, np.uint32))
        a, t = H.gpu_pair_args(pos, (L,), dummy, ntypes, r_cut, r_on, mode, virial, r_list_max=hint)
        a.d_n_neigh = keep["n_neigh"].data_ptr()
    else:
        a, t = H.gpu_pair_args(pos, (L,), nl, ntypes, r_cut, r_on, mode, virial, r_list_max=hint)
    if r_inner is not None:
        t["rinnersq"] = H._dev(np.full(ntypes * ntypes, float(r_inner) ** 2))
        a.d_rinnersq = t["rinnersq"].data_ptr()
    if compiler == "cells":
        plan.build_from_cells(cells, a, H._stream())
        info = plan.info()
        a.d_nlist, a.d_head_list, a.size_nlist = info["list_id"], info["head_id"], 0
    else:
        plan.build(a, H._stream())
        info = plan.info()
    assert info["valid"] == 1 and info["from_cells"] == (1 if compiler == "cells" else 0) and info["threads_per_particle"] == 1
    t["keep"] = keep
    return plan, a, t


def _run(plan, a, t, p, moved, bound, virial=False):
    """The planned kernel on ``moved`` with the bound (None: whole rows)."""
    import torch

    t["pos"].copy_(torch.from_numpy(np.ascontiguousarray(moved)).to("cuda:0"))
    t["force"].fill_(float("nan"))
    a.has_displacement_bound, a.displacement_bound = (0, 0.0) if bound is None else (1, float(bound))
    _lib.check(getattr(_lib.lib(), ENTRY)(plan.handle, C.byref(a), p.data_ptr(), H._stream()), ENTRY)
    out = H._finish(t, virial)
    return (out[0].copy(), out[1].copy()) if virial else out.copy()


def _counts(plan, ref):
    """Batch counts of the slices that hold particles, [slice, 0 .. PLAN_SHELLS], and the shell width; the bounds of the
    reference steps select the shell counts they were made for."""
    S = _shells()
    counts, w = plan.row_batches()
    assert counts.shape == (4 * plan.info()["n_tiles"], S + 1) and abs(w - ref["w"]) <= 2e-7 * w
    for n, (bound, _, _) in ref["steps"].items():
        assert _lib.lib().azp_pair_plan_shells_for(w, 1, bound) == n
    return counts[: -(-ref["pos0"].shape[0] // 64)], w


def _r_inner(cfg):
    """What azplugins_amd.pair passes for PerturbedLJ: the plan then builds its core and sure row classes."""
    return 2.0 ** (1.0 / 6.0) * cfg["params"]["sigma"] + cfg["r_buff"] + 1e-3


@pytest.mark.parametrize("compiler", ["cells", "list"])
@pytest.mark.parametrize("name", ["plj_sc20", "north_star8"])
def test_every_shell_count_equals_whole_rows(oracle, name, compiler):
    """(i), (ii): shell counts 0 ... PLAN_SHELLS through the displacement bound, particles moved onto the bound after the
    plan was compiled; the counts of the shells walked are read back and must be odd for some slices and even for others."""
    S = _shells()
    ref = _reference(oracle, name, range(S + 1))
    cfg = ref["cfg"]
    plan, a, t = _plan(compiler, ref["pos0"], cfg["L"], ref["nl"], cfg["r_cut"], cfg["r_buff"], r_inner=_r_inner(cfg))
    counts, w = _counts(plan, ref)
    assert np.all(np.diff(counts.astype(np.int64), axis=1) >= 0) and counts[:, 0].min() >= 1
    if compiler == "list":  # whole rows: ceil(longest row of the slice / 4)
        longest = np.pad(ref["nl"][0], (0, -len(ref["nl"][0]) % 64)).reshape(-1, 64).max(axis=1)
        assert np.array_equal(counts[:, S], (longest + 3) // 4)
    p = H._dev(np.atleast_2d(ref["params"]).astype(np.float64))
    both = 0
    for n in range(S + 1):
        bound, moved, f_ref = ref["steps"][n]
        odd = int((counts[:, n] & 1).sum())
        print("%s %s shells %d: batches %d..%d, odd in %d of %d slices" % (name, compiler, n, counts[:, n].min(), counts[:, n].max(),
                                                                         odd, counts.shape[0]))
        both += 0 < odd < counts.shape[0]
        f_bound = _run(plan, a, t, p, moved, bound)
        f_whole = _run(plan, a, t, p, moved, None)
        assert np.array_equal(f_bound, f_whole), "shells %d" % n
        assert_close(f_bound, f_ref, what="shells %d" % n)
    assert both >= 1  # some launch ran the peeled half iteration in some waves and not in others


@pytest.mark.parametrize("compiler", ["cells", "list"])
def test_rows_of_a_single_batch(oracle, compiler):
    """(ii), Kb = 1: four in-range entries per row, so with bound 0 every wave runs no whole iteration at all, only the
    half iteration on the gathers of the prologue."""
    S = _shells()
    shells = (0, 1, S // 2, S)
    ref = _reference(oracle, "thin_layers", shells)
    cfg = ref["cfg"]
    assert ref["nl"][0].max() > 4
    plan, a, t = _plan(compiler, ref["pos0"], cfg["L"], ref["nl"], cfg["r_cut"], cfg["r_buff"], r_inner=_r_inner(cfg))
    counts, w = _counts(plan, ref)
    assert np.all(counts[:, 0] == 1) and counts[:, S].max() >= 2
    p = H._dev(np.atleast_2d(ref["params"]).astype(np.float64))
    for n in shells:
        bound, moved, f_ref = ref["steps"][n]
        f_bound = _run(plan, a, t, p, moved, bound)
        assert np.array_equal(f_bound, _run(plan, a, t, p, moved, None)), "shells %d" % n
        assert_close(f_bound, f_ref, what="shells %d" % n)


@pytest.mark.parametrize("compiler", ["cells", "list"])
def test_narrow_tiles_take_the_loop_without_minimum_image(oracle, compiler):
    S = _shells()
    shells = (0, 1, S // 2, S - 1)
    ref = _reference(oracle, "plj_sc32_blocked", shells)
    cfg = ref["cfg"]
    plan, a, t = _plan(compiler, ref["pos0"], cfg["L"], ref["nl"], cfg["r_cut"], cfg["r_buff"], r_inner=_r_inner(cfg))
    counts, w = _counts(plan, ref)
    p = H._dev(np.atleast_2d(ref["params"]).astype(np.float64))
    both = 0
    for n in shells:
        bound, moved, f_ref = ref["steps"][n]
        odd = int((counts[:, n] & 1).sum())
        both += 0 < odd < counts.shape[0]
        f_bound = _run(plan, a, t, p, moved, bound)
        assert np.array_equal(f_bound, _run(plan, a, t, p, moved, None)), "shells %d" % n
        assert_close(f_bound, f_ref, what="shells %d" % n)
    assert both >= 1


@pytest.mark.parametrize("variant", ["two_types", "xplor", "virial"])
def test_instances_off_the_split_path_at_an_odd_count(oracle, variant):
    """(iii): the evaluator's plain form (per-pair coefficient lookup, xplor smoothing, virial accumulation) in the peeled
    half iteration."""
    S = _shells()
    cfg = syn.config_plj_sc(20)
    T = 2 if variant == "two_types" else 1
    mode = "xplor" if variant == "xplor" else "shift"
    virial = variant == "virial"
    n_part = cfg["xyz"].shape[0]
    typeid = (syn.hash64(17, np.arange(n_part, dtype=np.uint64), 7) % np.uint64(T)).astype(np.int64)
    pos0 = syn.pos4(cfg["xyz"], typeid)
    box = oracle.make_box(cfg["L"])
    r_cut, r_buff = cfg["r_cut"], cfg["r_buff"]
    tab = H.sym_table(T, PAIR_PARAMS[PLJ])
    params = np.array([oracle.pack_pair_params(PLJ, tab[i][j]) for i in range(T) for j in range(T)])
    nl = oracle.build_nlist(pos0, box, r_cut + r_buff, ntypes=T)
    plan, a, t = _plan("cells", pos0, cfg["L"], nl, r_cut, r_buff, ntypes=T, mode=mode, r_on=0.8 * r_cut, virial=virial)
    counts, w = plan.row_batches()
    counts = counts[: -(-n_part // 64)]
    odd = [n for n in range(1, S) if (counts[:, n] & 1).any()]
    assert odd
    n = odd[len(odd) // 2]
    bound = _bound_for(n, w)
    moved = syn.pos4(_moved(cfg["xyz"], cfg["L"], bound, seed=500), typeid)
    ref = oracle.pair_forces(PLJ, moved, box, nl, params, r_cut, 0.8 * r_cut, mode, ntypes=T, virial=virial, nthreads=8)
    p = H._dev(np.atleast_2d(params).astype(np.float64))
    got = _run(plan, a, t, p, moved, bound, virial)
    whole = _run(plan, a, t, p, moved, None, virial)
    if virial:
        assert np.array_equal(got[0], whole[0]) and np.array_equal(got[1], whole[1])
        assert_close(got[0], ref[0])
        assert_close(got[1], ref[1], what="virial")
    else:
        assert np.array_equal(got, whole)
        assert_close(got, ref)


@pytest.mark.parametrize("kind", ["dpd", "tpm"])
def test_chunk_walking_kernels_mid_cycle(oracle, kind):
    """(iv): the DPD thermostat and TwoPatchMorse kernels walk (count + 1) / 2 whole chunks of the same tables: a
    mid-cycle bound, particles moved onto it after the plan was compiled, against the oracle with the old list."""
    import torch

    S = _shells()
    r_buff = 0.4
    if kind == "dpd":
        cfg = syn.config_dpd(6000)
        r_cut, mode = 1.0, "none"
    else:
        cfg = syn.config_tpm(12, 12, 16)
        r_cut, mode = 1.6, "shift"
    n_part = cfg["xyz"].shape[0]
    pos0 = syn.pos4(cfg["xyz"])
    box = oracle.make_box(cfg["L"])
    nl = oracle.build_nlist(pos0, box, r_cut + r_buff)
    a, t = H.gpu_pair_args(pos0, (cfg["L"],), nl, 1, r_cut, 0.0, mode, False, r_list_max=r_cut + 2 * r_buff)
    plan = _lib.PairPlan()
    plan.build(a, H._stream())
    assert plan.info()["valid"] == 1
    counts, w = plan.row_batches()
    counts = counts[: -(-n_part // 64)]
    # a mid-cycle shell count at which some slice has an odd count (its last chunk is walked whole), if there is one
    odd = [n for n in range(1, S) if (counts[:, n] & 1).any()]
    n = min(odd, key=lambda m: abs(m - S // 2)) if odd else S // 2
    bound = _bound_for(n, w)
    moved = syn.pos4(_moved(cfg["xyz"], cfg["L"], bound, seed=700))
    t["pos"].copy_(torch.from_numpy(moved))
    a.has_displacement_bound, a.displacement_bound = 1, bound
    if kind == "dpd":
        vel = np.zeros((n_part, 4))
        vel[:, :3] = cfg["vel"]
        vel[:, 3] = 1.0
        params = np.atleast_2d(oracle.pack_pair_params("DPDGeneralWeight", cfg["params"]))
        f_ref = oracle.dpd_forces(moved, vel, cfg["tag"], box, nl, params, r_cut, 1.0, 0.01, 7, 99)
        p, v, tg = H._dev(params), H._dev(vel), H._dev(cfg["tag"], np.uint32)
        d = _lib.DPDArgs()
        d.pair = a
        d.d_vel, d.d_tag = v.data_ptr(), tg.data_ptr()
        d.timestep, d.deltaT, d.T, d.seed = 99, 0.01, 1.0, 7
        _lib.check(_lib.lib().azp_dpd_forces_planned_general_weight(plan.handle, C.byref(d), p.data_ptr(), H._stream()), "planned dpd")
        assert_close(H._finish(t, False), f_ref, what="dpd")
    else:
        params = np.atleast_2d(oracle.pack_pair_params("TwoPatchMorse", cfg["params"]))
        f_ref, t_ref = oracle.aniso_forces_tpm(moved, cfg["orientation"], box, nl, params, r_cut, mode)
        p, q = H._dev(params), H._dev(cfg["orientation"], np.float64)
        tq = torch.full((n_part, 4), float("nan"), dtype=torch.float64, device="cuda:0")
        g = _lib.AnisoArgs()
        g.pair = a
        g.d_orientation, g.d_torque = q.data_ptr(), tq.data_ptr()
        _lib.check(_lib.lib().azp_aniso_forces_planned_two_patch_morse(plan.handle, C.byref(g), p.data_ptr(), H._stream()), "planned tpm")
        f = H._finish(t, False)
        assert_close(f[:, :3], f_ref[:, :3], what="tpm force")
        assert_close(f[:, 3], f_ref[:, 3], what="tpm energy")
        assert_close(tq.cpu().numpy()[:, :3], t_ref[:, :3], what="tpm torque")
