"""Row lengths through the unrolled pair loop of the phased tile instances (tiled_loop_phases, pair_tiled.hpp).

The tail phase of a row runs three iterations per trip with the index words rotating through three names, the left-over
one or two iterations through a single-iteration body, and an odd batch count ends in the peeled half iteration; the core
phase hands its names over to the tail phase wherever it ends. What can go wrong there are the remainders and the
hand-over, so the launches below are chosen for their batch counts Kb (per slice, per shell count): every residue
modulo 6 (twice the unroll factor), rows of 0, 1 and 2 batches, and core phases of no iteration, of part of the row,
of all Kb / 2 iterations and of more than the row has. Forces and energies are compared with the oracle at the parity tests'
tolerance, and bit for bit with the launch that walks whole rows and tests every batch (no displacement
information: the form of tiled_loop).

4,096 particles of synthetic.config_plj_sc(16) in 16 tiles, stored so that one tile is one block of 8 x 8 x 4 lattice
sites with its first particle in the middle: every tile is narrow against the box, which the test checks with the
kernel's own criterion -- a wide tile would run tiled_loop with the per-pair minimum image and none of the above.
"""
import numpy as np
import pytest

import helpers as H
from azplugins_amd import synthetic as syn
from test_gpu_parity import assert_close
from test_gpu_row_ends import PLJ, _bound_for, _moved, _plan, _run

pytestmark = pytest.mark.gpu

N_SIDE = 16
BLOCK = (8, 8, 4)
R_BUFF = 0.4
UNROLL = 3
MARGIN = 1e-3  # separations this close to the inner radius count as "either side" (the plan classifies in single precision)

# sigma, r_cut, inner radius (None: the one azplugins_amd.pair passes, r_wca + r_buff + 1e-3) and the shell counts launched.
# Every case keeps r_wca + 2 b + 2e-4 <= r_inner <= r_cut: the first is the launcher's condition for the tail phase
# (plan_core_reach_sq), the second is what that condition takes for granted -- the plan compilers file only in-range
# entries in class core, so with r_inner > r_cut a buffer-shell entry closer than r_inner is not covered by the core
# count (profiles/pair_loop.md, "Found on the way").
CASES = {
    "long_rows": dict(sigma=1.0, r_cut=3.0, r_inner=None, shells=(0, 3, 7, 12)),   # 22 - 32 batches, core phase of 2 iterations
    "mid_rows": dict(sigma=1.0, r_cut=2.5, r_inner=None, shells=(0, 3, 7, 12)),    # 14 - 21 batches
    # at most the 6 nearest lattice neighbors in range, all of them core class: 1 - 2 batches at bound 0, core phase of
    # one iteration -- as long as the row or longer
    "short_rows": dict(sigma=0.9, r_cut=1.25, r_inner=1.25, shells=(0, 3, 6, 9)),
    # one to three of them in range: one batch at bound 0, no whole iteration, and a core phase of one
    "one_batch": dict(sigma=0.8, r_cut=1.0, r_inner=1.0, shells=(0, 2, 4)),
    # nearest pair of the lattice 0.86: nothing in range at bound 0 (Kb = 0), no core class
    "empty_rows": dict(sigma=0.6, r_cut=0.8, r_inner=0.8, shells=(0, 2, 5)),
    # r_wca = 0.673: core class empty, Kcore = 0 on long rows
    "no_core": dict(sigma=0.6, r_cut=3.0, r_inner=0.85, shells=(0, 3, 7)),
}


def _tiles_first_in_the_middle(cfg):
    """Memory order by blocks of BLOCK sites, inside a block by distance from its middle (nearest first)."""
    a = cfg["L"][0] / N_SIDE
    ijk = np.floor((cfg["xyz"] + 0.5 * cfg["L"]) / a + 1e-9).astype(np.int64) % N_SIDE
    b = np.asarray(BLOCK)
    nb = N_SIDE // b
    outer = ((ijk[:, 2] // b[2]) * nb[1] + ijk[:, 1] // b[1]) * nb[0] + ijk[:, 0] // b[0]
    off = (ijk % b) - b // 2
    inner = (off * off).sum(axis=1) * 1000 + ((off[:, 2] + 8) * 16 + off[:, 1] + 8) * 16 + off[:, 0] + 8
    return cfg["xyz"][np.lexsort((inner, outer))]


def _assert_narrow(pos, L, r_list_max):
    """The kernel's test, per tile: every member's image nearest the tile's first particle lies closer to it than
    L / 2 - r_list_max on each axis (then the staged images are trusted and the phased loop runs)."""
    xyz = pos[:, :3]
    assert xyz.shape[0] % 256 == 0
    c = np.repeat(xyz[::256], 256, axis=0)
    d = xyz - c
    d -= L * np.rint(d / L)
    assert np.all(np.abs(d) + r_list_max < 0.5 * L)


_CASE = {}


def _case(oracle, name):
    if name not in _CASE:
        spec = CASES[name]
        cfg = syn.config_plj_sc(N_SIDE)
        assert cfg["xyz"].shape[0] == 4096
        cfg["xyz"] = _tiles_first_in_the_middle(cfg)
        cfg["params"] = dict(cfg["params"], sigma=spec["sigma"])
        r_cut = spec["r_cut"]
        r_wca = 2.0 ** (1.0 / 6.0) * spec["sigma"]
        r_inner = spec["r_inner"] if spec["r_inner"] is not None else r_wca + R_BUFF + 1e-3
        assert r_inner <= r_cut
        pos0 = syn.pos4(cfg["xyz"])
        box = oracle.make_box(cfg["L"])
        nl = oracle.build_nlist(pos0, box, r_cut + R_BUFF)
        _assert_narrow(pos0, cfg["L"], r_cut + 2 * R_BUFF)
        # core-class entries per row, bracketed: separations below r_inner -+ MARGIN
        n_neigh, head, nlist = nl
        owner = np.repeat(np.arange(len(n_neigh)), n_neigh.astype(np.int64))
        assert np.array_equal(np.argsort(head.astype(np.int64), kind="stable"), np.arange(len(head)))
        dx = cfg["xyz"][nlist.astype(np.int64)] - cfg["xyz"][owner]
        dx -= cfg["L"] * np.rint(dx / cfg["L"])
        dist = np.linalg.norm(dx, axis=1)
        core = [np.bincount(owner, weights=(dist < r_inner + s * MARGIN), minlength=len(n_neigh)).astype(np.int64) for s in (-1, 1)]
        # chunks (8 entries per lane) that cover the core entries of a slice's 64 rows: lower and upper bracket
        kcore = [(-(-c.reshape(-1, 64).max(axis=1) // 8)) for c in core]
        _CASE[name] = dict(cfg=cfg, pos0=pos0, box=box, nl=nl, r_cut=r_cut, r_inner=r_inner, r_wca=r_wca, kcore=kcore,
                           params=oracle.pack_pair_params(PLJ, cfg["params"]))
    return _CASE[name]


def _paths(case, counts, shells, w):
    """What the launches of one case exercise: residues of Kb modulo twice the unroll factor, the short rows among
    them, and how the core phase (bracketed from the oracle's list) relates to the row's whole iterations."""
    lo, hi = case["kcore"]
    seen = dict(residues=set(), lengths=set(), kcore=set())
    for n in shells:
        # the launch takes the tail phase: sqrt(wca_rsq) + 2 b (1 + 1e-9) + 1e-4 <= r_inner (plan_core_reach_sq)
        assert case["r_wca"] + 2.0 * _bound_for(n, w) * (1 + 1e-9) + 1e-4 <= case["r_inner"] - 1e-4
        Kb = counts[:, n]
        K = Kb // 2
        seen["residues"].update((Kb % (2 * UNROLL)).tolist())
        seen["lengths"].update(Kb[Kb <= 2].tolist())
        for label, hit in (("none", (hi == 0) & (K > 0)), ("part", (lo > 0) & (hi < K)), ("all", (lo == K) & (hi == K) & (K > 0)),
                           ("above", lo > K)):
            if np.any(hit):
                seen["kcore"].add(label)
    return seen


def _counts(plan):
    counts, w = plan.row_batches()
    return counts[: 4096 // 64].astype(np.int64), w


@pytest.mark.parametrize("mode", ["shift", "none"])
@pytest.mark.parametrize("name", list(CASES))
def test_row_lengths(oracle, name, mode):
    case = _case(oracle, name)
    cfg = case["cfg"]
    shells = CASES[name]["shells"]
    plan, a, t = _plan("list", case["pos0"], cfg["L"], case["nl"], case["r_cut"], R_BUFF, mode=mode, r_inner=case["r_inner"])
    counts, w = _counts(plan)
    print(name, mode, {k: sorted(v) for k, v in _paths(case, counts, shells, w).items()})
    p = H._dev(np.atleast_2d(case["params"]).astype(np.float64))
    for n in shells:
        bound = _bound_for(n, w)
        moved = syn.pos4(_moved(cfg["xyz"], cfg["L"], bound, seed=900 + n))
        f_ref = oracle.pair_forces(PLJ, moved, case["box"], case["nl"], case["params"], case["r_cut"], 0.0, mode, nthreads=8)
        f_bound = _run(plan, a, t, p, moved, bound)
        f_whole = _run(plan, a, t, p, moved, None)
        differ = np.nonzero((f_bound.view(np.uint64) != f_whole.view(np.uint64)).any(axis=1))[0]
        print("  shells %d: Kb %d..%d, whole rows %d..%d, rows that differ from the whole-row launch: %d %s" % (
            n, counts[:, n].min(), counts[:, n].max(), counts[:, -1].min(), counts[:, -1].max(), differ.size,
            [(int(i), f_bound[i].tolist(), f_whole[i].tolist(), f_ref[i].tolist()) for i in differ[:3]]))
        assert np.array_equal(f_bound.view(np.uint64), f_whole.view(np.uint64)), "%s shells %d" % (name, n)
        assert_close(f_bound[:, :3], f_ref[:, :3], what="%s force, shells %d" % (name, n))
        assert_close(f_bound[:, 3], f_ref[:, 3], what="%s energy, shells %d" % (name, n))


def test_row_lengths_cover_every_path(oracle):
    """The launches of test_row_lengths, taken together: every residue of Kb modulo twice the unroll factor, rows of
    0, 1 and 2 batches, and core phases of no iteration, of part of the row, of exactly the row's whole iterations and
    of more than it has."""
    seen = dict(residues=set(), lengths=set(), kcore=set())
    for name in CASES:
        case = _case(oracle, name)
        plan, a, t = _plan("list", case["pos0"], case["cfg"]["L"], case["nl"], case["r_cut"], R_BUFF, r_inner=case["r_inner"])
        counts, w = _counts(plan)
        for key, val in _paths(case, counts, CASES[name]["shells"], w).items():
            seen[key] |= val
    assert seen["residues"] == set(range(2 * UNROLL)), seen
    assert seen["lengths"] == {0, 1, 2}, seen
    assert seen["kcore"] == {"none", "part", "all", "above"}, seen
