"""The cell-list row builder (csrc/nlist.hip: azp_nlist_count / azp_nlist_fill, kernel nlist_cell_kernel<FILL, MI>)
through the C ABI, every row of every case against the all-pairs FP64 reference of tests/nlist_ref.py.

The comparison is exact set equality: the generated configurations hold no pair within 1e-9 (relative, in r^2) of
its cutoff -- asserted on the reference, the generator reseeds until it holds -- while the two implementations'
r^2 differ by rounding alone (~1e-13 relative at these box sizes).

Which kernel instance a grid selects (nlist_scan): MI = true (minimum image per pair) when some PERIODIC axis has
fewer than 4 cells, else MI = false (images resolved once per staged candidate, relative to the home cell's centre).
"""

import functools

import numpy as np
import pytest

import helpers as H
import nlist_ref as R
from azplugins_amd import synthetic as syn

pytestmark = pytest.mark.gpu

SENT = H.NLIST_SENTINEL
INVALID_ARGUMENT = -1  # AZP_ERROR_INVALID_ARGUMENT (include/azp.h)
WIDTH = 1.07           # cell width in units of the largest r_list: floor(L / r_list) cells, 2.14 r_list on 2 cells

# three types, distinct radii, the pair 1-2 disabled (r_list = 0 -> rlistsq <= 0)
RL3 = np.array([[1.0, 0.8, 0.6], [0.8, 0.9, 0.0], [0.6, 0.0, 0.7]])
# type 2 disabled against everything: its rows are empty and nobody lists it
RL3_DEAD = np.array([[1.0, 0.8, 0.0], [0.8, 0.9, 0.0], [0.0, 0.0, 0.0]])


# ---------------------------------------------------------------------------
# configurations
# ---------------------------------------------------------------------------
def _uniform(seed, n, lo, hi):
    tag = np.arange(n, dtype=np.uint64)
    lo, hi = np.broadcast_to(lo, (3,)), np.broadcast_to(hi, (3,))
    return np.stack([lo[c] + syn.u01(seed, tag, c) * (hi[c] - lo[c]) for c in range(3)], axis=1)


def _types(seed, n, ntypes):
    return (syn.hash64(seed + 500, np.arange(n, dtype=np.uint64), 9) % np.uint64(ntypes)).astype(np.int64)


def liquid(dims, rl, n, seed, empty="last"):
    """n uniformly random particles (a liquid's lack of order) in a box of dims cells of WIDTH * max r_list, one cell
    left empty (its particles moved into the cell at the opposite corner), and 12 particles on the faces: per axis
    one exactly on +L/2, one on -L/2, one 1e-12 inside each (their other coordinates in the first cell)."""
    dims = np.asarray(dims)
    w = WIDTH * float(np.max(rl))
    L = dims * w
    xyz = _uniform(seed, n, -0.5 * L, 0.5 * L)
    cell = np.minimum(np.floor((xyz + 0.5 * L) / w).astype(np.int64), dims - 1)
    if empty == "last":
        xyz[np.all(cell == dims - 1, axis=1)] -= (dims - 1) * w
    elif empty == "first":
        xyz[np.all(cell == 0, axis=1)] += (dims - 1) * w
    if empty != "first":
        face = _uniform(seed + 1, 12, -0.5 * L, -0.5 * L + 0.5 * w)
        for k in range(3):
            face[4 * k: 4 * k + 4, k] = [0.5 * L[k], -0.5 * L[k], 0.5 * L[k] - 1e-12, -0.5 * L[k] + 1e-12]
        xyz[:12] = face
    return xyz, L


def settled(make, seed):
    """make(seed) -> dict(pos, L, periodic, rl, N[, tilt, exclusions]) and its reference, for the first seed (seed,
    seed + 100, ...) whose configuration has no borderline pair."""
    for s in range(seed, seed + 1000, 100):
        cfg = make(s)
        ref = R.all_pairs_rows(cfg["pos"], cfg["L"], cfg.get("tilt", (0, 0, 0)), cfg["periodic"], cfg["rl"], cfg["N"],
                               cfg.get("exclusions"))
        if ref[2] == 0:
            return cfg, ref
    raise AssertionError("no configuration without a borderline pair in 10 seeds")


def build_rows(cfg, row_capacity=0, dims=None, excl_pitch=None):
    rl = np.asarray(cfg["rl"], dtype=np.float64)
    a, t = H.gpu_cells(cfg["pos"], (cfg["L"], cfg.get("tilt", (0, 0, 0)), cfg["periodic"]), rl, ntypes=rl.shape[0], N=cfg["N"],
                       exclusions=cfg.get("exclusions"), dims=dims, excl_pitch=excl_pitch)
    return H.gpu_nlist_rows(a, t, row_capacity=row_capacity), a, t


def gpu_rows(out, n_neigh):
    return [np.sort(out["nlist"][h: h + n]) for h, n in zip(out["head"], n_neigh)]


def assert_exact_rows(out, ref):
    """Count-then-fill output == reference: d_n_neigh of the count pass, EVERY row as a sorted array (equal sorted
    arrays: the same set and no duplicate), nothing written behind the N counts or behind the last row."""
    ref_n, ref_rows, borderline = ref
    assert borderline == 0
    assert out["rc_count"] == 0 and out["rc_fill"] == 0
    assert np.array_equal(out["n_count"], ref_n), "d_n_neigh: first bad row %d" % int(np.flatnonzero(out["n_count"] != ref_n)[0])
    assert np.array_equal(out["n_neigh"], ref_n)  # (the exact fill leaves the counts alone)
    assert np.all(out["n_guard"] == SENT)
    size = int(ref_n.sum())
    assert out["size"] == size
    nl = out["nlist"]
    assert np.all(nl[size:] == SENT) and nl.size > size
    want = np.concatenate(ref_rows) if size else np.zeros(0, dtype=np.int64)
    row_id = np.repeat(np.arange(ref_n.size), ref_n)
    got = nl[:size][np.lexsort((nl[:size], row_id))]
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "row %d differs from the reference (%d words in all)" % (row_id[bad[0]], bad.size)


def cells_of(a, t):
    """(particles of every cell as a list of index arrays) from the binning the builder read."""
    ncell = int(a.grid.dim[0]) * int(a.grid.dim[1]) * int(a.grid.dim[2])
    start = t["cell_start"].cpu().numpy()[: ncell + 1]
    order = t["order"].cpu().numpy()
    return [order[start[c]: start[c + 1]] for c in range(ncell)]


# ---------------------------------------------------------------------------
# instances and stencils
# ---------------------------------------------------------------------------
#   cells      periodic axes -> instance
#   (2,2,2)    any periodic axis has 2 cells: MI = true, and the "visit each cell of the axis once" stencil (d < 3)
#   (3,3,3)    any periodic axis has 3 cells: MI = true, the wrapped stencil reaches all three cells
#   (4,4,4)    MI = false for every periodicity
#   (2,3,5)    MI = true when x or y is periodic ((1,1,1), (0,1,1), (1,0,1)); (0,0,0): MI = false
#   (1,4,4)    x non-periodic (one cell; L_x < 2 r_list would not be a legal periodic axis): MI = false
#   (5,4,6)    MI = false for every periodicity
#   (0,0,0) periodicity selects MI = false for every grid (the clipped stencil alone)
DIMS = [(2, 2, 2), (3, 3, 3), (4, 4, 4), (2, 3, 5), (1, 4, 4), (5, 4, 6)]
PERIODIC = [(1, 1, 1), (0, 1, 1), (1, 0, 1), (0, 0, 0)]
STENCIL_CASES = [(d, p) for d in DIMS for p in PERIODIC if all(d[k] >= 2 or not p[k] for k in range(3))]


@pytest.mark.parametrize("dims,periodic", STENCIL_CASES, ids=lambda v: "".join(str(x) for x in v))
def test_rows_for_every_stencil(dims, periodic):
    ncell = dims[0] * dims[1] * dims[2]
    n = min(2400, 60 * ncell) + 13

    def make(seed):
        xyz, L = liquid(dims, RL3, n, seed)
        return dict(pos=syn.pos4(xyz, _types(seed, n, 3)), L=L, periodic=periodic, rl=RL3, N=n)

    cfg, ref = settled(make, 11 + ncell)
    for k in range(3):
        assert not periodic[k] or cfg["L"][k] >= 2.1 * RL3.max()
    out, a, t = build_rows(cfg)
    assert tuple(a.grid.dim) == dims
    members = cells_of(a, t)
    assert any(m.size == 0 for m in members) and sum(m.size for m in members) == n
    assert ref[0].max() > 0
    assert_exact_rows(out, ref)


# ---------------------------------------------------------------------------
# ghosts
# ---------------------------------------------------------------------------
def _ghost_system(dims, periodic, n_local, n_ghost, seed):
    """Locals in the box (none in the first cell); ghosts up to one r_list beyond the faces of the non-periodic axes,
    the first 40 of them beyond the -face of the first non-periodic axis next to the first cell, which then holds
    ghosts alone."""
    xyz, L = liquid(dims, RL3, n_local, seed, empty="first")
    rmax, w = RL3.max(), WIDTH * RL3.max()
    open_axes = [k for k in range(3) if not periodic[k]]
    g = _uniform(seed + 2, n_ghost, -0.5 * L, 0.5 * L)
    depth = syn.u01(seed + 3, np.arange(n_ghost, dtype=np.uint64), 0) * rmax
    for q in range(n_ghost):
        k = open_axes[q % len(open_axes)]
        g[q, k] = (0.5 * L[k] + depth[q]) * (1.0 if (q // len(open_axes)) % 2 else -1.0)
    k0 = open_axes[0]
    g[:40] = _uniform(seed + 4, 40, -0.5 * L, -0.5 * L + w)
    g[:40, k0] = -0.5 * L[k0] - depth[:40]
    xyz = np.concatenate([xyz, g])
    return dict(pos=syn.pos4(xyz, _types(seed, xyz.shape[0], 3)), L=L, periodic=periodic, rl=RL3, N=n_local)


@pytest.mark.parametrize("dims,periodic", [((3, 4, 4), (0, 1, 1)), ((4, 3, 2), (0, 0, 0)), ((4, 4, 4), (1, 0, 1))],
                         ids=lambda v: "".join(str(x) for x in v))
def test_rows_with_ghosts(dims, periodic):
    """N < n_total: locals list ghosts, ghosts get no row, d_n_neigh has N entries; a cell of ghosts alone."""
    n_local, n_ghost = 1103, 421
    cfg, ref = settled(lambda s: _ghost_system(dims, periodic, n_local, n_ghost, s), 23)
    out, a, t = build_rows(cfg)
    assert tuple(a.grid.dim) == dims
    members = cells_of(a, t)
    assert members[0].size >= 40 and np.all(members[0] >= n_local)  # a cell whose home particles are all ghosts
    listed_ghosts = sum(int(np.count_nonzero(r >= n_local)) for r in ref[1])
    assert listed_ghosts > 100
    assert out["n_count"].shape == (n_local,)
    assert_exact_rows(out, ref)


def test_no_locals_is_a_successful_no_op():
    """N = 0 with n_total > 0: success, nothing counted, nothing written."""
    cfg = _ghost_system((3, 4, 4), (0, 1, 1), 300, 100, 5)
    cfg["N"] = 0
    out, a, t = build_rows(cfg)
    assert out["rc_count"] == 0 and out["rc_fill"] == 0
    assert out["n_count"].size == 0 and np.all(out["n_guard"] == SENT) and np.all(out["nlist"] == SENT)
    single, _, _ = build_rows(cfg, row_capacity=16)
    assert single["rc_fill"] == 0 and np.all(single["n_guard"] == SENT) and np.all(single["nlist"] == SENT)
    assert np.all(single["max_neigh"] == 0)


# ---------------------------------------------------------------------------
# types
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(3, 3, 3), (4, 4, 4)], ids=lambda v: "".join(str(x) for x in v))  # MI = true / false
@pytest.mark.parametrize("table", ["pair_disabled", "type_disabled"])
def test_rows_per_type_pair(dims, table):
    rl = RL3 if table == "pair_disabled" else RL3_DEAD
    n = 1511

    def make(seed):
        xyz, L = liquid(dims, rl, n, seed)
        return dict(pos=syn.pos4(xyz, _types(seed, n, 3)), L=L, periodic=(1, 1, 1), rl=rl, N=n)

    cfg, ref = settled(make, 31)
    out, a, t = build_rows(cfg)
    assert_exact_rows(out, ref)
    typ = R.types_of(cfg["pos"])
    rows = gpu_rows(out, out["n_count"])
    if table == "type_disabled":
        assert np.count_nonzero(typ == 2) > 100 and np.all(out["n_count"][typ == 2] == 0)
        assert all(not np.any(typ[r] == 2) for r in rows)
    else:
        for i in np.flatnonzero(typ == 1):
            assert not np.any(typ[rows[i]] == 2)
        # the radii are distinct and each is used: some listed pair of every live type pair lies beyond the next
        # smaller radius
        xyz = cfg["pos"][:, :3]
        for ta, tb in ((0, 0), (0, 1), (1, 1), (0, 2), (2, 2)):
            far = 0
            for i in np.flatnonzero(typ == ta)[:200]:
                j = rows[i][typ[rows[i]] == tb]
                x, y, z = R.min_image(xyz[i] - xyz[j], cfg["L"], (0, 0, 0), (1, 1, 1))
                far += int(np.count_nonzero(x * x + y * y + z * z > (rl[ta, tb] - 0.1) ** 2))
            assert far > 0, (ta, tb)


# ---------------------------------------------------------------------------
# cutoff precision
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(3, 3, 3), (4, 4, 4)], ids=lambda v: "".join(str(x) for x in v))  # MI = true / false
def test_cutoff_is_tested_in_double_precision(dims):
    """Pairs planted along an axis at r = r_list (1 -+ 1e-7), per type pair, half of them across a periodic face:
    the inner ones are listed, the outer ones are not (a single-precision acceptance test cannot tell them apart:
    2e-7 in r^2 is three float ulps, below the rounding of r^2 itself)."""
    n_bg = 701
    live = [(ta, tb) for ta in range(3) for tb in range(ta, 3) if RL3[ta, tb] > 0]

    def make(seed):
        xyz, L = liquid(dims, RL3, n_bg, seed)
        typ = list(_types(seed, n_bg, 3))
        planted, extra = [], []
        spots = _uniform(seed + 7, 4 * len(live), -0.25 * L, 0.0)
        for q, (ta, tb) in enumerate(live):
            for v, (inside, across) in enumerate(((True, False), (False, False), (True, True), (False, True))):
                k = (q + v) % 3
                r = RL3[ta, tb] * ((1.0 - 1e-7) if inside else (1.0 + 1e-7))
                pi = spots[4 * q + v].copy()
                if across:
                    pi[k] = 0.5 * L[k] - 0.25 * RL3[ta, tb]
                pj = pi.copy()
                pj[k] += r
                if pj[k] >= 0.5 * L[k]:
                    pj[k] -= L[k]
                assert across == (pj[k] < pi[k])
                i = n_bg + len(extra)
                extra += [pi, pj]
                typ += [ta, tb]
                planted.append((i, i + 1, inside))
        xyz = np.concatenate([xyz, np.array(extra)])
        return dict(pos=syn.pos4(xyz, np.array(typ)), L=L, periodic=(1, 1, 1), rl=RL3, N=xyz.shape[0], planted=planted)

    cfg, ref = settled(make, 41)
    out, a, t = build_rows(cfg)
    rows = gpu_rows(out, out["n_count"])
    assert len(cfg["planted"]) == 4 * 5
    for i, j, inside in cfg["planted"]:
        assert (j in rows[i]) == inside and (i in rows[j]) == inside, (i, j, inside)
    assert_exact_rows(out, ref)


# ---------------------------------------------------------------------------
# exclusions
# ---------------------------------------------------------------------------
def star_system(dims, periodic, n_stars, n_free, seed, rl=RL3, near=0.9, L=None):
    """Stars of 17 beads (R.star_bonds: 9, 4, 5 and 1 bonded partners) and free particles (0). A bonded bead sits at a
    random offset of up to ``near`` * max r_list from the bead it hangs on (mostly in range, often in the same
    cell), every fifth one 1.6 to 2.2 r_list away (an excluded partner out of range); positions wrapped."""
    rmax = float(np.max(rl))
    L = np.asarray(dims) * WIDTH * rmax if L is None else np.asarray(L, dtype=np.float64)
    n = n_stars * R.STAR_SIZE + n_free
    xyz = _uniform(seed, n, -0.5 * L, 0.5 * L)
    bonds = R.star_bonds(n_stars)
    tag = np.arange(bonds.shape[0], dtype=np.uint64)
    u = np.stack([syn.normal(seed + 1, tag, c) for c in range(3)], axis=1)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    length = (0.15 + (near - 0.15) * syn.u01(seed + 2, tag, 0)) * rmax
    far = (np.arange(bonds.shape[0]) % 5) == 3
    length[far] = (1.6 + 0.6 * syn.u01(seed + 3, tag, 0)[far]) * rmax
    parent, child = bonds.min(axis=1), bonds.max(axis=1)
    for b in np.argsort(child, kind="stable"):
        xyz[child[b]] = xyz[parent[b]] + length[b] * u[b]
    xyz = syn.wrap(xyz, L)
    return dict(pos=syn.pos4(xyz, _types(seed, n, np.asarray(rl).shape[0])), L=L, periodic=periodic, rl=rl, N=n, bonds=bonds,
                exclusions=R.exclusions_from_bonds(n, bonds))


@pytest.mark.parametrize("dims", [(2, 3, 5), (4, 4, 4)], ids=lambda v: "".join(str(x) for x in v))  # MI = true / false
def test_rows_with_many_exclusions(dims):
    """0, 1, 4, 5 and 9 exclusions per particle; the table's pitch is wider than N."""
    cfg, ref = settled(lambda s: star_system(dims, (1, 1, 1), 64, 211, s), 51)
    n = cfg["N"]
    n_excl, excl = cfg["exclusions"]
    assert sorted(set(n_excl.tolist())) == [0, 1, 4, 5, 9]
    out, a, t = build_rows(cfg, excl_pitch=n + 37)
    assert a.excl_pitch == n + 37
    assert_exact_rows(out, ref)
    # what the exclusions had to remove: bonded partners in range (some in the same cell); and partners out of range
    typ = R.types_of(cfg["pos"])
    b = cfg["bonds"]
    x, y, z = R.min_image(cfg["pos"][b[:, 0], :3] - cfg["pos"][b[:, 1], :3], cfg["L"], (0, 0, 0), (1, 1, 1))
    in_range = (x * x + y * y + z * z) <= RL3[typ[b[:, 0]], typ[b[:, 1]]] ** 2
    cell_of = t["cell_of"].cpu().numpy()
    assert np.count_nonzero(in_range) > 100 and np.count_nonzero(~in_range) > 100
    assert np.count_nonzero(in_range & (cell_of[b[:, 0]] == cell_of[b[:, 1]])) > 20
    _, plain, _ = R.all_pairs_rows(cfg["pos"], cfg["L"], (0, 0, 0), (1, 1, 1), RL3, n)
    assert sum(r.size for r in plain) == ref[0].sum() + 2 * np.count_nonzero(in_range)


# ---------------------------------------------------------------------------
# dense cells: batches of NL_CAP = 1280 candidates (csrc/nlist.hip:329) x NL_HOME = 1024 home particles
# (csrc/nlist.hip:330), the last batch padded to a multiple of 128
# ---------------------------------------------------------------------------
def _two_cells(h0, h1, px, seed):
    """A 2 x 1 x 1 grid (x periodic or not) with exactly h0 / h1 particles in its cells, indices shuffled; one type
    (the kernel's single-radius shortcut), r_list = 0.7: rows of about 180."""
    L = np.array([4.0, 2.0, 2.0])
    lo = _uniform(seed, h0, (-1.99, -1.0, -1.0), (-0.01, 1.0, 1.0))
    hi = _uniform(seed + 1, h1, (0.01, -1.0, -1.0), (1.99, 1.0, 1.0))
    xyz = np.concatenate([lo, hi])
    xyz = xyz[np.argsort(syn.hash64(seed + 2, np.arange(h0 + h1, dtype=np.uint64), 1), kind="stable")]
    return dict(pos=syn.pos4(xyz, np.zeros(h0 + h1, dtype=np.int64)), L=L, periodic=(px, 0, 0), rl=np.array([[0.7]]), N=h0 + h1)


@pytest.mark.parametrize("px", [0, 1])  # x periodic on 2 cells: MI = true; else MI = false
@pytest.mark.parametrize("h0,h1", [(1024, 256), (1025, 256), (1024, 257), (1025, 255)])
def test_dense_cell_batch_boundaries(h0, h1, px):
    """Exactly 1024 / 1025 home particles in a cell with exactly 1280 / 1281 candidates around it."""
    cfg, ref = settled(lambda s: _two_cells(h0, h1, px, s), 61)
    out, a, t = build_rows(cfg, dims=(2, 1, 1))
    assert sorted(m.size for m in cells_of(a, t)) == sorted((h0, h1))
    assert_exact_rows(out, ref)


def test_dense_single_cell():
    """One non-periodic cell of 2701 particles: three chunks of home particles (1024 + 1024 + 653), three batches
    of candidates (1280 + 1280 + 141), neither count a multiple of 128. Two types with rows of a few hundred."""
    n = 2701
    rl = np.array([[0.9, 1.0], [1.0, 1.4]])

    def make(seed):
        typ = (np.arange(n) % 97 == 5).astype(np.int64)
        return dict(pos=syn.pos4(_uniform(seed, n, -1.5, 1.5), typ), L=np.array([3.0, 3.0, 3.0]), periodic=(0, 0, 0), rl=rl, N=n)

    cfg, ref = settled(make, 71)
    assert n > 2 * 1024 and n > 2 * 1280 and n % 128 and (n - 2048) % 128 and (n - 2560) % 128
    out, a, t = build_rows(cfg, dims=(1, 1, 1))
    assert tuple(a.grid.dim) == (1, 1, 1)
    assert 100 < ref[0].mean() < 500
    assert_exact_rows(out, ref)


# ---------------------------------------------------------------------------
# single-pass fill
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _single_pass_system():
    n = 1511

    def make(seed):
        xyz, L = liquid((4, 4, 4), RL3, n, seed)
        return dict(pos=syn.pos4(xyz, _types(seed, n, 3)), L=L, periodic=(1, 1, 1), rl=RL3, N=n)

    return settled(make, 81)


@pytest.mark.parametrize("cap_kind", ["max_neigh", "max_neigh-1", "8"])
def test_single_pass_fill(cap_kind):
    """row_capacity > 0, rows at i * cap, *d_max_neigh zeroed beforehand: full counts in d_n_neigh, at most cap
    entries stored per row, *d_max_neigh raised to the largest count when a row overflows (include/azp.h)."""
    cfg, ref = _single_pass_system()
    ref_n, ref_rows, borderline = ref
    assert borderline == 0
    n, most = cfg["N"], int(ref_n.max())
    cap = {"max_neigh": most, "max_neigh-1": most - 1, "8": 8}[cap_kind]
    assert most > 9
    exact, _, _ = build_rows(cfg)
    assert_exact_rows(exact, ref)
    out, a, t = build_rows(cfg, row_capacity=cap)
    assert out["rc_fill"] == 0
    assert np.array_equal(out["n_neigh"], ref_n) and np.all(out["n_guard"] == SENT)  # the full counts
    assert np.all(out["max_neigh"][1:] == 0)
    assert out["max_neigh"][0] == (0 if cap >= most else most)
    nl = out["nlist"]
    stored = np.minimum(ref_n, cap)
    written = np.zeros(nl.size, dtype=bool)
    for i in range(n):
        row = nl[i * cap: i * cap + stored[i]]
        written[i * cap: i * cap + stored[i]] = True
        if ref_n[i] <= cap:
            assert np.array_equal(np.sort(row), ref_rows[i]), i
            # count-then-fill and the single pass give the same row
            assert np.array_equal(np.sort(row), np.sort(exact["nlist"][exact["head"][i]: exact["head"][i] + ref_n[i]])), i
        else:
            assert np.unique(row).size == cap and np.all(np.isin(row, ref_rows[i])), i
    overflowing = np.count_nonzero(ref_n > cap)
    assert (overflowing == 0) if cap_kind == "max_neigh" else (overflowing > 0)
    assert np.all(nl[~written] == SENT) and np.all(nl[written] != SENT)


# ---------------------------------------------------------------------------
# tilted boxes are refused
# ---------------------------------------------------------------------------
def tilted_system(tilt, seed=91):
    """A fully periodic box of 4 x 4 x 4 cells with tilt factors ``tilt``, particles uniform in fractional
    coordinates, one type, r_list = 1.5."""
    L = np.array([6.6, 6.6, 6.6])
    xy, xz, yz = tilt
    lattice = np.array([[L[0], 0.0, 0.0], [xy * L[1], L[1], 0.0], [xz * L[2], yz * L[2], L[2]]])
    n = 1201
    xyz = _uniform(seed, n, -0.5, 0.5) @ lattice
    return dict(pos=syn.pos4(xyz, np.zeros(n, dtype=np.int64)), L=L, tilt=tilt, periodic=(1, 1, 1), rl=np.array([[1.5]]), N=n)


@pytest.mark.parametrize("tilt", [(0.5, 0.0, 0.0), (0.5, 0.3, -0.4)], ids=["xy", "xy_xz_yz"])
def test_tilted_box_is_refused(tilt):
    """Cartesian cells with a +-1 stencil cannot see a neighbor across a tilted periodic face (its image is shifted by
    xy Ly, no whole number of cells); before the refusal the builder silently dropped 4,224 of the 71,092 reference entries
    of this system (5.9 %) with xy = 0.5 and 7,840 of 71,142 (11.0 %) with all three tilts, and listed nothing wrong. azp_nlist_count / azp_nlist_fill return
    AZP_ERROR_INVALID_ARGUMENT before any launch, the outputs untouched."""
    cfg, ref = settled(lambda s: tilted_system(tilt, s), 91)
    assert ref[2] == 0 and ref[0].sum() > 10000
    out, a, t = build_rows(cfg)
    assert out["rc_count"] == INVALID_ARGUMENT and out["rc_fill"] is None
    assert np.all(out["n_count"] == SENT) and np.all(out["n_guard"] == SENT)
    single, _, _ = build_rows(cfg, row_capacity=int(ref[0].max()))
    assert single["rc_fill"] == INVALID_ARGUMENT
    assert np.all(single["n_neigh"] == SENT) and np.all(single["n_guard"] == SENT)
    assert np.all(single["nlist"] == SENT) and np.all(single["max_neigh"] == 0)
    # the same particles in the untilted box are built (and match the reference)
    cfg0, ref0 = settled(lambda s: dict(tilted_system(tilt, s), tilt=(0.0, 0.0, 0.0)), 91)
    assert_exact_rows(build_rows(cfg0)[0], ref0)


# ---------------------------------------------------------------------------
# through the API: nlist.Cell with fused = False
# ---------------------------------------------------------------------------
def test_api_rows_two_consumers_branched_polymers():
    """Non-cubic box of (2, 3, 5) cells (MI = true), two types, TWO consumers with different r_cut matrices (the list
    radius is their per-pair maximum plus the buffer), star polymers whose bond exclusions make State.exclusion_table
    9 wide. Rows after run(0), after a forced single-pass rebuild, after moves below and above half the buffer."""
    import torch

    import azplugins_amd as azp

    buffer = 0.3
    rc1 = np.array([[1.0, 0.8], [0.8, 1.2]])
    rc2 = np.array([[0.9, 1.1], [1.1, 0.7]])
    rl = np.maximum(rc1, rc2) + buffer
    assert rl.max() == 1.5
    L = np.array([2.1, 3.1, 5.1]) * rl.max()
    cfg, ref = settled(lambda s: star_system(None, (1, 1, 1), 60, 187, s, rl=rl, near=0.7, L=L), 101)
    n = cfg["N"]
    typeid = R.types_of(cfg["pos"])
    snap = azp.Snapshot.from_arrays(cfg["pos"][:, :3], L, typeid=typeid, types=("A", "B"), bonds=cfg["bonds"])
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(snap)
    nl = azp.nlist.Cell(buffer=buffer)
    nl.fused = False
    pots = []
    for rc in (rc1, rc2):
        pot = azp.pair.Hertz(nlist=nl, default_r_cut=1.0)
        for (ta, tb), name in (((0, 0), ("A", "A")), ((0, 1), ("A", "B")), ((1, 1), ("B", "B"))):
            pot.r_cut[name] = float(rc[ta, tb])
            pot.params[name] = dict(epsilon=1.0)
        pots.append(pot)
    sim.operations.integrator = azp.Integrator(dt=0.001, forces=pots)
    sim.run(0)
    assert sim.state.exclusion_table()[1].shape[0] == 9
    assert tuple(nl._cells.grid.dim) == (2, 3, 5)

    def assert_rows(ref):
        nn = nl.n_neigh.cpu().numpy().astype(np.int64)
        hd = nl.head_list.cpu().numpy().astype(np.int64)
        li = nl.nlist.cpu().numpy().astype(np.int64)
        assert ref[2] == 0 and np.array_equal(nn, ref[0])
        for i in range(n):
            assert np.array_equal(np.sort(li[hd[i]: hd[i] + nn[i]]), ref[1][i]), i

    assert nl.num_builds == 1 and int(nl.head_list[1].item()) == ref[0][0]  # exact rows
    assert_rows(ref)
    nl.compute(sim.state, force=True)  # the fill alone, rows of the learned capacity
    cap = nl._row_capacity
    assert nl.num_builds == 2 and nl.size == n * cap and int(nl.head_list[1].item()) == cap
    assert_rows(ref)

    def displacement(amplitude, seed):
        tag = np.arange(n, dtype=np.uint64)
        v = np.stack([syn.normal(seed, tag, c) for c in range(3)], axis=1)
        return v * (amplitude * (0.5 + 0.5 * syn.u01(seed + 1, tag, 0)) / np.linalg.norm(v, axis=1))[:, None]

    def move(amplitude, seed):
        v = displacement(amplitude, seed)
        sim.state.pos[:, :3] += torch.from_numpy(v).to(sim.state.pos.device)
        sim.state.position_generation += 1
        nl.compute(sim.state)
        return np.linalg.norm(v, axis=1)

    d = move(0.45 * buffer, 7)
    assert d.min() > 0 and d.max() < 0.5 * buffer
    assert nl.num_builds == 2  # nobody moved farther than half the buffer: the rows stand
    assert_rows(ref)
    for seed in range(8, 18):  # (reseeded until the moved configuration has no borderline pair)
        pos = sim.state.pos.cpu().numpy()
        pos[:, :3] += displacement(0.9 * buffer, seed)
        ref2 = R.all_pairs_rows(pos, L, (0, 0, 0), (1, 1, 1), rl, n, cfg["exclusions"])
        if ref2[2] == 0:
            break
    d2 = move(0.9 * buffer, seed)
    assert np.array_equal(sim.state.pos.cpu().numpy(), pos)
    assert d2.min() > 0.4 * buffer
    assert np.linalg.norm(pos[:, :3] - cfg["pos"][:, :3], axis=1).max() > 0.5 * buffer
    assert nl.num_builds >= 3  # a rebuild was observed
    assert_rows(ref2)
