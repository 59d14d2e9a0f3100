"""Generated systems for the binning tests (test_gpu_binning.py on the GPU, test_binning_ref.py without one).

* ``occupancy_case``: particles placed cell by cell from a per-cell count chosen beforehand, so that the occupancies
  that select a path of azp_nlist_bin's per-cell sort (csrc/nlist.hip) are there by construction, and so are occupied
  cells at the first and last cell of the grid and on both sides of every 4,096-cell block of its scan.
* ``clumped``: a fully periodic box of many cells with few particles: clumps of 16 around cell corners (each one
  straddles up to 8 cells), so that rows are long although most cells are empty.

Only numpy here: the cell rule below is the reference, not the library's.
"""

import functools

import numpy as np

import nlist_ref as R
from azplugins_amd import synthetic as syn

SCAN_BLOCK = 4096  # cells per trip / per workgroup of the scan kernels
SMALL_SET = (0, 1, 7, 8, 9, 70)                  # thread-per-cell sort: registers up to 8, memory above
WAVE_SET = (0, 1, 63, 64, 65, 128, 129, 500)     # wave-per-cell sort: trips of 64
CELL_WIDTH = np.array([1.1, 0.9, 1.3])           # (three different widths: a swapped axis lands in another cell)

# (dims, n_total) of the table in the issue; the expected path follows from the rule in azp_nlist_bin (paths_of)
TABLE = [
    ((16, 16, 16), 24576),
    ((16, 16, 16), 24577),
    ((17, 241, 1), 3001),
    ((32, 32, 32), 20011),
    ((9, 11, 331), 20011),
    ((5, 73, 101), 230003),
    ((32, 32, 40), 20011),
    ((41, 41, 41), 17),
    ((41, 41, 41), 18),
    ((64, 64, 64), 200003),
    ((17, 241, 1), 30011),
]


def paths_of(dims, n):
    """(scan path, sort kernel) azp_nlist_bin selects: the three-kernel scan when the grid has more than 8 blocks of
    4,096 cells and the block totals + the grand total fit into d_order_tmp (n words); the thread-per-cell sort up to
    6 particles per cell on average."""
    ncell = int(np.prod(dims))
    nblk = (ncell + SCAN_BLOCK - 1) // SCAN_BLOCK
    scan = "scan3x%d" % nblk if (nblk > 8 and nblk + 1 <= n) else "scan1x%d" % nblk
    return scan, ("small" if n <= 6 * ncell else "wave")


def case_id(case):
    dims, n = case
    return "%dx%dx%d-n%d-%s-%s" % (tuple(dims) + (n,) + paths_of(dims, n))


def cell_rule(xyz, lo, width, dims, periodic):
    """Cell id of every position: floor((x - lo) / width) per axis, wrapped on a periodic axis, clamped on another;
    x fastest."""
    dims = np.asarray(dims, dtype=np.int64)
    c = np.floor((np.asarray(xyz, dtype=np.float64) - lo) / width).astype(np.int64)
    for k in range(3):
        c[:, k] = np.mod(c[:, k], dims[k]) if periodic[k] else np.clip(c[:, k], 0, dims[k] - 1)
    return (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]


def marked_cells(ncell):
    """The first and the last cell, and the cells on both sides of every block boundary of the scan."""
    m = [0, ncell - 1]
    for b in range(SCAN_BLOCK, ncell, SCAN_BLOCK):
        m += [b - 1, b]
    return np.unique(np.array(m, dtype=np.int64))


def _counts(dims, n, seed):
    """Per-cell counts that sum to n: the occupancy set of the sort kernel the case selects, the marked cells
    occupied, some cells left empty, the rest spread over hashed cells."""
    ncell = int(np.prod(dims))
    wanted = SMALL_SET if paths_of(dims, n)[1] == "small" else WAVE_SET
    counts = np.zeros(ncell, dtype=np.int64)
    marks = marked_cells(ncell)
    hashed = np.argsort(syn.hash64(seed, np.arange(ncell, dtype=np.uint64), 3), kind="stable")
    free = hashed[~np.isin(hashed, marks)]
    if n < sum(wanted) + 4 * marks.size:
        # too few particles for the set (41^3 with 17 / 18: these cases are about the switch between the scans): one
        # per marked cell as far as they go, the first and the last cell first, the remainder into the first cell
        first = np.concatenate([[0, ncell - 1], marks[1:-1]])[:n]
        counts[first] = 1
        counts[0] += n - first.size
        return counts
    edge = [v for v in wanted if 0 < v < 70]
    counts[marks] = np.array(edge)[np.arange(marks.size) % len(edge)]  # (edge occupancies ON the block boundaries)
    big = [v for v in wanted if v > 0]
    counts[free[: len(big)]] = big
    empty, free = free[len(big): len(big) + 8], free[len(big) + 8:]
    rest = n - int(counts.sum())
    assert rest >= 0 and free.size > 0
    base = rest // free.size
    u = syn.hash64(seed + 1, free.astype(np.uint64), 4)
    if base == 0:
        g = 1 + (u % np.uint64(6)).astype(np.int64)     # 1 .. 6 per occupied cell, most cells empty
        g[np.cumsum(g) - g >= rest] = 0
    else:
        spread = min(base, 3)
        g = base - spread + (u % np.uint64(2 * spread + 1)).astype(np.int64)
    while True:  # settle the remainder one particle per cell
        r = rest - int(g.sum())
        if r == 0:
            break
        pick = np.flatnonzero(g > 0)[: abs(r)]
        g[pick] += 1 if r > 0 else -1
    counts[free] = g
    assert np.all(counts[empty] == 0) and counts.sum() == n
    return counts


@functools.lru_cache(maxsize=None)
def occupancy_case(dims, n, seed=7):
    """dict(xyz [n, 3] in cell-major order, cell [n], counts [ncell], L, lo, width): counts[c] particles at the
    centre of cell c plus a jitter below 0.4 of the width per axis (no particle within 0.1 width of a face: the cell
    of each is beyond doubt). Do not modify the arrays."""
    dims_a = np.asarray(dims, dtype=np.int64)
    counts = _counts(dims, n, seed)
    cell = np.repeat(np.arange(counts.size, dtype=np.int64), counts)
    ijk = np.stack([cell % dims_a[0], (cell // dims_a[0]) % dims_a[1], cell // (dims_a[0] * dims_a[1])], axis=1)
    tag = np.arange(n, dtype=np.uint64)
    jitter = np.stack([0.8 * (syn.u01(seed + 2, tag, c) - 0.5) for c in range(3)], axis=1)
    assert np.all(np.abs(jitter) < 0.4)
    L = dims_a * CELL_WIDTH
    lo = -0.5 * L
    xyz = lo + (ijk + 0.5 + jitter) * CELL_WIDTH
    return dict(xyz=xyz, cell=cell, counts=counts, L=L, lo=lo, width=CELL_WIDTH.copy(), dims=tuple(dims))


def shuffled(n, seed=19):
    """A seeded permutation of n indices."""
    return np.argsort(syn.hash64(seed, np.arange(n, dtype=np.uint64), 5), kind="stable")


# ---------------------------------------------------------------------------
# clumped systems on grids of many cells
# ---------------------------------------------------------------------------
WIDTH = 1.07  # cell width in units of the list radius (test_gpu_nlist_rows.WIDTH)
CLUMP = 16


def clumped(dims, r_list, seed, n_clumps=280, n_free=240, width=WIDTH):
    """(xyz [n, 3], L): n_clumps clumps of 16 particles, each uniform in a cube of edge 0.9 r_list centred on a cell
    CORNER (the clump straddles up to 8 cells), eight of them on faces, edges and the corner of the periodic box; n_free
    particles uniform in the box; wrapped, indices shuffled."""
    dims = np.asarray(dims, dtype=np.int64)
    w = width * float(r_list)
    L = dims * w
    q = np.arange(n_clumps, dtype=np.uint64)
    corner = np.stack([(syn.hash64(seed, q, c) % np.uint64(dims[c])).astype(np.int64) for c in range(3)], axis=1)
    a, b = dims // 3, (2 * dims) // 3
    corner[:8] = [(0, a[1], b[2]), (a[0], 0, b[2]), (a[0], b[1], 0), (0, b[1], a[2]),   # faces
                  (0, 0, a[2]), (0, a[1], 0), (b[0], 0, 0),                             # edges
                  (0, 0, 0)]                                                            # the corner
    tag = np.arange(n_clumps * CLUMP, dtype=np.uint64)
    off = np.stack([0.9 * float(r_list) * (syn.u01(seed + 1, tag, c) - 0.5) for c in range(3)], axis=1)
    members = -0.5 * L + np.repeat(corner, CLUMP, axis=0) * w + off
    ftag = np.arange(n_free, dtype=np.uint64)
    free = np.stack([(syn.u01(seed + 2, ftag, c) - 0.5) * L[c] for c in range(3)], axis=1)
    xyz = syn.wrap(np.concatenate([members, free]), L)
    return xyz[shuffled(xyz.shape[0], seed + 3)], L


def settled(make, seed):
    """make(seed) -> dict(pos, L, periodic, rl, N) and its all-pairs reference, for the first seed (seed, seed + 100,
    ...) whose configuration has no borderline pair (as test_gpu_nlist_rows.settled)."""
    for s in range(seed, seed + 1000, 100):
        cfg = make(s)
        ref = R.all_pairs_rows(cfg["pos"], cfg["L"], (0, 0, 0), cfg["periodic"], cfg["rl"], cfg["N"])
        if ref[2] == 0:
            return cfg, ref
    raise AssertionError("no configuration without a borderline pair in 10 seeds")


def _types(seed, n, ntypes):
    return (syn.hash64(seed + 500, np.arange(n, dtype=np.uint64), 9) % np.uint64(ntypes)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def clumped_system(dims, rl_key, seed=3, width=WIDTH):
    """(cfg, all-pairs reference) of the clumped system on ``dims`` cells with the list radii ``rl_key`` (a tuple of
    tuples) and cells ``width`` list radii wide, computed once per session. Do not modify."""
    rl = np.array(rl_key, dtype=np.float64)

    def make(s):
        xyz, L = clumped(dims, rl.max(), s, width=width)
        n = xyz.shape[0]
        return dict(pos=syn.pos4(xyz, _types(s, n, rl.shape[0])), L=L, periodic=(1, 1, 1), rl=rl, N=n)

    return settled(make, seed)


def clumped_facts(cfg, ref, dims):
    """What the reference must show for the system to test anything: dict(mean_row, crossing = listed pairs across
    the periodic face of each axis, top_cell = largest occupied cell id, occupied_above = {2^15: n, 2^16: n})."""
    n_neigh, rows, borderline = ref
    xyz, L = cfg["pos"][:, :3], np.asarray(cfg["L"])
    i = np.repeat(np.arange(n_neigh.size), n_neigh)
    j = np.concatenate(rows)
    d = np.abs(xyz[i] - xyz[j])
    cell = cell_rule(xyz, -0.5 * L, L / np.asarray(dims), dims, (1, 1, 1))
    occupied = np.unique(cell)
    return dict(borderline=borderline, mean_row=float(n_neigh.mean()),
                crossing=[int(np.count_nonzero(d[:, k] > 0.5 * L[k])) // 2 for k in range(3)],
                top_cell=int(occupied.max()), max_occupancy=int(np.bincount(cell).max()),
                occupied_above={b: int(np.count_nonzero(occupied >= b)) for b in (32768, 65536)})
