"""Tile plans of a chosen size, in numpy: the staged-set size of every tile as the plan compiler defines it
(pair_plan.hip), and a builder of configurations whose largest staged set is exactly K particles."""

import functools

import numpy as np

from azplugins_amd import synthetic as syn

# the liquid of staged_set_config: 64 x 12 x 12 simple-cubic sites, spacing 1, x fastest
NX, NY, NZ = 64, 12, 12
LIQUID = NX * NY * NZ
JITTER = 0.08


def cap_for(max_stage):
    """LDS slots of the tile kernel for a largest staged set (pair_plan.hpp: plan_cap_for; slot 0 is the dummy)."""
    need = max_stage + 1
    for cap in (1024, 1536, 1664, 2048):
        if need <= cap:
            return cap
    return 2560


def row_entries(nl, N):
    """(owner row, listed particle) of every entry of the first N rows of a HOOMD-format list."""
    n_neigh, head, nlist = nl
    n = np.asarray(n_neigh[:N], dtype=np.int64)
    h = np.asarray(head[:N], dtype=np.int64)
    owner = np.repeat(np.arange(N, dtype=np.int64), n)
    offs = np.arange(int(n.sum()), dtype=np.int64) - np.repeat(np.cumsum(n) - n, n)
    return owner, np.asarray(nlist, dtype=np.int64)[np.repeat(h, n) + offs]


def stage_sizes(nl, N, n_total, tb):
    """Staged-set size of every tile of tb consecutive particles: the number of distinct particles that the rows of the
    tile's members list (pair_plan.hip: the hash set of a tile's list entries)."""
    owner, j = row_entries(nl, N)
    n_tiles = (N + tb - 1) // tb
    key = np.unique((owner // tb) * n_total + j)
    return np.bincount(key // n_total, minlength=n_tiles)


def _liquid():
    k = np.arange(LIQUID)
    xyz = np.stack([k % NX, (k // NX) % NY, k // (NX * NY)], axis=1).astype(np.float64)
    tag = np.arange(LIQUID, dtype=np.uint64)
    return xyz + np.stack([(2.0 * syn.u01(41, tag, c) - 1.0) * JITTER for c in range(3)], axis=1)


def _centre_stage(xyz, tb, r):
    """Staged set of the tile at the centre of the liquid (periodic along x only), by brute force."""
    m = tb // NX
    t = (6 * NY + (6 - m // 2) // m * m) // m
    mem = xyz[t * tb:(t + 1) * tb]
    d = xyz[:, None, :] - mem[None, :, :]
    d[..., 0] -= NX * np.rint(d[..., 0] / NX)
    r2 = (d * d).sum(axis=2)
    r2[np.arange(t * tb, (t + 1) * tb), np.arange(tb)] = np.inf  # (a particle does not list itself)
    return int((r2 < r * r).any(axis=1).sum())


def _sites(n, z0, Lx, Ly, s):
    """n sites in layers from z0 up, at least s apart (across the periodic x and y faces too); and the top layer's z."""
    nx, ny = max(int(Lx // s), 1), max(int(Ly // s), 1)
    k = np.arange(n)
    layer, rem = k // (nx * ny), k % (nx * ny)
    xyz = np.stack([(rem % nx + 0.5) * (Lx / nx), (rem // nx + 0.5) * (Ly / ny), z0 + layer * s], axis=1)
    return xyz, z0 + (int(layer.max()) if n else 0) * s


@functools.lru_cache(maxsize=None)
def staged_set_config(K, tb, pad=0):
    """Positions (n x 4, one type) and box whose tile plan of tb-particle tiles (tb = 64, 128, 256) stages exactly K
    particles in its fullest tile, with the oracle's list of radius r_list: an ordinary list (every entry within
    r_list, symmetric).

    A 64 x 12 x 12 simple-cubic liquid in x-fastest order (a tile = tb / 64 whole x-lines), periodic along x only,
    with the smallest list radius (to 1e-3) at which its centre tile stages more than K particles. Over-full tiles are
    then shrunk: a listed particle that is not a member of the fullest tile moves to an isolated site in a vacuum slab
    above the liquid, which takes exactly that particle out of the tile's set and adds to no set. The fullest tile is
    shrunk to K at a time until no tile holds more; the last one shrunk holds K. ``pad`` isolated particles follow the
    liquid (tiles with nothing to stage). Returns dict(pos, L, r_list, N, stage, nl, moved)."""
    import oracle

    assert tb in (64, 128, 256) and K > 0
    xyz = _liquid()
    lo, hi = 0.9, 5.0
    while hi - lo > 1e-3:
        mid = 0.5 * (lo + hi)
        lo, hi = (lo, mid) if _centre_stage(xyz, tb, mid) >= K + 2 else (mid, hi)
    r = hi
    s = r + 0.5                       # spacing of the isolated sites
    Ly = NY + r + 1.0                 # the liquid does not see its own y image
    nl = oracle.build_nlist(oracle.pos4(xyz), oracle.make_box((NX, Ly, NZ + 2 * r + 2.0)), r)
    owner, j = row_entries(nl, LIQUID)
    n_tiles = LIQUID // tb
    key = np.unique((owner // tb) * LIQUID + j)
    kt, kj = key // LIQUID, key % LIQUID
    bounds = np.searchsorted(kt, np.arange(n_tiles + 1))
    sets = [set(kj[bounds[t]:bounds[t + 1]].tolist()) for t in range(n_tiles)]
    by_j = np.argsort(kj, kind="stable")
    jb = np.searchsorted(kj[by_j], np.arange(LIQUID + 1))
    rows = np.searchsorted(owner, np.arange(0, LIQUID + 1, tb))
    moved = np.zeros(LIQUID, dtype=bool)
    dirty = set()
    while True:
        for t in dirty:  # a moved particle's row is empty now: its own tile's set is recounted
            own, lst = owner[rows[t]:rows[t + 1]], j[rows[t]:rows[t + 1]]
            sets[t] = set(lst[~moved[own] & ~moved[lst]].tolist())
        dirty.clear()
        sizes = np.array([len(x) for x in sets])
        t = int(np.argmax(sizes))
        if sizes[t] <= K:
            break
        cand = np.array(sorted(x for x in sets[t] if x // tb != t), dtype=np.int64)
        cand = cand[np.argsort(syn.hash64(7, cand.astype(np.uint64), 3), kind="stable")]
        pick = cand[: sizes[t] - K]
        assert pick.size == sizes[t] - K
        for p in pick.tolist():
            moved[p] = True
            for u in kt[by_j[jb[p]:jb[p + 1]]].tolist():
                sets[u].discard(p)
            dirty.add(p // tb)
        assert len(sets[t]) == K
    n_moved = int(moved.sum())
    sites, z_top = _sites(n_moved + pad, NZ - 1 + JITTER + s, NX, Ly, s)
    out = np.concatenate([xyz, sites[n_moved:]])
    out[np.flatnonzero(moved)] = sites[:n_moved]
    L = np.array([NX, Ly, z_top + s + 0.2])
    pos = oracle.pos4(syn.wrap(out - 0.5 * L, L))
    n = pos.shape[0]
    nl = oracle.build_nlist(pos, oracle.make_box(L), r)
    stage = stage_sizes(nl, n, n, tb)
    assert stage.max() == K and np.array_equal(stage[:n_tiles], sizes), "staged-set builder"
    return dict(pos=pos, L=L, r_list=r, N=n, stage=stage, nl=nl, moved=n_moved)
