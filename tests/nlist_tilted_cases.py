"""Tilted and partly periodic boxes for the cell-list tests (tests/test_nlist_tilted.py on the CPU,
tests/test_gpu_nlist_tilted.py on the GPU), and a NumPy restatement of the fractional-cell scheme of csrc/nlist.hip:
bin by the fractional coordinates along the lattice vectors, search the +-1 stencil, take the minimum image per
pair or fix the image of every staged particle once, relative to the home cell's centre.

The reference of both test files is tests/nlist_ref.all_pairs_rows, which knows no grid."""

import numpy as np

import nlist_ref as R
from azplugins_amd import synthetic as syn

TILT3 = (0.5, 0.3, -0.4)
R_LIST = 1.5

# (L, tilt, cells the product must choose at r_list = 1.5)
GRID_CASES = [
    ((6.6, 6.6, 6.6), TILT3, (3, 4, 4)),
    ((9.0, 8.0, 7.5), TILT3, (4, 4, 5)),
    ((4.0, 7.0, 3.2), TILT3, (2, 4, 2)),
]


def lattice(L, tilt):
    """Rows a, b, c: the lattice vectors of HOOMD's BoxDim."""
    xy, xz, yz = tilt
    return np.array([[L[0], 0.0, 0.0], [xy * L[1], L[1], 0.0], [xz * L[2], yz * L[2], L[2]]])


def fractional(xyz, L, tilt):
    """f on [-0.5, 0.5) for a wrapped particle: f_z = z / Lz, f_y = (y - yz z) / Ly, f_x = (x - xy y - (xz - xy yz) z) / Lx."""
    xy, xz, yz = tilt
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    return np.stack([(x - xy * y - (xz - xy * yz) * z) / L[0], (y - yz * z) / L[1], z / L[2]], axis=1)


def uniform(seed, n, lo, hi):
    tag = np.arange(n, dtype=np.uint64)
    lo, hi = np.broadcast_to(lo, (3,)), np.broadcast_to(hi, (3,))
    return np.stack([lo[c] + syn.u01(seed, tag, c) * (hi[c] - lo[c]) for c in range(3)], axis=1)


def types(seed, n, ntypes):
    return (syn.hash64(seed + 500, np.arange(n, dtype=np.uint64), 9) % np.uint64(ntypes)).astype(np.int64)


def tilted_liquid(L, tilt, periodic, n, seed, rl=R_LIST, ntypes=1, n_extra=0):
    """n particles uniform in fractional coordinates (a liquid's lack of order) and, behind them, ``n_extra``
    ghost-like particles up to one r_list beyond the faces of the open axes (n_total = n + n_extra > N = n)."""
    L = np.asarray(L, dtype=np.float64)
    f = uniform(seed, n, -0.5, 0.5)
    if n_extra:
        open_axes = [k for k in range(3) if not periodic[k]]
        g = uniform(seed + 2, n_extra, -0.5, 0.5)
        depth = syn.u01(seed + 3, np.arange(n_extra, dtype=np.uint64), 0) * float(np.max(rl))
        for q in range(n_extra):
            k = open_axes[q % len(open_axes)]
            g[q, k] = (0.5 + depth[q] / L[k]) * (1.0 if (q // len(open_axes)) % 2 else -1.0)
        f = np.concatenate([f, g])
    xyz = f @ lattice(L, tilt)
    rl = np.asarray(rl, dtype=np.float64)
    rl = rl.reshape(1, 1) if rl.ndim == 0 else rl
    return dict(pos=syn.pos4(xyz, types(seed, xyz.shape[0], ntypes)), L=L, tilt=tuple(tilt), periodic=tuple(periodic), rl=rl, N=n)


def wrap_tilted(xyz, L, tilt, periodic=(1, 1, 1)):
    """The image of every position inside the box: fractional coordinates of the periodic axes on [-0.5, 0.5)."""
    f = fractional(np.asarray(xyz, dtype=np.float64), L, tilt)
    for k in range(3):
        if periodic[k]:
            f[:, k] -= np.floor(f[:, k] + 0.5)
    return f @ lattice(L, tilt)


def tilted_stars(L, tilt, n_stars, n_free, seed, rl, near=0.9):
    """Stars of 17 beads (nlist_ref.star_bonds: 9, 4, 5 and 1 bonded partners) and free particles in a fully periodic
    tilted box, types at random. A bonded bead sits up to ``near`` * max r_list from the bead it hangs on, every fifth
    one 1.6 to 2.2 r_list away (an excluded partner out of range); positions wrapped into the box."""
    L = np.asarray(L, dtype=np.float64)
    rl = np.asarray(rl, dtype=np.float64)
    rmax = float(rl.max())
    n = n_stars * R.STAR_SIZE + n_free
    xyz = uniform(seed, n, -0.5, 0.5) @ lattice(L, tilt)
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
    xyz = wrap_tilted(xyz, L, tilt)
    return dict(pos=syn.pos4(xyz, types(seed, n, rl.shape[0])), L=L, tilt=tuple(tilt), periodic=(1, 1, 1), rl=rl, N=n, bonds=bonds,
                exclusions=R.exclusions_from_bonds(n, bonds))


def settled(make, seed):
    """make(seed) -> configuration and its all-pairs reference, for the first seed (seed, seed + 100, ...) whose
    configuration has no borderline pair (the discipline of tests/test_gpu_nlist_rows.py)."""
    for s in range(seed, seed + 1000, 100):
        cfg = make(s)
        ref = R.all_pairs_rows(cfg["pos"], cfg["L"], cfg.get("tilt", (0, 0, 0)), cfg["periodic"], cfg["rl"], cfg["N"],
                               cfg.get("exclusions"))
        if ref[2] == 0:
            return cfg, ref
    raise AssertionError("no configuration without a borderline pair in 10 seeds")


def _stencil_axis(c, d, periodic):
    """Cells of one axis that the search around cell c visits (nlist_cell_kernel's index arithmetic)."""
    if periodic:
        return list(range(d)) if d < 3 else [(c + o + d) % d for o in (-1, 0, 1)]
    return [c + o for o in (-1, 0, 1) if 0 <= c + o < d]


def fractional_cell_rows(cfg, dims, rule):
    """Rows of ``cfg`` by the scheme under test. ``rule``: "pair" -- minimum image of every candidate pair;
    "staged" -- every particle of the stencil, and the home particle, replaced once by the image whose fractional
    coordinates lie nearest to the home cell's centre, n_k = rint(f_k - fc_k), then plain differences."""
    pos, L, tilt, periodic, rl, N = (cfg[k] for k in ("pos", "L", "tilt", "periodic", "rl", "N"))
    xyz = pos[:, :3]
    typ = R.types_of(pos)
    h = lattice(L, tilt)
    f = fractional(xyz, L, tilt)
    dims = np.asarray(dims)
    cell = np.floor((f + 0.5) * dims).astype(np.int64)
    for k in range(3):
        cell[:, k] = cell[:, k] % dims[k] if periodic[k] else np.clip(cell[:, k], 0, dims[k] - 1)
    members = {}
    for i, c in enumerate(map(tuple, cell)):
        members.setdefault(c, []).append(i)
    per = np.array([1.0 if p else 0.0 for p in periodic])
    rows = [None] * N
    for c, home in members.items():
        cand = [j for cx in _stencil_axis(c[0], dims[0], periodic[0]) for cy in _stencil_axis(c[1], dims[1], periodic[1])
                for cz in _stencil_axis(c[2], dims[2], periodic[2]) for j in members.get((cx, cy, cz), ())]
        cand = np.array(cand, dtype=np.int64)
        assert np.unique(cand).size == cand.size  # every cell once
        home = np.array([i for i in home if i < N], dtype=np.int64)
        if home.size == 0:
            continue
        if rule == "staged":
            fc = (np.array(c) + 0.5) / dims - 0.5
            xj = xyz[cand] - (np.rint(f[cand] - fc) * per) @ h
            xi = xyz[home] - (np.rint(f[home] - fc) * per) @ h
            d = xi[:, None, :] - xj[None, :, :]
            x, y, z = d[..., 0], d[..., 1], d[..., 2]
        else:
            x, y, z = R.min_image(xyz[home][:, None, :] - xyz[cand][None, :, :], L, tilt, periodic)
        r = rl[typ[home][:, None], typ[cand][None, :]]
        acc = (r > 0.0) & (x * x + y * y + z * z <= r * r) & (home[:, None] != cand[None, :])
        for q, i in enumerate(home):
            rows[i] = np.sort(cand[acc[q]])
    return rows
