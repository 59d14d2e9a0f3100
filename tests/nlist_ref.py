"""All-pairs neighbor rows in numpy (FP64, no cells): the reference the cell-list row builder
(csrc/nlist.hip) is pinned against. Nothing here knows about a grid or a stencil, so a mistake in
those cannot be shared with the code under test (oracle.build_nlist is itself a 27-cell search).
Also the star-polymer topology the exclusion and bond-table tests use."""

import numpy as np

BORDERLINE_REL = 1e-9  # pairs with |r^2 - r_list^2| <= this * r_list^2 are "borderline" (must not exist)


def types_of(pos4):
    """Type ids from the low 32 bits of pos.w (HOOMD's __scalar_as_int)."""
    w = np.ascontiguousarray(np.asarray(pos4, dtype=np.float64)[:, 3])
    return (w.view(np.int64) & 0xFFFFFFFF).astype(np.int64)


def min_image(d, L, tilt, periodic):
    """HOOMD's BoxDim::minImage on an array of separations d[..., 3]: z first, then y, then x,
    every shift along a tilted lattice vector."""
    x, y, z = d[..., 0].copy(), d[..., 1].copy(), d[..., 2].copy()
    xy, xz, yz = (float(t) for t in tilt)
    if periodic[2]:
        img = np.rint(z / L[2])
        z -= L[2] * img
        y -= L[2] * yz * img
        x -= L[2] * xz * img
    if periodic[1]:
        img = np.rint(y / L[1])
        y -= L[1] * img
        x -= L[1] * xy * img
    if periodic[0]:
        x -= L[0] * np.rint(x / L[0])
    return x, y, z


def all_pairs_rows(pos4, L, tilt, periodic, r_list, N, exclusions=None, chunk=256):
    """Rows of the full neighbor list of particles [0, N) over all n_total particles of ``pos4``.

    rows[i]: sorted j in [0, n_total) with j != i, r_list[ti, tj] > 0, minimum-image r^2 <= r_list^2,
    j not among i's exclusions. ``exclusions``: (n_excl[N], excl[N, width]).
    Returns (n_neigh int64[N], rows, borderline); borderline counts the pairs (excluded or not) whose
    r^2 is within BORDERLINE_REL of the cutoff: with none of those, any correct FP64 builder lists
    exactly these sets."""
    pos4 = np.asarray(pos4, dtype=np.float64)
    n_total = pos4.shape[0]
    L = np.broadcast_to(np.asarray(L, dtype=np.float64), (3,))
    typ = types_of(pos4)
    rl = np.asarray(r_list, dtype=np.float64)
    if rl.ndim == 0:
        rl = np.full((int(typ.max()) + 1 if n_total else 1,) * 2, float(rl))
    xyz = pos4[:, :3]
    rows = []
    borderline = 0
    cols = np.arange(n_total)
    for i0 in range(0, N, chunk):
        i1 = min(i0 + chunk, N)
        x, y, z = min_image(xyz[i0:i1, None, :] - xyz[None, :, :], L, tilt, periodic)
        rsq = x * x + y * y + z * z
        r = rl[typ[i0:i1, None], typ[None, :]]
        rlsq = r * r
        live = (r > 0.0) & (cols[None, :] != np.arange(i0, i1)[:, None])
        borderline += int(np.count_nonzero(live & (np.abs(rsq - rlsq) <= BORDERLINE_REL * rlsq)))
        acc = live & (rsq <= rlsq)
        if exclusions is not None:
            n_excl, excl = exclusions
            n_excl = np.asarray(n_excl, dtype=np.int64)[i0:i1]
            excl = np.asarray(excl, dtype=np.int64)[i0:i1]
            local = np.arange(i1 - i0)
            for e in range(excl.shape[1]):
                has = n_excl > e
                acc[local[has], excl[has, e]] = False
        rows.extend(np.flatnonzero(a) for a in acc)
    n_neigh = np.array([r.size for r in rows], dtype=np.int64).reshape(N)
    return n_neigh, rows, borderline


# ---------------------------------------------------------------------------
# branched topology: per-particle bond counts {0, 1, 4, 5, 9}
# ---------------------------------------------------------------------------
STAR_SIZE = 17


def star_bonds(n_stars, first=0):
    """Bonds of ``n_stars`` 17-bead stars laid out from particle ``first``: a hub with 9 arms (9 bonds), arm 0 with 3
    more beads on it (4 bonds), arm 1 with 4 more (5 bonds), every other bead a leaf (1 bond). Members of a bond in
    alternating order, so that both positions in a bond occur on every kind of bead."""
    bonds = []
    for s in range(n_stars):
        h = first + s * STAR_SIZE
        for arm in range(9):
            bonds.append((h, h + 1 + arm))
        for c in range(3):
            bonds.append((h + 1, h + 10 + c))
        for c in range(4):
            bonds.append((h + 2, h + 13 + c))
    bonds = np.array(bonds, dtype=np.int64).reshape(-1, 2)
    flip = (np.arange(bonds.shape[0]) % 3) == 1
    bonds[flip] = bonds[flip][:, ::-1]
    return bonds


def exclusions_from_bonds(N, bonds):
    """(n_excl uint32[N], excl uint32[N, width]): the bonded partners of the particles below N."""
    partners = [[] for _ in range(N)]
    for a, b in np.asarray(bonds, dtype=np.int64).reshape(-1, 2):
        if a < N:
            partners[a].append(b)
        if b < N:
            partners[b].append(a)
    n_excl = np.array([len(p) for p in partners], dtype=np.uint32)
    excl = np.zeros((N, max(int(n_excl.max()) if N else 0, 1)), dtype=np.uint32)
    for i, p in enumerate(partners):
        excl[i, :len(p)] = p
    return n_excl, excl
