"""Fixtures shared by tests/test_rdf.py (which checks every random one for edge pairs on the CPU) and
tests/test_gpu_rdf.py. A fixture is a dict: xyz (n, 3), types (n,), type_names, box = (L, tilt, periodic), r_max,
num_bins and ``groups``: the (filter_a, filter_b) pairs it is used with, a filter being None (All) or a tuple of type
names. Every seed below was checked with ``rdf_ref.edge_pairs(...) == 0`` for each of its groups (test_rdf.py repeats
the check); none had to be skipped."""

import numpy as np

TYPE_NAMES = ("A", "B", "C", "D")  # (no particle is of type D: Type(["D"]) is an empty group)
ALL_ALL = (None, None)
AB_BC = (("A", "B"), ("B", "C"))
EMPTY = (("D",), None)
ORTHO = (0.0, 0.0, 0.0)
PBC = (1, 1, 1)


def mask(names, type_names=TYPE_NAMES):
    """One flag per type for a group given as a tuple of type names; None (every particle) stays None."""
    return None if names is None else np.array([t in names for t in type_names], dtype=np.uint8)


def _uniform(n, L, seed, tilt=ORTHO, stretch_z=1.0):
    rng = np.random.default_rng(seed)
    f = rng.random((n, 3)) - 0.5
    f[:, 2] *= stretch_z
    L = np.asarray(L, dtype=np.float64)
    xy, xz, yz = tilt
    z = f[:, 2] * L[2]
    y = f[:, 1] * L[1] + yz * z
    x = f[:, 0] * L[0] + xy * f[:, 1] * L[1] + xz * z  # (f_x a + f_y b + f_z c of the HOOMD box)
    return np.stack([x, y, z], axis=1), rng.integers(0, 3, n)


def _fixture(xyz, types, L, r_max, num_bins, groups, tilt=ORTHO, periodic=PBC):
    return dict(xyz=np.ascontiguousarray(xyz, dtype=np.float64), types=np.asarray(types, dtype=np.int64), type_names=TYPE_NAMES,
                box=(tuple(float(x) for x in np.broadcast_to(L, (3,))), tuple(tilt), tuple(periodic)), r_max=float(r_max),
                num_bins=int(num_bins), groups=tuple(groups))


def tile(n):
    """All-pairs tile and mask edges: n uniform random points (n = 1: one particle at the origin); r_max = 4 in a box
    of 10 gives two cells per axis, so only the all-pairs path is valid."""
    if n == 1:
        return _fixture(np.zeros((1, 3)), [1], 10.0, 4.0, 64, (ALL_ALL, AB_BC))
    xyz, types = _uniform(n, (10.0, 10.0, 10.0), 100 + n)
    return _fixture(xyz, types, 10.0, 4.0, 64, (ALL_ALL, AB_BC) + ((EMPTY,) if n == 257 else ()))


TILE_SIZES = (1, 2, 255, 256, 257, 1000)


def bins(num_bins):
    xyz, types = _uniform(300, (9.0, 9.0, 9.0), 7)
    return _fixture(xyz, types, 9.0, 3.0, num_bins, (ALL_ALL,))


BIN_COUNTS = (1, 64, 1000, 8192)


def cells(name):
    """Fixtures on which both paths are valid (r_max = 2.5): 3, 4 and 5 cells per axis, a non-cubic grid, a
    non-periodic axis with particles beyond its faces, a non-cubic box and a cluster that puts half the particles into
    one cell."""
    if name == "three":
        L, seed = (7.5, 7.5, 7.5), 11
    elif name == "four":
        L, seed = (10.0, 10.0, 10.0), 12
    elif name == "five":
        L, seed = (12.5, 12.5, 12.5), 13
    elif name == "noncubic":
        L, seed = (7.5, 10.3, 13.1), 14
    elif name == "slab":
        # z is not periodic: two clamped cells, and a fifth of the particles lie beyond the faces in z
        xyz, types = _uniform(600, (8.0, 9.0, 5.0), 15, stretch_z=1.25)
        return _fixture(xyz, types, (8.0, 9.0, 5.0), 2.5, 50, (ALL_ALL, AB_BC), periodic=(1, 1, 0))
    elif name == "cluster":
        xyz, types = _uniform(600, (10.0, 10.0, 10.0), 16)
        rng = np.random.default_rng(17)
        xyz[:300] = np.array([-5.0, -2.5, 0.0]) + 0.05 + 2.4 * rng.random((300, 3))  # inside cell (0, 1, 2) of the 4^3 grid
        return _fixture(xyz, types, 10.0, 2.5, 50, (ALL_ALL, AB_BC))
    else:
        raise KeyError(name)
    xyz, types = _uniform(600, L, seed)
    return _fixture(xyz, types, L, 2.5, 50, (ALL_ALL, AB_BC))


CELL_NAMES = ("three", "four", "five", "noncubic", "slab", "cluster")


def two_cells():
    """Two cells of width r_max on x: the cells path is not valid, path 0 has to take all-pairs."""
    xyz, types = _uniform(400, (6.0, 10.0, 10.0), 21)
    return _fixture(xyz, types, (6.0, 10.0, 10.0), 2.5, 50, (ALL_ALL,))


def triclinic():
    """All three tilts non-zero. Perpendicular widths 8.24, 9.28, 11: r_max = 4 is below half of each."""
    L, tilt = (9.0, 10.0, 11.0), (0.3, -0.2, 0.4)
    xyz, types = _uniform(400, L, 31, tilt=tilt)
    return _fixture(xyz, types, L, 4.0, 80, (ALL_ALL, AB_BC), tilt=tilt)


def random_fixtures():
    """name -> fixture, every random fixture the GPU tests compare with the reference."""
    out = {"tile%d" % n: tile(n) for n in TILE_SIZES}
    out.update({"bins%d" % n: bins(n) for n in BIN_COUNTS})
    out.update({"cells_" + n: cells(n) for n in CELL_NAMES})
    out["two_cells"] = two_cells()
    out["triclinic"] = triclinic()
    return out


def dyadic_lattice():
    """Simple cubic lattice of spacing 1 filling a box of 8: 512 particles, every coordinate a multiple of 1/8 (offset
    -3.875), r_max = 4, 32 bins, scale = 8: every operation is exact in any order, with or without FMA. Every particle
    has 6 neighbours at r = 1 (bin 8, on its lower edge: all hits of a wave share one bin), 6 at r = 2 (bin 16, on its
    lower edge) and 6 at r = 4 = r_max (excluded)."""
    g = np.arange(8) - 3.875
    xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    types = (np.arange(512) % 3)
    return _fixture(xyz, types, 8.0, 4.0, 32, (ALL_ALL, AB_BC))


def dyadic_points():
    """Hand-placed points (multiples of 1/8) in the same box: pairs at r = 2 (bin 16), r = 2.5 (bin 20: (1.5, 2, 0)),
    r = 4 (excluded) and r = 3.875 (bin 31, the last)."""
    xyz = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [1.5, 2.0, 0.0], [0.0, 0.0, 4.0], [0.0, -3.875, 0.0], [-3.0, 0.125, -3.0]])
    return _fixture(xyz, [0, 0, 0, 0, 0, 0], 8.0, 4.0, 32, (ALL_ALL,))
