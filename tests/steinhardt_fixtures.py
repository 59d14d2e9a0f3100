"""Fixtures shared by tests/test_steinhardt.py (which checks each one's own conditions on the CPU: no pair within 1e-9
of r_max^2, no bond within 1e-6 of q_threshold, no q_l within 1e-8 of a histogram edge) and tests/test_gpu_steinhardt.py.
A fixture is a dict: xyz (n, 3), types (n,), type_names, box = (L, tilt, periodic), r_max. The row tile and the
candidate chunk of the kernels are 256: the sizes are 256, 257 and 515."""

import numpy as np

TYPE_NAMES = ("A", "B", "C")
ORTHO = (0.0, 0.0, 0.0)
PBC = (1, 1, 1)
AB = ("A", "B")
NUM_BINS = 100


def mask(names):
    """One flag per type for a group given as a tuple of type names; None (every particle) stays None."""
    return None if names is None else np.array([t in names for t in TYPE_NAMES], dtype=np.uint8)


def _fixture(xyz, types, L, r_max, tilt=ORTHO, periodic=PBC):
    xyz = np.ascontiguousarray(xyz, dtype=np.float64)
    return dict(xyz=xyz, types=np.asarray(types, dtype=np.int64), type_names=TYPE_NAMES,
                box=(tuple(float(x) for x in np.broadcast_to(L, (3,))), tuple(tilt), tuple(periodic)), r_max=float(r_max))


def _lattice(basis, cells, a=2.0):
    g = np.arange(cells) * a
    origin = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 1, 3)
    xyz = (origin + np.asarray(basis, dtype=np.float64)[None, :, :] * a).reshape(-1, 3)
    return xyz - 0.5 * cells * a + 0.25  # (multiples of 1/4: every separation is exact)


FCC = ((0, 0, 0), (0.5, 0.5, 0), (0.5, 0, 0.5), (0, 0.5, 0.5))
BCC = ((0, 0, 0), (0.5, 0.5, 0.5))
SC = ((0, 0, 0),)

# name -> (basis, r_max, neighbours, (q4, q6)); 4 x 4 x 4 cells of a = 2 in a box of 8
LATTICES = {
    "fcc": (FCC, 1.6, 12, (0.190941, 0.574524)),
    "bcc8": (BCC, 1.8, 8, (0.509175, 0.628539)),
    "bcc14": (BCC, 2.2, 14, (0.036370, 0.510688)),
    "sc": (SC, 2.5, 6, (0.763763, 0.353553)),
}


def lattice(name):
    """fcc (256 particles), bcc (128) or sc (64) on dyadic positions, one type."""
    basis, r_max = LATTICES[name][:2]
    xyz = _lattice(basis, 4)
    return _fixture(xyz, np.zeros(xyz.shape[0]), 8.0, r_max)


def _uniform(n, L, seed, tilt=ORTHO):
    rng = np.random.default_rng(seed)
    f = rng.random((n, 3)) - 0.5
    L = np.broadcast_to(np.asarray(L, dtype=np.float64), (3,))
    xy, xz, yz = tilt
    z = f[:, 2] * L[2]
    y = f[:, 1] * L[1] + yz * z
    x = f[:, 0] * L[0] + xy * f[:, 1] * L[1] + xz * z
    return np.stack([x, y, z], axis=1), rng.integers(0, 3, n)


TILT = (0.2, -0.1, 0.3)


def random(n, kind="cube"):
    """n uniform points of three types in a box of 8 with r_max = 2 (four cells per axis): ``cube``; ``tilted`` (all
    three tilts, all-pairs only); ``slab`` (z not periodic)."""
    if kind == "cube":
        xyz, types = _uniform(n, 8.0, 1000 + n)
        return _fixture(xyz, types, 8.0, 2.0)
    if kind == "tilted":
        xyz, types = _uniform(n, 8.0, 2000 + n, tilt=TILT)
        return _fixture(xyz, types, 8.0, 2.0, tilt=TILT)
    if kind == "slab":
        xyz, types = _uniform(n, 8.0, 3000 + n)
        return _fixture(xyz, types, 8.0, 2.0, periodic=(1, 1, 0))
    raise KeyError(kind)


RANDOM = {"cube257": (257, "cube"), "cube515": (515, "cube"), "tilted257": (257, "tilted"), "tilted515": (515, "tilted"),
          "slab257": (257, "slab")}


def sparse():
    """40 points in a cube of 12 with r_max = 1.5: some have no neighbour."""
    xyz, types = _uniform(40, 12.0, 51)
    return _fixture(xyz, types, 12.0, 1.5)


def blob():
    """300 points within 0.9 of the centre (1, 1, 1) of one cell of the 4^3 grid of a cube of 8, r_max = 2: one cell
    holds more than 256 rows, every row has more than 256 candidates, and every particle has the other 299 as
    neighbours (the diameter is 1.8)."""
    rng = np.random.default_rng(61)
    v = rng.normal(size=(300, 3))
    v *= (0.9 * rng.random(300) ** (1.0 / 3.0) / np.linalg.norm(v, axis=1))[:, None]
    return _fixture(v + 1.0, rng.integers(0, 3, 300), 8.0, 2.0)


TWO_PHASE = dict(l=6, q_threshold=0.7, solid_threshold=8)


def two_phase():
    """An fcc lattice (256 particles, a = 2, box of 8) jittered by up to 0.03 per coordinate where x < 0 and by up to
    0.35 where x >= 0; r_max = 1.75."""
    xyz = _lattice(FCC, 4)
    rng = np.random.default_rng(71)
    amp = np.where(xyz[:, 0] < 0.0, 0.03, 0.35)[:, None]
    xyz = xyz + amp * (2.0 * rng.random(xyz.shape) - 1.0)
    return _fixture(xyz, np.zeros(xyz.shape[0]), 8.0, 1.75)
