"""Fixtures shared by tests/test_cluster_properties.py (which checks each one's own conditions on the CPU) and
tests/test_gpu_cluster_properties.py: those of tests/cluster_fixtures.py and the ones below, which put clusters across the
periodic boundary and rows of several clusters into one wave. A fixture is the dict of tests/steinhardt_fixtures.py."""

import functools

import numpy as np

import cluster_fixtures as cf
import cluster_properties_ref as pref
import cluster_ref
import steinhardt_fixtures as sf
import steinhardt_ref

GROUPS = cf.GROUPS
NOT_PERIODIC = (0, 0, 0)


def wrap_cube(xyz, L):
    """Positions brought back into the cube [-L/2, L/2)^3."""
    xyz = np.asarray(xyz, dtype=np.float64)
    return xyz - L * np.floor((xyz + 0.5 * L) / L)


def dimer():
    """Two particles 0.5 apart across the face x = 4 of a cube of 8."""
    return sf._fixture([[3.875, 1.0, -2.0], [-3.625, 1.25, -2.0]], [0, 1], 8.0, 1.0)


ROD_N, ROD_SPACING = 65, 1.0 / 160.0


def rod():
    """65 particles along the first lattice vector of the tilted box of steinhardt_fixtures (L = 8), 1/160 of it apart (0.05;
    the rod extends over 0.4 of the box: compact), through the corner region (+, +, +): fractional coordinates
    s_x = 249/256 + k/160 mod 1 (the rod leaves through the face s_x = 1 after its fourth particle), s_y = s_z = 1 - 1/256
    (1/32 from the two other faces of that corner)."""
    L, (xy, xz, yz) = 8.0, sf.TILT
    H = np.array([[L, xy * L, xz * L], [0.0, L, yz * L], [0.0, 0.0, L]])
    s = np.empty((ROD_N, 3))
    s[:, 0] = np.mod(63.0 / 64.0 - 3.0 / 256.0 + ROD_SPACING * np.arange(ROD_N), 1.0)
    s[:, 1] = 1.0 - 1.0 / 256.0
    s[:, 2] = 1.0 - 1.0 / 256.0
    xyz = (s - 0.5) @ H.T
    return sf._fixture(xyz, np.arange(ROD_N) % 3, L, 0.19, tilt=sf.TILT)


@functools.lru_cache(maxsize=None)
def _two_phase_solid_rows():
    f, p = sf.two_phase(), sf.TWO_PHASE
    st = steinhardt_ref.reference(f["xyz"], f["types"], f["box"], None, (p["l"],), f["r_max"], q_threshold=p["q_threshold"])
    return np.flatnonzero(st["num_connections"] >= p["solid_threshold"])


def two_phase_solid():
    """The solid particles of steinhardt_fixtures.two_phase() (138) as a system of their own at its r_max = 1.75: a
    slab that spans the box in y and z, so its one cluster is not compact."""
    f = sf.two_phase()
    rows = _two_phase_solid_rows()
    return sf._fixture(f["xyz"][rows], f["types"][rows], 8.0, f["r_max"])


# through each face, each edge and the corner of the cube, in units of the fixture's own shift
DIRECTIONS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
# name -> (builder, the shift that carries the fixture's clusters across the boundary)
TRANSLATED = {"blob": (sf.blob, 3.0), "bridge": (cf.bridge, 4.0), "two_phase_solid": (two_phase_solid, 3.0)}


def translated(name, direction):
    """Fixture ``name`` moved by ``shift * direction`` and wrapped back into its cube of 8; ``vector`` is the move."""
    build, shift = TRANSLATED[name]
    f = dict(build())
    v = shift * np.asarray(direction, dtype=np.float64)
    f["xyz"] = np.ascontiguousarray(wrap_cube(f["xyz"] + v, 8.0))
    f["vector"] = v
    return f


def _ball(rng, n, radius):
    v = rng.normal(size=(n, 3))
    return v * (radius * rng.random(n) ** (1.0 / 3.0) / np.linalg.norm(v, axis=1))[:, None]


def interleaved():
    """Two blobs of 70 (radius 0.9, r_max = 2: every pair inside one is an edge) around (-1.5, -1.5, -1.5) and (2, 2, 2),
    their rows alternating: every wave holds lanes of two clusters in turn."""
    rng = np.random.default_rng(81)
    a = _ball(rng, 70, 0.9) - 1.5
    b = _ball(rng, 70, 0.9) + 2.0
    xyz = np.empty((140, 3))
    xyz[0::2] = a
    xyz[1::2] = b
    return sf._fixture(xyz, rng.integers(0, 3, 140), 8.0, 2.0)


def dimers():
    """32 dimers (0.3 apart, r_max = 0.5) on a 4 x 4 x 2 grid of spacing 2 in 64 consecutive rows: one wave, 32 clusters
    of two lanes each."""
    rng = np.random.default_rng(82)
    g = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(2), indexing="ij"), axis=-1).reshape(-1, 3) * 2.0 - 3.0
    g = g + 0.2 * (rng.random(g.shape) - 0.5)
    xyz = np.empty((64, 3))
    xyz[0::2] = g
    xyz[1::2] = g + np.array([0.3, 0.0, 0.0])
    return sf._fixture(xyz, np.zeros(64), 8.0, 0.5)


ONE_CLUSTER_N = (1, 63, 64, 65, 257, 1030, 4096)


def one_cluster(n):
    """n points within 0.9 of (1, 1, 1) in a cube of 8 without a periodic axis, r_max = 2: one cluster of all n by
    construction (the diameter is 1.8). The sizes sit on both sides of a wave (64), of a workgroup (256) and of the scan's
    workgroup (1024); 4096 has shift = 49."""
    rng = np.random.default_rng(9000 + n)
    return sf._fixture(_ball(rng, n, 0.9) + 1.0, np.zeros(n), 8.0, 2.0, periodic=NOT_PERIODIC)


# every fixture that goes through both references; the one_cluster fixtures have a reference of their own (no unwrapping)
FIXTURES = dict(cf.FIXTURES)
FIXTURES.update({"dimer": dimer, "rod": rod, "two_phase_solid": two_phase_solid, "interleaved": interleaved, "dimers": dimers})
for _name in TRANSLATED:
    for _k, _d in enumerate(DIRECTIONS):
        FIXTURES["%s_moved%d" % (_name, _k)] = (lambda n=_name, d=_d: translated(n, d))

NEVER_COMPACT = ("ring_ascending", "ring_descending", "ring_shuffled", "sc")  # (they wrap round the box)


def random_fixture(name):
    """Whether ``name`` is one of the fixtures the bound of 4 non-compact clusters applies to (not ``ring_*``, not ``sc``)."""
    return not name.startswith("ring_") and name != "sc"


@functools.lru_cache(maxsize=None)
def fixture(name):
    return FIXTURES[name]()


@functools.lru_cache(maxsize=None)
def expected(name, group):
    """Computed once per (fixture, group) and shared; nobody writes to it: the labels of tests/cluster_ref.py and the two
    references of tests/cluster_properties_ref.py on them, as (labels, by_edges, by_formula)."""
    f = fixture(name)
    out = cluster_ref.reference(f["xyz"], f["types"], f["box"], sf.mask(group), f["r_max"], tags=cf.tags_of(f))
    return out, pref.by_edges(f["xyz"], f["box"], out["keys"], f["r_max"]), pref.by_formula(f["xyz"], f["box"], out["keys"])
