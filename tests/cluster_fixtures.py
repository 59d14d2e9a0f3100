"""Fixtures shared by tests/test_cluster.py (which checks each one's own condition on the CPU: no pair within 1e-9 of
r_max^2, and re-derives the figures below) and tests/test_gpu_cluster.py. A fixture is the dict of
tests/steinhardt_fixtures.py (xyz, types, type_names, box = (L, tilt, periodic), r_max) with an optional ``tags`` (n,).
The positions come from steinhardt_fixtures; the cut-offs are chosen for the percolation regime, where clusters of
every size exist. The row tile and the candidate chunk of the walk are 256: the sizes are 257, 300, 515, 600, 1030."""

import numpy as np

import steinhardt_fixtures as sf

TYPE_NAMES = sf.TYPE_NAMES
AB = sf.AB
GROUPS = (None, AB)
SIZE_BINS = 64


def _with(f, r_max, tags=None):
    f = dict(f)
    f["r_max"] = float(r_max)
    if tags is not None:
        f["tags"] = np.asarray(tags, dtype=np.uint32)
    return f


# name -> (builder of the positions, r_max, clusters, edges, largest) for the group of all particles; the figures are
# from scipy on the all-pairs distances, minimum over the 27 nearest images, and tests/test_cluster.py re-derives them
def _uniform1030():
    xyz, types = sf._uniform(1030, 8.0, 2030)
    return sf._fixture(xyz, types, 8.0, 0.6)


PERCOLATION = {
    "cube257": (lambda: sf.random(257, "cube"), 0.9, 116, 184, 13),
    "cube515_lo": (lambda: sf.random(515, "cube"), 0.75, 169, 453, 24),
    "cube515_hi": (lambda: sf.random(515, "cube"), 0.85, 63, 675, 229),
    "tilted515": (lambda: sf.random(515, "tilted"), 0.8, 134, 544, 45),
    "slab257": (lambda: sf.random(257, "slab"), 0.95, 80, 234, 23),
    "uniform1030": (_uniform1030, 0.6, 318, 952, 59),
}

RING_N, RING_SPACING, RING_BOX, RING_R_MAX = 600, 0.125, (75.0, 2.0, 2.0), 0.19
RING_TAGS = ("ascending", "descending", "shuffled")


def ring(tags="ascending", removed=()):
    """600 particles on a line along x, spacing 1/8, in a periodic box (75, 2, 2) with r_max = 0.19: the chain closes
    through the boundary (one cluster, 600 edges). ``tags`` along the line: ascending, descending or a seeded
    permutation; ``removed``: positions along the line that are left out."""
    k = np.array([i for i in range(RING_N) if i not in set(removed)])
    xyz = np.zeros((k.shape[0], 3))
    xyz[:, 0] = -37.5 + RING_SPACING * k + 0.0625  # (multiples of 1/16: every separation is exact)
    xyz[:, 1] = 0.25
    xyz[:, 2] = -0.5
    t = {"ascending": np.arange(RING_N), "descending": np.arange(RING_N)[::-1],
         "shuffled": np.random.default_rng(600).permutation(RING_N)}[tags][k]
    return _with(sf._fixture(xyz, np.asarray(k % 3), RING_BOX, RING_R_MAX), RING_R_MAX, tags=t)


BRIDGE_A = ((-0.9, 0.0, 0.0), (-1.5, 0.0, 0.0), (-1.5, 0.5, 0.0), (-2.0, 0.25, 0.3), (-0.9, 0.6, 0.1))
BRIDGE_B = ((0.9, 0.0, 0.0), (1.4, 0.1, 0.0), (1.4, -0.4, 0.2), (1.9, 0.3, -0.2))
BRIDGE_C = ((0.0, 0.0, 0.0),)


def bridge():
    """Two compact groups, five particles of type A and four of type B, joined only by one particle of type C at the
    origin that is within r_max = 1 of one particle of each. The C row comes first, so it holds the smallest tag."""
    xyz = np.array(BRIDGE_C + BRIDGE_A + BRIDGE_B)
    types = [2] + [0] * len(BRIDGE_A) + [1] * len(BRIDGE_B)
    return sf._fixture(xyz, types, 8.0, 1.0)


def single():
    return sf._fixture([[0.5, -0.25, 1.0]], [1], 8.0, 1.0)


def sc_singletons():
    """The simple cubic lattice (64 particles, spacing 2) below its spacing: 64 clusters of one, no edge."""
    return _with(sf.lattice("sc"), 1.9)


TWO_PHASE_R_MAX = 1.4  # inside the first shell (1.33 .. 1.50 where the jitter is small): the solid part falls into pieces


def two_phase():
    """sf.two_phase(): the clusters of its solid particles (``sf.TWO_PHASE``) at its own r_max = 1.75 (one cluster) and
    at ``TWO_PHASE_R_MAX`` (11 clusters, the largest of 123)."""
    return sf.two_phase()


# name -> builder; every one is run for both GROUPS on the all-pairs path and, unless tilted, on the cells path
FIXTURES = {name: (lambda b=b, r=r: _with(b(), r)) for name, (b, r, _, _, _) in PERCOLATION.items()}
FIXTURES.update({
    "ring_ascending": lambda: ring("ascending"),
    "ring_descending": lambda: ring("descending"),
    "ring_shuffled": lambda: ring("shuffled"),
    "ring_minus_one": lambda: ring("shuffled", removed=(217,)),
    "ring_minus_two": lambda: ring("shuffled", removed=(100, 350)),
    "bridge": bridge,
    "blob": sf.blob,          # r_max = 2: one cluster of 300, every pair an edge
    "sparse": sf.sparse,      # r_max = 1.5: mostly singletons
    "sc": lambda: sf.lattice("sc"),  # r_max = 2.5: one cluster of 64, 192 edges
    "sc_singletons": sc_singletons,
    "single": single,
})


def tilted(f):
    return any(t != 0.0 for t in f["box"][1])


def tags_of(f):
    return np.asarray(f.get("tags", np.arange(f["xyz"].shape[0])), dtype=np.uint32)
