"""Seeded systems for the dihedral tests (NumPy only; imports nothing of the project): the 375-particle parity system
and its reference results, computed once per (potential, box) by tests/dihedral_ref.py and shared by the GPU tests."""

import functools
import math

import numpy as np

import dihedral_ref as ref

N_CHAINS, CHAIN_LEN = 40, 9
N_PARITY = 375
BOXES = {"cubic": ((14.0, 14.0, 14.0), (0.0, 0.0, 0.0)), "triclinic": ((14.0, 13.0, 15.0), (0.2, -0.1, 0.15))}
PARAMS = {"Periodic": [dict(k=10.0, d=1, n=1, phi0=0.0), dict(k=6.0, d=-1, n=3, phi0=0.6)],
          "OPLS": [dict(k1=3.0, k2=-1.5, k3=2.0, k4=0.7), dict(k1=-2.0, k2=4.0, k3=0.5, k4=-1.2)]}
MIN_SIN = 0.4  # the sine of every bend angle (a, b, c and b, c, d) of the parity system is at least this
RING = (360, 361, 362, 363)
CENTRE, LEFT, RIGHT = (364, 365), (366, 367, 368), (369, 370, 371)
LONE = (372, 373, 374)


def wrap(xyz, L, tilt=(0.0, 0.0, 0.0)):
    """Into the centred box through fractional coordinates."""
    h = ref.box_matrix(L, tilt)
    f = np.linalg.solve(h, np.asarray(xyz, dtype=np.float64).T)
    f -= np.floor(f + 0.5)
    return np.ascontiguousarray((h @ f).T)


def random_chain(rng, start, length, bond=(0.9, 1.1), theta=(0.5, math.pi - 0.5)):
    """A random walk with bond lengths and bending angles drawn from the given ranges; the torsions are uniform."""
    x = np.zeros((length, 3))
    x[0] = start
    u = rng.normal(size=3)
    u /= np.linalg.norm(u)
    x[1] = x[0] + rng.uniform(*bond) * u
    for i in range(2, length):
        back = (x[i - 2] - x[i - 1]) / np.linalg.norm(x[i - 2] - x[i - 1])
        n = np.cross(back, rng.normal(size=3))
        n /= np.linalg.norm(n)
        th = rng.uniform(*theta)
        x[i] = x[i - 1] + rng.uniform(*bond) * (math.cos(th) * back + math.sin(th) * n)
    return x


def _bend_sine(x, y, z):
    u, v = x - y, z - y
    c = u @ v / math.sqrt((u @ u) * (v @ v))
    return math.sqrt(max(1.0 - c * c, 0.0))


@functools.lru_cache(maxsize=None)
def parity_system(box="cubic"):
    """375 particles (block boundaries at 64, 128 and 256 are crossed, 375 is no multiple of 64): 40 chains of 9 whose
    dihedral types alternate (rows 0-359, an interior bead has 4 table entries), a puckered 4-ring with all four
    cyclic dihedrals on the same four particles (360-363), a branched cluster -- a centre bond 364-365 with three
    neighbours on either side, 9 dihedrals, so that each centre particle carries 9 table entries, more than the
    kernel's batch -- (364-371) and three particles without dihedrals (372-374). Positions are wrapped into the box, so
    dihedrals straddle every periodic face. Returns (xyz, dihedrals, typeid, L, tilt)."""
    L, tilt = BOXES[box]
    rng = np.random.default_rng(2025)
    xyz = np.zeros((N_PARITY, 3))
    dihedrals = []
    for c in range(N_CHAINS):
        first = c * CHAIN_LEN
        xyz[first:first + CHAIN_LEN] = random_chain(rng, rng.uniform(-6.5, 6.5, size=3), CHAIN_LEN)
        dihedrals += ref.chain_dihedrals(first, CHAIN_LEN)
    xyz[list(RING)] = np.array([[0.0, 0.0, 0.25], [1.0, 0.05, -0.25], [1.05, 1.0, 0.3], [-0.05, 0.95, -0.2]]) + np.array([6.7, -6.6, 3.0])
    dihedrals += ref.ring_dihedrals(*RING)
    o = np.array([-6.8, 6.5, -6.9])
    xyz[CENTRE[0]], xyz[CENTRE[1]] = o, o + np.array([1.0, 0.1, -0.05])
    xyz[list(LEFT)] = o + np.array([[-0.5, 0.8, 0.1], [-0.4, -0.5, 0.7], [-0.45, -0.35, -0.75]])
    xyz[list(RIGHT)] = xyz[CENTRE[1]] + np.array([[0.45, 0.2, 0.85], [0.5, -0.85, -0.2], [0.4, 0.6, -0.7]])
    dihedrals += ref.branched_dihedrals(LEFT, CENTRE[0], CENTRE[1], RIGHT)
    xyz[list(LONE)] = rng.uniform(-6.5, 6.5, size=(3, 3))
    typeid = np.arange(len(dihedrals)) % 2
    # conditioning, checked on the unwrapped coordinates
    for a, b, c, d in dihedrals:
        assert _bend_sine(xyz[a], xyz[b], xyz[c]) >= MIN_SIN and _bend_sine(xyz[b], xyz[c], xyz[d]) >= MIN_SIN, (a, b, c, d)
        assert max(np.abs(xyz[b] - xyz[a]).max(), np.abs(xyz[c] - xyz[b]).max(), np.abs(xyz[d] - xyz[c]).max()) < 2.0
    return wrap(xyz, L, tilt), np.array(dihedrals), typeid, L, tilt


@functools.lru_cache(maxsize=None)
def parity_reference(name, box="cubic"):
    xyz, dihedrals, typeid, L, tilt = parity_system(box)
    return ref.evaluate(name, PARAMS[name], xyz, dihedrals, typeid, L, tilt)


def chain_bonds():
    """The bonds of the 40 chains of the parity system."""
    return np.array([(c * CHAIN_LEN + i, c * CHAIN_LEN + i + 1) for c in range(N_CHAINS) for i in range(CHAIN_LEN - 1)])


def chain_angles():
    """The angles of the 40 chains of the parity system."""
    return np.array([(c * CHAIN_LEN + i, c * CHAIN_LEN + i + 1, c * CHAIN_LEN + i + 2) for c in range(N_CHAINS)
                     for i in range(CHAIN_LEN - 2)])


EDGE_PHI = (0.0, math.pi, math.pi - 1e-9, -(math.pi - 1e-9), 1.0)


def edge_system():
    """Five separate dihedrals in a cubic box of 20 with a = o + (1, 0, 0), b = o, c = o + (0, 0, 1) and
    d = o + (cos phi, sin phi, 1), which has the dihedral angle phi: exactly 0 (cis, d = o + (1, 0, 1)), exactly pi
    (trans, d = o + (-1, 0, 1)) -- the origins are small integers, so these coordinates are exact in binary and the four
    members are exactly coplanar -- pi - 1e-9 and -(pi - 1e-9), on either side of the cut of atan2, and phi = 1.

    The last one is there for the scale of the comparison. Where U' vanishes at 0 and pi (Periodic with phi0 = 0, OPLS)
    the forces of the first four are 1e-8 k at the most, while the reference's own phi carries the rounding of atan2
    near pi, ulp(pi) = 4.4e-16, an absolute error of k ulp(pi) in the force: 1e-10 of an array holding those four alone
    would be a bound of 1e-18, which the reference itself misses. With a dihedral in general position in the array, the
    parity bound is 1e-10 of a force of order k, as for every other system. Returns (xyz, dihedrals, L)."""
    xyz = []
    for o, phi in zip(((4.0, 0.0, 0.0), (-4.0, 2.0, 0.0), (0.0, -5.0, 1.0), (0.0, 5.0, -2.0), (3.0, 3.0, 3.0)), EDGE_PHI):
        o = np.array(o)
        d = {0.0: (1.0, 0.0, 1.0), math.pi: (-1.0, 0.0, 1.0)}.get(phi, (math.cos(phi), math.sin(phi), 1.0))
        xyz += [o + [1.0, 0.0, 0.0], o, o + [0.0, 0.0, 1.0], o + np.array(d)]
    return np.array(xyz), np.array([(4 * j, 4 * j + 1, 4 * j + 2, 4 * j + 3) for j in range(5)]), (20.0, 20.0, 20.0)


PARAMS_EDGE = {"Periodic-n1": ("Periodic", dict(k=10.0, d=1, n=1, phi0=0.0)),
               "Periodic-n2": ("Periodic", dict(k=8.0, d=-1, n=2, phi0=0.7)),
               "Periodic-n3": ("Periodic", dict(k=6.0, d=1, n=3, phi0=-1.1)),
               "OPLS": ("OPLS", dict(k1=3.0, k2=-1.5, k3=2.0, k4=0.7))}
