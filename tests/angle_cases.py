"""Seeded systems for the angle tests (NumPy only; imports nothing of the project): the 367-particle parity system
and its reference results, computed once per (potential, box) by tests/angle_ref.py and shared by the GPU tests."""

import functools
import math

import numpy as np

import angle_ref as ref

N_CHAINS, CHAIN_LEN = 40, 9
N_PARITY = 367
BOXES = {"cubic": ((14.0, 14.0, 14.0), (0.0, 0.0, 0.0)), "triclinic": ((14.0, 13.0, 15.0), (0.2, -0.1, 0.15))}
PARAMS = [dict(k=10.0, t0=2.0), dict(k=25.0, t0=2.8)]
MIN_SIN = 0.1  # every angle of the parity system stays this far from 0 and pi (theta = acos c is ill-conditioned there)


def wrap(xyz, L, tilt=(0.0, 0.0, 0.0)):
    """Into the centred box through fractional coordinates."""
    h = ref.box_matrix(L, tilt)
    f = np.linalg.solve(h, np.asarray(xyz, dtype=np.float64).T)
    f -= np.floor(f + 0.5)
    return np.ascontiguousarray((h @ f).T)


def random_chain(rng, start, length, bond=(0.9, 1.1), theta=(0.3, math.pi - 0.3)):
    """A random walk with bond lengths and bending angles drawn from the given ranges."""
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


@functools.lru_cache(maxsize=None)
def parity_system(box="cubic"):
    """367 particles (a block boundary at 256 is crossed): 40 chains of 9 whose angle types alternate (rows 0-359),
    a triangle with three angles on the same three particles (360-362), a 6-arm star whose centre (363) is the vertex
    of 15 angles -- more table entries than the kernel's batch -- and whose arms are the first beads of chains 0-5,
    and three particles without angles (364-366). Positions are wrapped into the box, so members sit across every
    periodic face. Returns (xyz, angles, typeid, L, tilt)."""
    L, tilt = BOXES[box]
    rng = np.random.default_rng(2024)
    xyz = np.zeros((N_PARITY, 3))
    angles = []
    for c in range(N_CHAINS):
        first = c * CHAIN_LEN
        # (chains 0-5 start close together: their first beads are the arms of the star)
        start = rng.uniform(-2.5, 2.5, size=3) if c < 6 else rng.uniform(-6.5, 6.5, size=3)
        xyz[first:first + CHAIN_LEN] = random_chain(rng, start, CHAIN_LEN)
        angles += ref.chain_angles(first, CHAIN_LEN)
    xyz[360:363] = np.array([[0.0, 0.0, 0.0], [1.1, 0.0, 0.0], [0.4, 0.9, 0.2]]) + np.array([6.6, -6.4, 3.0])
    angles += ref.triangle_angles(360, 361, 362)
    arms = [c * CHAIN_LEN for c in range(6)]
    xyz[363] = xyz[arms].mean(axis=0) + np.array([0.3, -0.2, 0.1])
    angles += ref.star_angles(363, arms)
    xyz[364:367] = rng.uniform(-6.5, 6.5, size=(3, 3))
    typeid = np.arange(len(angles)) % 2
    # conditioning, checked on the unwrapped coordinates (arms of the star within the minimum-image range)
    for a, b, c in angles:
        dab, dcb = xyz[a] - xyz[b], xyz[c] - xyz[b]
        cos = dab @ dcb / math.sqrt((dab @ dab) * (dcb @ dcb))
        assert math.sqrt(1.0 - cos * cos) > MIN_SIN and max(np.abs(dab).max(), np.abs(dcb).max()) < 6.0
    return wrap(xyz, L, tilt), np.array(angles), typeid, L, tilt


@functools.lru_cache(maxsize=None)
def parity_reference(name, box="cubic"):
    xyz, angles, typeid, L, tilt = parity_system(box)
    return ref.evaluate(name, PARAMS, xyz, angles, typeid, L, tilt)


def chain_bonds():
    """The bonds of the 40 chains of the parity system."""
    return np.array([(c * CHAIN_LEN + i, c * CHAIN_LEN + i + 1) for c in range(N_CHAINS) for i in range(CHAIN_LEN - 1)])


def edge_system():
    """Four separate angles in a cubic box of 20, coordinates exact in binary where exactness matters:
    0 and 1 exactly collinear (theta = pi, c = -1 exactly), 2 with theta = 5e-4 (sin theta below the 1e-3 floor),
    3 with theta = 1e-2 (above it). Angle types: 0, 1, 1, 0 -- PARAMS_EDGE gives type 0 t0 = pi and type 1 t0 = 2."""
    xyz, angles = [], []
    for o in ((4.0, 0.0, 0.0), (-4.0, 2.0, 0.0)):
        o = np.array(o)
        xyz += [o + [1.0, 0.0, 0.0], o, o + [-2.0, 0.0, 0.0]]
    for o, th in (((0.0, -5.0, 1.0), 5e-4), ((0.0, 5.0, -1.0), 1e-2)):
        o = np.array(o)
        xyz += [o + [1.0, 0.0, 0.0], o, o + 1.3 * np.array([math.cos(th), math.sin(th), 0.0])]
    angles = [(3 * j, 3 * j + 1, 3 * j + 2) for j in range(4)]
    return np.array(xyz), np.array(angles), np.array([0, 1, 1, 0]), (20.0, 20.0, 20.0)


PARAMS_EDGE = [dict(k=10.0, t0=math.pi), dict(k=10.0, t0=2.0)]
