"""NumPy reference for ``compute.BondedDistribution``: the definitions of ``include/azp.h`` ("distributions of the bonded
coordinates") restated, and the seeded chain systems its tests share. The minimum image and the dihedral angle come
from ``angle_ref`` / ``dihedral_ref`` by import; nothing of the project is imported.

The coordinate ``x`` of a group: ``r = |r_a - r_b|`` for bonds and special pairs on ``[r_min, r_max)``,
``theta = atan2(|dab x dcb|, dab . dcb)`` for angles on [0, pi], ``phi = atan2(|b2| (b1 . n2), n1 . n2)`` for dihedrals on
[-pi, pi]. With ``scale = num_bins / (hi - lo)``: ``k = min(int((x - lo) * scale), num_bins - 1)``; a bond with
``r < r_min`` or ``r >= r_max`` goes to ``outside``."""

import functools
import math

import numpy as np

import angle_ref
import dihedral_ref

ARITY = {"bond": 2, "pair": 2, "angle": 3, "dihedral": 4}


def limits(kind, r_min=None, r_max=None):
    if ARITY[kind] == 2:
        return float(r_min), float(r_max)
    return (0.0, math.pi) if kind == "angle" else (-math.pi, math.pi)


def coordinates(kind, pos, groups, L, tilt=(0.0, 0.0, 0.0)):
    """The coordinate of every group, float64 (m,)."""
    pos = np.asarray(pos, dtype=np.float64)[:, :3]
    groups = np.asarray(groups, dtype=np.int64).reshape(-1, ARITY[kind])
    x = np.zeros(groups.shape[0])
    for j, g in enumerate(groups):
        if ARITY[kind] == 2:
            d = angle_ref.min_image(pos[g[0]] - pos[g[1]], L, tilt)
            x[j] = np.sqrt(d @ d)
        elif kind == "angle":
            dab = angle_ref.min_image(pos[g[0]] - pos[g[1]], L, tilt)
            dcb = angle_ref.min_image(pos[g[2]] - pos[g[1]], L, tilt)
            n = np.cross(dab, dcb)
            x[j] = np.arctan2(np.sqrt(n @ n), dab @ dcb)
        else:
            x[j] = dihedral_ref.angle_of(*dihedral_ref.separations(pos[g[0]], pos[g[1]], pos[g[2]], pos[g[3]], L, tilt))
    return x


def histogram(kind, pos, groups, typeid, n_types, num_bins, L, tilt=(0.0, 0.0, 0.0), r_min=None, r_max=None):
    """dict: ``counts`` int64 (n_types, num_bins), ``outside`` and ``num_groups`` int64 (n_types,), and per group ``x``
    and ``index`` = (x - lo) * scale, the number whose integer part is the bin (for the guard of the exact tests)."""
    lo, hi = limits(kind, r_min, r_max)
    scale = num_bins / (hi - lo)
    typeid = np.asarray(typeid, dtype=np.int64).reshape(-1)
    x = coordinates(kind, pos, groups, L, tilt)
    index = (x - lo) * scale
    inside = (x >= lo) & (x < hi) if ARITY[kind] == 2 else np.ones(x.shape, dtype=bool)
    k = np.minimum(index[inside].astype(np.int64), num_bins - 1)
    counts = np.zeros((n_types, num_bins), dtype=np.int64)
    np.add.at(counts, (typeid[inside], k), 1)
    return dict(counts=counts, outside=np.bincount(typeid[~inside], minlength=n_types).astype(np.int64),
                num_groups=np.bincount(typeid, minlength=n_types).astype(np.int64), x=x, index=index, inside=inside)


def guard(index):
    """The smallest distance of a group's ``index`` from an integer: above it a coordinate that differs from this
    module's in its last bits still falls into the same bin."""
    index = np.asarray(index, dtype=np.float64)
    return float(np.abs(index - np.rint(index)).min()) if index.size else 1.0


# ---------------------------------------------------------------------------
# the chain systems the tests share
# ---------------------------------------------------------------------------
BOXES = {"cubic": ((14.0, 14.0, 14.0), (0.0, 0.0, 0.0)), "triclinic": ((14.0, 13.0, 15.0), (0.2, -0.1, 0.15))}
BOND_RANGE = (0.93, 1.08)   # bond lengths are drawn from [0.9, 1.1): some fall outside on either side
PAIR_RANGE = (1.2, 3.2)     # 1-4 distances


def _wrap(xyz, L, tilt):
    h = angle_ref.box_matrix(L, tilt)
    f = np.linalg.solve(h, np.asarray(xyz, dtype=np.float64).T)
    f -= np.floor(f + 0.5)
    return np.ascontiguousarray((h @ f).T)


def _random_chain(rng, start, length, bond=(0.9, 1.1), theta=(0.5, math.pi - 0.5)):
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


@functools.lru_cache(maxsize=None)
def chain_system(n_chains=40, chain_len=8, box="triclinic", seed=2026):
    """``n_chains`` random-walk chains of ``chain_len`` beads plus one trimer (40 x 8 + 3 = 323 particles: more than one
    block of 256 and no multiple of 64), wrapped into the box, so groups sit across every periodic face. Bonds, angles
    and dihedrals run along the chains; the special pairs are the 1-4 pairs (first and last member of every dihedral).
    The types of every kind alternate between two. Returns a dict: ``xyz``, ``L``, ``tilt`` and per kind
    ``<kind>s`` (members) and ``<kind>_typeid``."""
    L, tilt = BOXES[box]
    rng = np.random.default_rng(seed)
    n = n_chains * chain_len + 3
    xyz = np.zeros((n, 3))
    bonds, angles, dihedrals = [], [], []
    for c in list(range(n_chains)) + ["trimer"]:
        first, length = (c * chain_len, chain_len) if c != "trimer" else (n_chains * chain_len, 3)
        xyz[first:first + length] = _random_chain(rng, rng.uniform(-6.5, 6.5, size=3), length)
        bonds += [(first + i, first + i + 1) for i in range(length - 1)]
        angles += angle_ref.chain_angles(first, length)
        dihedrals += dihedral_ref.chain_dihedrals(first, length)
    out = dict(xyz=_wrap(xyz, L, tilt), L=L, tilt=tilt, bonds=np.array(bonds), angles=np.array(angles),
               dihedrals=np.array(dihedrals))
    out["pairs"] = out["dihedrals"][:, [0, 3]]
    for kind in ARITY:
        out[kind + "_typeid"] = np.arange(len(out[kind + "s"])) % 2
    return out


def ranges(kind):
    """The keyword arguments ``r_min`` / ``r_max`` the tests use for ``kind`` on the chain systems."""
    if ARITY[kind] != 2:
        return {}
    lo, hi = BOND_RANGE if kind == "bond" else PAIR_RANGE
    return dict(r_min=lo, r_max=hi)


@functools.lru_cache(maxsize=None)
def chain_reference(kind, num_bins=64, **system):
    s = chain_system(**system)
    return histogram(kind, s["xyz"], s[kind + "s"], s[kind + "_typeid"], 2, num_bins, s["L"], s["tilt"], **ranges(kind))
