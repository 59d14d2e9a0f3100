"""NumPy restatement of the wall potentials' definition (azplugins_amd.wall, include/azp.h "wall potentials"):
geometries, both potentials, modes and the extrapolated branch, per wall and summed. Plain float64 in the order the
formulas are written; the signed distance uses left-to-right sums and the correctly rounded square root, which is what
the kernel promises for it.

A wall is a dict: ``dict(kind="plane", origin, normal)``, ``dict(kind="sphere", radius, origin, inside)`` or
``dict(kind="cylinder", radius, origin, axis, inside)``. A type's parameters are the dict the Python class takes."""

import math

import numpy as np

import box_ref


def _ln(x):
    # (scalars go through libm, as the C fold does; arrays through numpy)
    return np.log(x) if isinstance(x, np.ndarray) else math.log(x)


def lj93(p, r):
    """(V, F = -dV/dr) of the LJ 9-3 wall at distance r, no shift."""
    s = p["sigma"] / r
    s3 = s * s * s
    s9 = s3 * s3 * s3
    return p["epsilon"] * ((2.0 / 15.0) * s9 - s3), p["epsilon"] * (1.2 * s9 - 3.0 * s3) / r


def colloid(p, z):
    """(V, F = -dV/dz) of the colloid wall at distance z of the particle centre, no shift."""
    a = p["a"]
    s2 = p["sigma"] * p["sigma"]
    C1 = p["A"] * (s2 * s2 * s2) / 7560.0
    C2 = p["A"] / 6.0
    m = z - a
    q = z + a
    m2, q2 = m * m, q * q
    m7, q7 = m2 * m2 * m2 * m, q2 * q2 * q2 * q
    D = z * z - a * a
    V = C1 * ((7.0 * a - z) / m7 + (7.0 * a + z) / q7) - C2 * (2.0 * a * z / D + _ln(m / q))
    F = 6.0 * C1 * ((8.0 * a - z) / (m7 * m) + (8.0 * a + z) / (q7 * q)) - 4.0 * C2 * (a * a * a) / (D * D)
    return V, F


POTENTIALS = {"lj93": lj93, "colloid": colloid}


def active(kind, p):
    if kind == "lj93":
        return p["epsilon"] != 0.0 and p["r_cut"] != 0.0
    return p["A"] != 0.0 and p["a"] > 0.0 and p["r_cut"] != 0.0


def fold(kind, p, mode):
    """What a type's parameter row holds beside the coefficients: (r_cut, r_extrap, shift, V(e), F_e)."""
    if not active(kind, p):
        return 0.0, 0.0, 0.0, 0.0, 0.0
    c = float(p["r_cut"])
    e = float(p.get("r_extrap", 0.0))
    shift = POTENTIALS[kind](p, c)[0] if mode == "shift" else 0.0
    Ve, Fe = POTENTIALS[kind](p, e) if e > 0.0 else (0.0, 0.0)
    return c, e, shift, Ve, Fe


def wrap(pos, L, tilt=(0.0, 0.0, 0.0), periodic=(1, 1, 1)):
    """BoxDim::wrap for one shift per axis: tests/box_ref.py."""
    return box_ref.wrap(pos, None, L, tilt, periodic)[0]


def unit(v):
    v = [float(c) for c in v]
    n = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    return np.array([v[0] / n, v[1] / n, v[2] / n])


def distance(wall, x):
    """Signed distance d (N,) and unit vector u (N, 3) of the wrapped positions x."""
    o = np.asarray(wall.get("origin", (0.0, 0.0, 0.0)), dtype=np.float64)
    dx, dy, dz = x[:, 0] - o[0], x[:, 1] - o[1], x[:, 2] - o[2]
    if wall["kind"] == "plane":
        n = unit(wall["normal"])
        d = (n[0] * dx + n[1] * dy) + n[2] * dz
        return d, np.broadcast_to(n, x.shape).copy()
    if wall["kind"] == "cylinder":
        a = unit(wall["axis"])
        t = (dx * a[0] + dy * a[1]) + dz * a[2]
        dx, dy, dz = dx - t * a[0], dy - t * a[1], dz - t * a[2]
    elif wall["kind"] != "sphere":
        raise ValueError(wall["kind"])
    rho = np.sqrt((dx * dx + dy * dy) + dz * dz)
    s = np.stack([dx, dy, dz], axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        radial = np.where(rho[:, None] > 0.0, s / rho[:, None], 0.0)
    if wall.get("inside", True):
        return wall["radius"] - rho, -radial
    return rho - wall["radius"], radial


def evaluate(kind, walls, params, mode, pos, typeid, L, tilt=(0.0, 0.0, 0.0), periodic=(1, 1, 1)):
    """Per-wall forces (W, N, 3), energies (W, N) and distances (W, N); ``params`` is a list indexed by type id.
    The sums over the walls, in list order, are ``forces.sum`` taken wall by wall: see ``total``."""
    x = wrap(pos, L, tilt, periodic)
    typeid = np.asarray(typeid)
    N = x.shape[0]
    F = np.zeros((len(walls), N, 3))
    E = np.zeros((len(walls), N))
    D = np.zeros((len(walls), N))
    V = POTENTIALS[kind]
    for w, wall in enumerate(walls):
        d, u = distance(wall, x)
        D[w] = d
        for t, p in enumerate(params):
            c, e, shift, Ve, Fe = fold(kind, p, mode)
            mine = typeid == t
            linear = mine & (e > 0.0) & (d < e)
            standard = mine & ~linear & (d > 0.0) & (d < c)
            if standard.any():
                with np.errstate(all="ignore"):
                    v, f = V(p, d[standard])
                E[w, standard] = v - shift
                F[w, standard] = f[:, None] * u[standard]
            if linear.any():
                E[w, linear] = (Ve - shift) + Fe * (e - d[linear])
                F[w, linear] = Fe * u[linear]
    return F, E, D


def total(F, E):
    """Contributions of the walls added in list order."""
    f = np.zeros_like(F[0])
    e = np.zeros_like(E[0])
    for w in range(F.shape[0]):
        f = f + F[w]
        e = e + E[w]
    return f, e
