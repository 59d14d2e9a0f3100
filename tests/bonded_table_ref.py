"""Float64 NumPy reference for the tabulated angle and dihedral potentials: the definitions of ``include/azp.h``
("tabulated angle and dihedral potentials") restated as plain loops. The minimum image, the dihedral angle and the
virial rows come from ``angle_ref`` / ``dihedral_ref`` by import; nothing of the project is imported.

A table is ``dict(U=array, tau=array)`` with ``width = len(U) >= 2`` samples on ``n = width - 1`` equal intervals, both
end points stored, ``tau = -dU/d(angle)``:

* angle: knots ``theta_k = k pi / n``; ``theta = acos(c)``, index ``theta * (n / pi)``; ``g = dU/dc = tau / s`` with
  ``s = max(sqrt((1 - c)(1 + c)), 1e-3)``;
* dihedral: knots ``phi_k = -pi + 2 pi k / n``; ``phi = atan2(...)``, index ``(phi + pi) * (n / (2 pi))``;
  ``U' = dU/dphi = -tau``. ``phi = +pi`` reads the last knot, ``phi = -pi`` the first.

Between the knots: ``k = min(int(index), n - 1)``, ``f = index - k``, ``U = U_k + f (U_{k+1} - U_k)``, ``tau`` likewise."""

import math

import numpy as np

import angle_ref
import dihedral_ref

S_FLOOR = angle_ref.S_FLOOR


def angle_knots(width):
    return np.arange(width) * (math.pi / (width - 1))


def dihedral_knots(width):
    return -math.pi + np.arange(width) * (2.0 * math.pi / (width - 1))


def sample(kind, width, U, tau):
    """``dict(U, tau)`` of ``width`` samples of the functions ``U(x)`` and ``tau(x)`` at the knots of ``kind``."""
    x = angle_knots(width) if kind == "angle" else dihedral_knots(width)
    return dict(U=np.array([U(v) for v in x], dtype=np.float64), tau=np.array([tau(v) for v in x], dtype=np.float64))


def interpolate(table, index):
    """(U, tau) at the index coordinate ``index`` in [0, n]."""
    U, tau = np.asarray(table["U"], dtype=np.float64), np.asarray(table["tau"], dtype=np.float64)
    n = len(U) - 1
    k = min(int(index), n - 1)
    f = index - k
    return U[k] + f * (U[k + 1] - U[k]), tau[k] + f * (tau[k + 1] - tau[k])


def angle_table(table, theta):
    """(U, tau) of an angle table at ``theta`` in [0, pi]."""
    n = len(table["U"]) - 1
    return interpolate(table, theta * (n / math.pi))


def dihedral_table(table, phi):
    """(U, tau) of a dihedral table at ``phi`` in [-pi, pi]."""
    n = len(table["U"]) - 1
    return interpolate(table, (phi + math.pi) * (n / (2.0 * math.pi)))


def _accumulate(out, members, forces, U, W):
    w6 = np.array([W[r, s] for r, s in angle_ref._VIRIAL_ROWS]) / len(members)
    for i, F in zip(members, forces):
        out["force"][i] += F
        out["energies"][i] += U / len(members)
        out["virial"][i] += w6


def _empty(n, m):
    return dict(force=np.zeros((n, 3)), energies=np.zeros(n), virial=np.zeros((n, 6)), U=np.zeros(m), x=np.zeros(m))


def evaluate_angles(tables, pos, angles, typeid, L, tilt=(0.0, 0.0, 0.0)):
    """Loop over the angles; ``tables``: one table per angle type. Returns ``energy``, ``force`` (n, 3), ``energies``
    (n,), ``virial`` (n, 6) and per angle ``U`` and ``x`` = theta."""
    pos = np.asarray(pos, dtype=np.float64)[:, :3]
    angles = np.asarray(angles, dtype=np.int64).reshape(-1, 3)
    out = _empty(pos.shape[0], angles.shape[0])
    for j, ((a, b, c), t) in enumerate(zip(angles, np.asarray(typeid, dtype=np.int64))):
        dab = angle_ref.min_image(pos[a] - pos[b], L, tilt)
        dcb = angle_ref.min_image(pos[c] - pos[b], L, tilt)
        rab, rcb = np.sqrt(dab @ dab), np.sqrt(dcb @ dcb)
        cos = min(max((dab @ dcb) / (rab * rcb), -1.0), 1.0)
        s = max(np.sqrt((1.0 - cos) * (1.0 + cos)), S_FLOOR)
        theta = np.arccos(cos)
        U, tau = angle_table(tables[t], theta)
        g = tau / s
        Fa = -g * (dcb / (rab * rcb) - cos * dab / (rab * rab))
        Fc = -g * (dab / (rab * rcb) - cos * dcb / (rcb * rcb))
        _accumulate(out, (a, b, c), (Fa, -Fa - Fc, Fc), U, np.outer(dab, Fa) + np.outer(dcb, Fc))
        out["U"][j], out["x"][j] = U, theta
    out["energy"] = float(out["U"].sum())
    return out


def evaluate_dihedrals(tables, pos, dihedrals, typeid, L, tilt=(0.0, 0.0, 0.0)):
    """Loop over the dihedrals; ``tables``: one table per dihedral type. Returns what ``evaluate_angles`` returns, with
    ``x`` = phi."""
    pos = np.asarray(pos, dtype=np.float64)[:, :3]
    dihedrals = np.asarray(dihedrals, dtype=np.int64).reshape(-1, 4)
    out = _empty(pos.shape[0], dihedrals.shape[0])
    for j, (g, t) in enumerate(zip(dihedrals, np.asarray(typeid, dtype=np.int64))):
        b1, b2, b3 = dihedral_ref.separations(pos[g[0]], pos[g[1]], pos[g[2]], pos[g[3]], L, tilt)
        phi = dihedral_ref.angle_of(b1, b2, b3)
        U, tau = dihedral_table(tables[t], phi)
        n1, n2 = np.cross(b1, b2), np.cross(b2, b3)
        b2len = np.sqrt(b2 @ b2)
        ga = -(b2len / (n1 @ n1)) * n1
        gd = (b2len / (n2 @ n2)) * n2
        s12, s32 = (b1 @ b2) / (b2 @ b2), (b3 @ b2) / (b2 @ b2)
        gb = -(1.0 + s12) * ga + s32 * gd
        gc = -(1.0 + s32) * gd + s12 * ga
        F = (tau * ga, tau * gb, tau * gc, tau * gd)   # F_m = -U' g_m = tau g_m
        _accumulate(out, g, F, U, np.outer(-b1, F[0]) + np.outer(b2, F[2]) + np.outer(b2 + b3, F[3]))
        out["U"][j], out["x"][j] = U, phi
    out["energy"] = float(out["U"].sum())
    return out
