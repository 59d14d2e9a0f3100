"""Float64 NumPy reference for the angle potentials: a plain loop over the angles with the formulas of
``include/azp.h`` ("angle forces"). Imports nothing of the project.

Members ``a, b, c`` with ``b`` the vertex; ``dab = r_a - r_b``, ``dcb = r_c - r_b`` (minimum image);
``c = dab.dcb / (|dab||dcb|)`` clamped to [-1, 1]; ``s = max(sqrt(1 - c^2), 1e-3)``;
Harmonic: ``U = 1/2 k (acos c - t0)^2``, ``g = -k (acos c - t0) / s``; CosineSquared: ``U = 1/2 k (c - cos t0)^2``,
``g = k (c - cos t0)``; ``F_a = -g (dcb / (|dab||dcb|) - c dab / |dab|^2)``, ``F_c`` with a and c exchanged,
``F_b = -F_a - F_c``. Each member gets ``U / 3`` and the virial ``1/3 (dab (x) F_a + dcb (x) F_c)``
(rows xx, xy, xz, yy, yz, zz)."""

import numpy as np

S_FLOOR = 1e-3


def box_matrix(L, tilt=(0.0, 0.0, 0.0)):
    """Columns are the lattice vectors of a HOOMD box (Lx, Ly, Lz, xy, xz, yz)."""
    Lx, Ly, Lz = (float(x) for x in L)
    xy, xz, yz = (float(x) for x in tilt)
    return np.array([[Lx, xy * Ly, xz * Lz], [0.0, Ly, yz * Lz], [0.0, 0.0, Lz]])


def min_image(d, L, tilt=(0.0, 0.0, 0.0)):
    """Minimum image of one separation, axis by axis from z down (HOOMD ``BoxDim::minImage``)."""
    d = np.array(d, dtype=np.float64)
    h = box_matrix(L, tilt)
    for k in (2, 1, 0):
        d -= h[:, k] * np.rint(d[k] / h[k, k])
    return d


def potential(name, params, c):
    """(U, g = dU/dc) of one angle with cosine ``c`` (already clamped)."""
    k, t0 = float(params["k"]), float(params["t0"])
    if name == "Harmonic":
        s = max(np.sqrt((1.0 - c) * (1.0 + c)), S_FLOOR)
        dth = np.arccos(c) - t0
        return 0.5 * k * dth * dth, -k * dth / s
    if name == "CosineSquared":
        dc = c - np.cos(t0)
        return 0.5 * k * dc * dc, k * dc
    raise ValueError(name)


def one_angle(name, params, ra, rb, rc, L, tilt=(0.0, 0.0, 0.0)):
    """U, F_a, F_b, F_c, dab, dcb of one angle."""
    dab = min_image(np.asarray(ra, dtype=np.float64) - rb, L, tilt)
    dcb = min_image(np.asarray(rc, dtype=np.float64) - rb, L, tilt)
    rab, rcb = np.sqrt(dab @ dab), np.sqrt(dcb @ dcb)
    c = min(max((dab @ dcb) / (rab * rcb), -1.0), 1.0)
    U, g = potential(name, params, c)
    Fa = -g * (dcb / (rab * rcb) - c * dab / (rab * rab))
    Fc = -g * (dab / (rab * rcb) - c * dcb / (rcb * rcb))
    return U, Fa, -Fa - Fc, Fc, dab, dcb


_VIRIAL_ROWS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def evaluate(name, params, pos, angles, typeid, L, tilt=(0.0, 0.0, 0.0)):
    """Loop over the angles. ``params``: one dict per angle type. Returns a dict: ``energy`` (total), ``force`` (n, 3),
    ``energies`` (n,) per-particle, ``virial`` (n, 6), and per angle ``U`` (m,), ``F`` (m, 3, 3) = (F_a, F_b, F_c),
    ``d`` (m, 2, 3) = (dab, dcb)."""
    pos = np.asarray(pos, dtype=np.float64)[:, :3]
    angles = np.asarray(angles, dtype=np.int64).reshape(-1, 3)
    n, m = pos.shape[0], angles.shape[0]
    force, energies, virial = np.zeros((n, 3)), np.zeros(n), np.zeros((n, 6))
    Us, Fs, ds = np.zeros(m), np.zeros((m, 3, 3)), np.zeros((m, 2, 3))
    for j, ((a, b, c), t) in enumerate(zip(angles, np.asarray(typeid, dtype=np.int64))):
        U, Fa, Fb, Fc, dab, dcb = one_angle(name, params[t], pos[a], pos[b], pos[c], L, tilt)
        W = (np.outer(dab, Fa) + np.outer(dcb, Fc)) / 3.0
        w6 = np.array([W[r, s] for r, s in _VIRIAL_ROWS])
        for i, F in ((a, Fa), (b, Fb), (c, Fc)):
            force[i] += F
            energies[i] += U / 3.0
            virial[i] += w6
        Us[j], Fs[j], ds[j] = U, (Fa, Fb, Fc), (dab, dcb)
    return dict(energy=float(Us.sum()), force=force, energies=energies, virial=virial, U=Us, F=Fs, d=ds)


def energy_only(name, params, pos, angles, typeid, L, tilt=(0.0, 0.0, 0.0)):
    """Total energy straight from ``acos`` (no force code involved), for force-from-energy checks."""
    pos = np.asarray(pos, dtype=np.float64)[:, :3]
    E = 0.0
    for (a, b, c), t in zip(np.asarray(angles, dtype=np.int64).reshape(-1, 3), np.asarray(typeid, dtype=np.int64)):
        dab = min_image(pos[a] - pos[b], L, tilt)
        dcb = min_image(pos[c] - pos[b], L, tilt)
        theta = np.arccos(min(max((dab @ dcb) / np.sqrt((dab @ dab) * (dcb @ dcb)), -1.0), 1.0))
        k, t0 = float(params[t]["k"]), float(params[t]["t0"])
        E += 0.5 * k * (theta - t0) ** 2 if name == "Harmonic" else 0.5 * k * (np.cos(theta) - np.cos(t0)) ** 2
    return E


# ---------------------------------------------------------------------------
# topologies the host and the GPU tests share
# ---------------------------------------------------------------------------
def chain_angles(first, length):
    """The length - 2 angles of a linear chain of consecutive indices."""
    return [(first + i, first + i + 1, first + i + 2) for i in range(length - 2)]


def triangle_angles(i, j, k):
    """Three angles on the same three particles, each particle the vertex once."""
    return [(i, j, k), (j, k, i), (k, i, j)]


def star_angles(centre, arms):
    """Every pair of arms with the centre as the vertex: 15 angles for 6 arms."""
    return [(arms[p], centre, arms[q]) for p in range(len(arms)) for q in range(p + 1, len(arms))]


def table_loop(angles, typeid, n_local):
    """The per-particle angle table by a plain loop: ``entries[i]`` is the list of (other0, other1, type, position)
    of local particle ``i`` in angle order."""
    entries = [[] for _ in range(n_local)]
    for (a, b, c), t in zip(angles, typeid):
        for me, others, which in ((a, (b, c), 0), (b, (a, c), 1), (c, (a, b), 2)):
            if me < n_local:
                entries[me].append((int(others[0]), int(others[1]), int(t), which))
    return entries
