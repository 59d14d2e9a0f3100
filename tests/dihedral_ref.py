"""Float64 NumPy reference for the dihedral potentials: a plain loop over the dihedrals with the formulas of
``include/azp.h`` ("dihedral forces"). Imports nothing of the project.

Members ``a, b, c, d``; ``b1 = r_b - r_a``, ``b2 = r_c - r_b``, ``b3 = r_d - r_c`` (minimum image); ``n1 = b1 x b2``,
``n2 = b2 x b3``; ``phi = atan2(|b2| (b1 . n2), n1 . n2)``. Periodic: ``U = 1/2 k (1 + d cos(n phi - phi0))``; OPLS:
``U = 1/2 [k1 (1 + cos phi) + k2 (1 - cos 2 phi) + k3 (1 + cos 3 phi) + k4 (1 - cos 4 phi)]``. ``F_m = -U' g_m`` with
``g_a = -(|b2| / |n1|^2) n1``, ``g_d = (|b2| / |n2|^2) n2``, ``g_b = -(1 + s) g_a + t g_d``,
``g_c = -(1 + t) g_d + s g_a``, ``s = b1 . b2 / |b2|^2``, ``t = b3 . b2 / |b2|^2``. Each member gets ``U / 4`` and the
virial ``1/4 ((-b1) (x) F_a + b2 (x) F_c + (b2 + b3) (x) F_d)`` (rows xx, xy, xz, yy, yz, zz)."""

import numpy as np


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


def separations(ra, rb, rc, rd, L, tilt=(0.0, 0.0, 0.0)):
    return (min_image(np.asarray(rb, dtype=np.float64) - ra, L, tilt), min_image(np.asarray(rc, dtype=np.float64) - rb, L, tilt),
            min_image(np.asarray(rd, dtype=np.float64) - rc, L, tilt))


def angle_of(b1, b2, b3):
    """phi in (-pi, pi], IUPAC: cis is 0, trans is pi."""
    n1, n2 = np.cross(b1, b2), np.cross(b2, b3)
    return float(np.arctan2(np.sqrt(b2 @ b2) * (b1 @ n2), n1 @ n2))


def potential(name, params, phi):
    """(U, U' = dU/dphi) of one dihedral."""
    if name == "Periodic":
        k, d, n, phi0 = float(params["k"]), float(params["d"]), float(params["n"]), float(params["phi0"])
        return 0.5 * k * (1.0 + d * np.cos(n * phi - phi0)), -0.5 * k * d * n * np.sin(n * phi - phi0)
    if name == "OPLS":
        k1, k2, k3, k4 = (float(params[key]) for key in ("k1", "k2", "k3", "k4"))
        U = 0.5 * (k1 * (1.0 + np.cos(phi)) + k2 * (1.0 - np.cos(2.0 * phi)) + k3 * (1.0 + np.cos(3.0 * phi))
                   + k4 * (1.0 - np.cos(4.0 * phi)))
        dU = 0.5 * (-k1 * np.sin(phi) + 2.0 * k2 * np.sin(2.0 * phi) - 3.0 * k3 * np.sin(3.0 * phi) + 4.0 * k4 * np.sin(4.0 * phi))
        return U, dU
    raise ValueError(name)


def one_dihedral(name, params, ra, rb, rc, rd, L, tilt=(0.0, 0.0, 0.0)):
    """U, (F_a, F_b, F_c, F_d), (b1, b2, b3), phi of one dihedral."""
    b1, b2, b3 = separations(ra, rb, rc, rd, L, tilt)
    n1, n2 = np.cross(b1, b2), np.cross(b2, b3)
    phi = angle_of(b1, b2, b3)
    U, dU = potential(name, params, phi)
    b2len = np.sqrt(b2 @ b2)
    ga = -(b2len / (n1 @ n1)) * n1
    gd = (b2len / (n2 @ n2)) * n2
    s, t = (b1 @ b2) / (b2 @ b2), (b3 @ b2) / (b2 @ b2)
    gb = -(1.0 + s) * ga + t * gd
    gc = -(1.0 + t) * gd + s * ga
    return U, (-dU * ga, -dU * gb, -dU * gc, -dU * gd), (b1, b2, b3), phi


_VIRIAL_ROWS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def evaluate(name, params, pos, dihedrals, typeid, L, tilt=(0.0, 0.0, 0.0)):
    """Loop over the dihedrals. ``params``: one dict per dihedral type. Returns a dict: ``energy`` (total), ``force``
    (n, 3), ``energies`` (n,) per-particle, ``virial`` (n, 6), and per dihedral ``U`` (m,), ``phi`` (m,), ``F``
    (m, 4, 3) = (F_a, F_b, F_c, F_d), ``b`` (m, 3, 3) = (b1, b2, b3), ``W`` (m, 6) the whole virial."""
    pos = np.asarray(pos, dtype=np.float64)[:, :3]
    dihedrals = np.asarray(dihedrals, dtype=np.int64).reshape(-1, 4)
    n, m = pos.shape[0], dihedrals.shape[0]
    force, energies, virial = np.zeros((n, 3)), np.zeros(n), np.zeros((n, 6))
    Us, phis, Fs, bs, Ws = np.zeros(m), np.zeros(m), np.zeros((m, 4, 3)), np.zeros((m, 3, 3)), np.zeros((m, 6))
    for j, (g, t) in enumerate(zip(dihedrals, np.asarray(typeid, dtype=np.int64))):
        U, F, (b1, b2, b3), phi = one_dihedral(name, params[t], pos[g[0]], pos[g[1]], pos[g[2]], pos[g[3]], L, tilt)
        W = np.outer(-b1, F[0]) + np.outer(b2, F[2]) + np.outer(b2 + b3, F[3])
        w6 = np.array([W[r, s] for r, s in _VIRIAL_ROWS])
        for i, Fm in zip(g, F):
            force[i] += Fm
            energies[i] += U / 4.0
            virial[i] += w6 / 4.0
        Us[j], phis[j], Fs[j], bs[j], Ws[j] = U, phi, F, (b1, b2, b3), w6
    return dict(energy=float(Us.sum()), force=force, energies=energies, virial=virial, U=Us, phi=phis, F=Fs, b=bs, W=Ws)


def energy_only(name, params, pos, dihedrals, typeid, L, tilt=(0.0, 0.0, 0.0)):
    """Total energy straight from ``atan2`` (no force code involved), for force-from-energy checks."""
    pos = np.asarray(pos, dtype=np.float64)[:, :3]
    E = 0.0
    for g, t in zip(np.asarray(dihedrals, dtype=np.int64).reshape(-1, 4), np.asarray(typeid, dtype=np.int64)):
        phi = angle_of(*separations(pos[g[0]], pos[g[1]], pos[g[2]], pos[g[3]], L, tilt))
        E += potential(name, params[t], phi)[0]
    return float(E)


# ---------------------------------------------------------------------------
# topologies the host and the GPU tests share
# ---------------------------------------------------------------------------
def chain_dihedrals(first, length):
    """The length - 3 dihedrals of a linear chain of consecutive indices."""
    return [(first + i, first + i + 1, first + i + 2, first + i + 3) for i in range(length - 3)]


def ring_dihedrals(i, j, k, l):
    """The four cyclic dihedrals of a 4-ring, all on the same four particles."""
    return [(i, j, k, l), (j, k, l, i), (k, l, i, j), (l, i, j, k)]


def branched_dihedrals(left, b, c, right):
    """Every dihedral (p, b, c, q) over the centre bond b-c, p a neighbour of b and q a neighbour of c: 9 for 3 + 3."""
    return [(p, b, c, q) for p in left for q in right]


def table_loop(dihedrals, typeid, n_local):
    """The per-particle dihedral table by a plain loop: ``entries[i]`` is the list of (other0, other1, other2,
    type | position << 30) of local particle ``i`` in dihedral order."""
    entries = [[] for _ in range(n_local)]
    for g, t in zip(dihedrals, typeid):
        for which, me in enumerate(g):
            if me < n_local:
                others = [int(x) for k, x in enumerate(g) if k != which]
                entries[me].append((others[0], others[1], others[2], int(t) | (which << 30)))
    return entries
