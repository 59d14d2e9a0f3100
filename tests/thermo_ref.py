"""numpy / ``math.fsum`` restatement of the thermodynamic sums (``azp_thermo_sums``, include/azp.h) and of the
definitions of ``compute.ThermodynamicQuantities``: what the tests compare the kernel and the host function against.

``terms`` gives, for each of the 20 slots, the array of the terms the slot adds up (one entry per selected particle,
or per selected particle and force); ``exact`` their correctly rounded sum and the sum of their magnitudes. The
terms use the operation order the kernel documents (csrc/thermo.hip), so that the comparison measures the summation
and not the terms."""

import math

import numpy as np

NSUMS = 20
ORDER = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))  # xx, xy, xz, yy, yz, zz

# the error bound of a slot relative to the sum of the magnitudes of its terms: no term passes through more than 200
# additions (the depth is derived in csrc/azp_reduce.hpp: 86 up to N = 2^24, 182 up to 2^26 for thermo.hip's terms;
# each addition at most 2^-53 relative to the partial sum, which the sum of the magnitudes bounds), a few roundings
# inside each term, and slack
REL_BOUND = 256.0 * 2.0 ** -53


def terms(vel, select, forces=(), virials=(), orientation=None, angmom=None, inertia=None):
    """``vel`` (N, 4) with the mass in column 3; ``select`` boolean (N,); ``forces``: (N, 4) arrays; ``virials``: one
    (6, N) array or None per force; the rotational arrays all or none. Returns a list of 20 one-dimensional arrays."""
    vel = np.asarray(vel, dtype=np.float64)
    sel = np.asarray(select, dtype=bool)
    v = vel[sel, :3]
    m = vel[sel, 3]
    out = [np.zeros(0) for _ in range(NSUMS)]
    out[0] = np.ones(int(sel.sum()))
    p = m[:, None] * v
    for a in range(3):
        out[1 + a] = p[:, a]
    for c, (a, b) in enumerate(ORDER):
        out[4 + c] = p[:, a] * v[:, b]
    vir_terms = [[] for _ in range(6)]
    e_terms = []
    for k, f in enumerate(forces):
        e_terms.append(np.asarray(f, dtype=np.float64)[sel, 3])
        w = virials[k] if k < len(virials) else None
        if w is not None:
            for c in range(6):
                vir_terms[c].append(np.asarray(w, dtype=np.float64)[c, sel])
    for c in range(6):
        out[10 + c] = np.concatenate(vir_terms[c]) if vir_terms[c] else np.zeros(0)
    out[16] = np.concatenate(e_terms) if e_terms else np.zeros(0)
    if orientation is not None:
        q = np.asarray(orientation, dtype=np.float64)[sel]
        l = np.asarray(angmom, dtype=np.float64)[sel]
        I = np.asarray(inertia, dtype=np.float64)[sel]
        # vector part of conj(q) p / 2 (scalar parts first)
        s = np.stack([0.5 * ((q[:, 0] * l[:, 1] - l[:, 0] * q[:, 1]) - (q[:, 2] * l[:, 3] - q[:, 3] * l[:, 2])),
                      0.5 * ((q[:, 0] * l[:, 2] - l[:, 0] * q[:, 2]) - (q[:, 3] * l[:, 1] - q[:, 1] * l[:, 3])),
                      0.5 * ((q[:, 0] * l[:, 3] - l[:, 0] * q[:, 3]) - (q[:, 1] * l[:, 2] - q[:, 2] * l[:, 1]))], axis=1)
        nz = I != 0.0
        out[17] = 0.5 * (s[nz] * s[nz] / I[nz])
        out[18] = np.ones(int(nz.sum()))
    return out


def particle_terms(vel, select, forces=(), virials=(), orientation=None, angmom=None, inertia=None):
    """The arguments of ``terms``; returns the ``(20, N)`` array of what each particle adds to each slot in
    ``thermo_partial``, bit for bit: the virial and energy terms are added over the forces serially from ``0.0``, the
    rotational term over the axes serially, unselected rows are ``+0.0``. ``reduction_ref.tree_sum`` of it is the
    kernel's row."""
    vel = np.asarray(vel, dtype=np.float64)
    sel = np.asarray(select, dtype=bool)
    N = vel.shape[0]
    out = np.zeros((NSUMS, N))
    v, m = vel[:, :3], vel[:, 3]
    out[0] = 1.0
    p = m[:, None] * v
    for a in range(3):
        out[1 + a] = p[:, a]
    for c, (a, b) in enumerate(ORDER):
        out[4 + c] = p[:, a] * v[:, b]
    for k, f in enumerate(forces):
        out[16] = out[16] + np.asarray(f, dtype=np.float64)[:, 3]
        w = virials[k] if k < len(virials) else None
        if w is not None:
            for c in range(6):
                out[10 + c] = out[10 + c] + np.asarray(w, dtype=np.float64)[c]
    if orientation is not None:
        q = np.asarray(orientation, dtype=np.float64)
        l = np.asarray(angmom, dtype=np.float64)
        I = np.asarray(inertia, dtype=np.float64)
        s = np.stack([0.5 * ((q[:, 0] * l[:, 1] - l[:, 0] * q[:, 1]) - (q[:, 2] * l[:, 3] - q[:, 3] * l[:, 2])),
                      0.5 * ((q[:, 0] * l[:, 2] - l[:, 0] * q[:, 2]) - (q[:, 3] * l[:, 1] - q[:, 1] * l[:, 3])),
                      0.5 * ((q[:, 0] * l[:, 3] - l[:, 0] * q[:, 3]) - (q[:, 1] * l[:, 2] - q[:, 2] * l[:, 1]))], axis=1)
        for k in range(3):
            nz = I[:, k] != 0.0
            ke = 0.5 * (s[:, k] * s[:, k] / np.where(nz, I[:, k], 1.0))
            out[17] = out[17] + np.where(nz, ke, 0.0)
            out[18] = out[18] + np.where(nz, 1.0, 0.0)
    out[:, ~sel] = 0.0
    return out


def exact(term_arrays):
    """(correctly rounded sum, sum of magnitudes) of every slot."""
    sums = np.array([math.fsum(t.tolist()) for t in map(np.asarray, term_arrays)])
    mags = np.array([float(np.abs(t).sum()) for t in term_arrays])  # (a bound's scale: plain summation will do)
    return sums, mags


def quantities(sums, n_global, volume, conserves_momentum, rotational):
    """The definitions of the issue, restated on a row of sums."""
    s = np.asarray(sums, dtype=np.float64)
    n_g = s[0]
    K = s[4:10]
    W = s[10:16]
    tdof = 3 * n_g - (3 * n_g / n_global if conserves_momentum and n_global else 0.0)
    rdof = s[18] if rotational else 0.0
    ke_t = 0.5 * (K[0] + K[3] + K[5])
    ke = ke_t + (s[17] if rotational else 0.0)
    dof = tdof + rdof
    P = (K + W) / volume
    return dict(num_particles=int(n_g), volume=volume, translational_degrees_of_freedom=tdof, rotational_degrees_of_freedom=rdof,
                degrees_of_freedom=dof, translational_kinetic_energy=ke_t, rotational_kinetic_energy=s[17], kinetic_energy=ke,
                potential_energy=s[16], kinetic_temperature=(2 * ke / dof if dof > 0 else 0.0), pressure_tensor=tuple(P),
                pressure=(P[0] + P[3] + P[5]) / 3, linear_momentum=tuple(s[1:4]))
