"""float64 numpy restatement of csrc/thermo_field.hip (compute.ThermodynamicField): the bin of a particle
(csrc/field_bin.hpp), the 18 terms per particle and the 64-ary butterfly tree that sums the members of a bin in tag
order. Every operation is the plain IEEE operation of the kernels in their order, so ``row`` reproduces every word of
the kernels' row bit for bit -- where ``atan2`` of the host agrees with the device's, which the tests arrange by
keeping particles an ulp away from the theta edges.

Positions are expected INSIDE the box (the kernels wrap them first; ``box_ref.wrap`` restates that up to the FMA of a
tilted shift)."""

import math

import numpy as np

NSUMS = 18
WAVE = 64
CARTESIAN, CYLINDRICAL = 0, 1
U = 2.0**-53


def bin_1d(x, lo, hi, n):
    """floor(((x - lo) / (hi - lo)) * n), -1 outside [0, n)."""
    f = np.floor(((x - lo) / (hi - lo)) * float(n))
    ok = (f >= 0.0) & (f < float(n))
    return np.where(ok, f, -1.0).astype(np.int64)


def bins(xyz, coordinates, num_bins, lower, upper):
    """Raveled bin of every particle, -1 outside the grid: z + nz (y + ny x) with a dimension that is not binned counting
    as size 1; cylindrical: (r, theta, z), theta = atan2(y, x) in [0, 2 pi)."""
    xyz = np.asarray(xyz, dtype=np.float64)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if coordinates == CYLINDRICAL:
        theta = np.arctan2(y, x)
        theta = np.where(theta < 0.0, theta + 2.0 * math.pi, theta)
        coords = (np.sqrt(x * x + y * y), theta, z)
    else:
        coords = (x, y, z)
    ok = np.ones(len(xyz), dtype=bool)
    b = []
    for d in range(3):
        if num_bins[d] > 0:
            k = bin_1d(coords[d], lower[d], upper[d], num_bins[d])
            ok &= k >= 0
            b.append(k)
        else:
            b.append(np.zeros(len(xyz), dtype=np.int64))
    ny, nz = max(num_bins[1], 1), max(num_bins[2], 1)
    return np.where(ok, b[2] + nz * (b[1] + ny * b[0]), -1)


def terms(vel, forces=(), virials=()):
    """(N, 18) terms: 1, m, m v_a, (m v_a) v_b (xx, xy, xz, yy, yz, zz), the virials of the forces added in their order
    starting from +0.0 (``virials[f]``: (6, N) or None), the energies (``forces[f][:, 3]``) likewise."""
    vel = np.asarray(vel, dtype=np.float64)
    n = vel.shape[0]
    m = vel[:, 3]
    px, py, pz = m * vel[:, 0], m * vel[:, 1], m * vel[:, 2]
    t = np.zeros((n, NSUMS))
    t[:, 0] = 1.0
    t[:, 1] = m
    t[:, 2], t[:, 3], t[:, 4] = px, py, pz
    t[:, 5], t[:, 6], t[:, 7] = px * vel[:, 0], px * vel[:, 1], px * vel[:, 2]
    t[:, 8], t[:, 9], t[:, 10] = py * vel[:, 1], py * vel[:, 2], pz * vel[:, 2]
    for f, force in enumerate(forces):
        t[:, 17] = t[:, 17] + np.asarray(force, dtype=np.float64)[:, 3]
        vir = virials[f] if f < len(virials) else None
        if vir is not None:
            t[:, 11:17] = t[:, 11:17] + np.asarray(vir, dtype=np.float64).T
    return t


def levels(n):
    """Levels of the tree over n members: ceil(log64 n), at least 1."""
    lv, reach = 1, WAVE
    while reach < n:
        lv, reach = lv + 1, reach * WAVE
    return lv


def _butterfly(v):
    """``group_sum<64>`` over axis 1 (64 lanes): the balanced pairwise sum; its DPP and permute steps pair lane ``l`` with
    ``l ^ s`` (or with a lane that holds the same value), and IEEE addition is commutative."""
    lanes = np.arange(WAVE)
    for s in (1, 2, 4, 8, 16, 32):
        v = v + v[:, lanes ^ s]
    return v[:, 0]


def tree(values):
    """Sum over axis 0 of (n, k) float64 in the kernels' order: pad with +0.0 to a multiple of 64, replace every run of
    64 by its butterfly, repeat until one value remains. n = 0: +0.0."""
    v = np.asarray(values, dtype=np.float64)
    if v.ndim == 1:
        return tree(v[:, None])[0]
    if v.shape[0] == 0:
        return np.zeros(v.shape[1])
    while True:
        n = v.shape[0]
        runs = (n + WAVE - 1) // WAVE
        padded = np.zeros((runs * WAVE,) + v.shape[1:])
        padded[:n] = v
        v = _butterfly(padded.reshape((runs, WAVE) + v.shape[1:]))
        if runs == 1:
            return v[0]


def row(bin_of, tags, member, t, types, ntypes, n_bins):
    """The kernels' row, (n_bins, 18 + ntypes): ``bin_of`` (-1: outside), ``tags`` and ``types`` per particle, ``member``
    the filter's selection (None: all), ``t`` the (N, 18) terms."""
    bin_of = np.asarray(bin_of)
    sel = bin_of >= 0
    if member is not None:
        sel &= np.asarray(member, dtype=bool)
    out = np.zeros((n_bins, NSUMS + ntypes))
    idx = np.nonzero(sel)[0]
    idx = idx[np.lexsort((np.asarray(tags)[idx], bin_of[idx]))]
    b = bin_of[idx]
    starts = np.nonzero(np.r_[True, b[1:] != b[:-1]])[0] if len(idx) else np.zeros(0, dtype=np.int64)
    ends = np.r_[starts[1:], len(idx)]
    types = np.asarray(types)
    for s, e in zip(starts, ends):
        rows = idx[s:e]
        out[b[s], :NSUMS] = tree(t[rows])
        ty = types[rows]
        out[b[s], NSUMS:] = np.bincount(ty[(ty >= 0) & (ty < ntypes)], minlength=ntypes)
    return out


def bound(abs_terms_sum, n, n_forces):
    """|tree - exact| <= (6 L + F + 1) 2^-53 sum|term|: a term passes 6 additions per level of the tree, F across the
    forces, and one more covers the rounding of the bound's own evaluation."""
    return (6 * levels(n) + n_forces + 1) * U * abs_terms_sum
