"""All-pairs numpy reference for ``compute.Steinhardt`` and ``compute.SolidLiquid`` (``azp_steinhardt_compute``,
DESIGN 4.28).

The spherical harmonics come from the recurrence the kernel runs (``csrc/steinhardt_device.hpp``), evaluated in
``np.longdouble`` (64 bits of mantissa here) with the kernel's own N_lm (``compute.steinhardt_norms``); they are pinned
against ``scipy.special.sph_harm_y`` in tests/test_steinhardt.py. The sums are left unrounded, so the device's
fixed-point words can be held against the exact value: 0.5 units of 2^-40 of quantisation per bond plus the kernel's
evaluation error.

``box`` is ``(L, tilt, periodic)`` as in tests/rdf_ref.py; the minimum image is the device's, in plain IEEE operations.
``edge_gap`` and ``threshold_gap`` assert a fixture's own conditions: no pair within rounding of r_max, no bond within
rounding of q_threshold, so that every integer the device reports has to be the reference's."""

import numpy as np

from azplugins_amd import compute

LD = np.longdouble
FIXED = LD(2) ** 40


def ylm(d, l):
    """Y_lm of the directions of ``d`` (n, 3) for the terms ``l``: longdouble (n, words) in the layout of the kernel's
    words (``compute.steinhardt_words``: Re at offset + 2 m, Im at offset + 2 m + 1), m >= 0 only. A zero vector
    gives zeros."""
    l = [int(x) for x in l]
    d = np.asarray(d, dtype=LD).reshape(-1, 3)
    r = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    zero = r == 0
    r = np.where(zero, LD(1), r)
    ux, uy, uz = d[:, 0] / r, d[:, 1] / r, d[:, 2] / r
    words, offsets = compute.steinhardt_words(l)
    norms = {x: [LD(v) for v in compute.steinhardt_norms(x)] for x in l}
    out = np.zeros((d.shape[0], words), dtype=LD)
    l_max = max(l)
    cm, sm = np.ones_like(ux), np.zeros_like(ux)
    qmm = LD(1)
    for m in range(l_max + 1):
        if m:
            cm, sm = cm * ux - sm * uy, cm * uy + sm * ux
            qmm = qmm * LD(-(2 * m - 1))
        ql, qprev = np.full_like(ux, qmm), np.zeros_like(ux)
        for x in range(m, l_max + 1):
            if x in l:
                off = offsets[l.index(x)] + 2 * m
                out[:, off] = norms[x][m] * ql * cm
                if m:
                    out[:, off + 1] = norms[x][m] * ql * sm
            if x == l_max:
                break
            ql, qprev = (LD(2 * x + 1) * uz * ql - LD(x + m) * qprev) / LD(x + 1 - m), ql
    out[zero] = 0
    return out


def ylm_complex(d, l, m):
    """Y_lm of one (l, m >= 0) as complex longdouble pairs (re, im) of the directions of ``d``."""
    w = ylm(d, [l])
    return w[:, 2 * m], w[:, 2 * m + 1]


def _separations(xyz, box):
    """(n, n, 3) float64: r_i - r_j through the device's minimum image (rint form, z then y then x)."""
    L, tilt, periodic = box
    L = [float(x) for x in L]
    xy, xz, yz = (float(t) for t in tilt)
    pos = np.asarray(xyz, dtype=np.float64)
    d = pos[:, None, :] - pos[None, :, :]
    x, y, z = d[..., 0].copy(), d[..., 1].copy(), d[..., 2].copy()
    if xy == 0.0 and xz == 0.0 and yz == 0.0:
        if periodic[2]:
            z = z - L[2] * np.rint(z * (1.0 / L[2]))
        if periodic[1]:
            y = y - L[1] * np.rint(y * (1.0 / L[1]))
        if periodic[0]:
            x = x - L[0] * np.rint(x * (1.0 / L[0]))
    else:
        if periodic[2]:
            img = np.rint(z * (1.0 / L[2]))
            z = z - L[2] * img
            y = y - L[2] * yz * img
            x = x - L[2] * xz * img
        if periodic[1]:
            img = np.rint(y * (1.0 / L[1]))
            y = y - L[1] * img
            x = x - L[1] * xy * img
        if periodic[0]:
            x = x - L[0] * np.rint(x * (1.0 / L[0]))
    return np.stack([x, y, z], axis=-1)


def _group(types, mask):
    types = np.asarray(types, dtype=np.int64)
    return np.ones(types.shape[0], dtype=bool) if mask is None else np.asarray(mask, dtype=bool)[types]


def _pairs(xyz, types, box, mask):
    in_g = _group(types, mask)
    d = _separations(xyz, box)
    rsq = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    both = in_g[:, None] & in_g[None, :] & ~np.eye(in_g.shape[0], dtype=bool)
    return in_g, d, rsq, both


def edge_gap(xyz, types, box, mask, r_max, tol=1e-9):
    """Asserts that no pair of the group has |rsq - r_max^2| < tol and returns the smallest such distance."""
    _, _, rsq, both = _pairs(xyz, types, box, mask)
    gap = float(np.abs(rsq[both] - float(r_max) ** 2).min()) if both.any() else np.inf
    assert gap >= tol, "a pair sits %g from r_max^2" % gap
    return gap


def _norm_sq(q, l, off):
    """sum over m = -l .. l of |q_lm|^2 from the stored m >= 0, added in the order m = 0, 1, ..."""
    acc = q[:, off] * q[:, off] + q[:, off + 1] * q[:, off + 1]
    for m in range(1, l + 1):
        acc = acc + 2 * (q[:, off + 2 * m] * q[:, off + 2 * m] + q[:, off + 2 * m + 1] * q[:, off + 2 * m + 1])
    return acc


def _ql(q, l):
    words, offsets = compute.steinhardt_words(l)
    return np.stack([np.sqrt(4 * LD(np.pi) / LD(2 * x + 1) * _norm_sq(q, x, off)) for x, off in zip(l, offsets)], axis=1)


def reference(xyz, types, box, mask, l, r_max, q_threshold=None):
    """Everything the device reports, from exact sums. Returns a dict:
    ``in_group`` (n,) bool, ``num_neighbors`` (n,) int64, ``S`` (n, words) longdouble = sum of Y_lm 2^40 over the bonds
    (unrounded), ``q`` (n, len(l)) float64, ``T`` (n, words) longdouble = sum over i and its neighbours of q_lm 2^40 (0
    outside the group), ``qbar`` (n, len(l)) float64; with ``q_threshold`` (one l): ``bonds`` = (i, j, d) of every
    bond with two non-zero norms and ``num_connections`` (n,) int64."""
    l = [int(x) for x in l]
    in_g, d, rsq, both = _pairs(xyz, types, box, mask)
    n = in_g.shape[0]
    acc = both & (rsq < float(r_max) * float(r_max))
    i_idx, j_idx = np.nonzero(acc)
    words = compute.steinhardt_words(l)[0]
    S = np.zeros((n, words), dtype=LD)
    if i_idx.size:
        np.add.at(S, i_idx, ylm(-d[i_idx, j_idx], l) * FIXED)  # the bond points from i to j
    nb = acc.sum(axis=1).astype(np.int64)
    denom = np.where(nb > 0, nb, 1).astype(LD)[:, None]
    qlm = np.where(nb[:, None] > 0, S / FIXED / denom, LD(0))
    T = np.zeros((n, words), dtype=LD)
    T[in_g] = qlm[in_g] * FIXED
    if i_idx.size:
        np.add.at(T, i_idx, qlm[j_idx] * FIXED)
    qbar_lm = T / FIXED / (nb + 1).astype(LD)[:, None]
    out = dict(in_group=in_g, num_neighbors=nb, S=S, q=_ql(qlm, l).astype(np.float64), T=T,
               qbar=_ql(qbar_lm, l).astype(np.float64))
    if q_threshold is not None:
        assert len(l) == 1
        norm = np.sqrt(_norm_sq(qlm, l[0], 0))
        ok = (norm[i_idx] > 0) & (norm[j_idx] > 0)
        bi, bj = i_idx[ok], j_idx[ok]
        qi, qj = qlm[bi], qlm[bj]
        dot = qi[:, 0] * qj[:, 0]
        for m in range(1, l[0] + 1):
            dot = dot + 2 * (qi[:, 2 * m] * qj[:, 2 * m] + qi[:, 2 * m + 1] * qj[:, 2 * m + 1])
        dval = (dot / (norm[bi] * norm[bj])).astype(np.float64)
        out["bonds"] = (bi, bj, dval)
        out["num_connections"] = np.bincount(bi[dval > float(q_threshold)], minlength=n).astype(np.int64)
    return out


def threshold_gap(ref, q_threshold, tol=1e-6):
    """Asserts that no bond of ``reference(..., q_threshold)`` has |d - q_threshold| < tol; returns the smallest."""
    dval = ref["bonds"][2]
    gap = float(np.abs(dval - float(q_threshold)).min()) if dval.size else np.inf
    assert gap >= tol, "a bond sits %g from q_threshold" % gap
    return gap


def summary(ref, l, num_bins, average=False, solid_threshold=None):
    """The summary row the device writes, from a ``reference``: exact for every word but the sums of q_l (words
    4 .. 4 + len(l)), which are llrint(q_l 2^40) of the reference's own q_l."""
    g = ref["in_group"]
    q = (ref["qbar"] if average else ref["q"])[g]
    nt = len(l)
    row = np.zeros(compute.steinhardt_summary_width(nt, num_bins), dtype=np.int64)
    nb = ref["num_neighbors"][g]
    row[0], row[1], row[2] = g.sum(), (nb > 0).sum(), nb.sum()
    for t in range(nt):
        row[4 + t] = np.rint(q[:, t].astype(LD) * FIXED).astype(np.int64).sum()
        k = np.minimum((q[:, t] * num_bins).astype(np.int64), num_bins - 1)
        row[4 + nt + t * num_bins: 4 + nt + (t + 1) * num_bins] = np.bincount(k, minlength=num_bins)
    if solid_threshold is not None:
        nc = ref["num_connections"][g]
        row[3] = (nc >= solid_threshold).sum()
        row[4 + nt + nt * num_bins:] = np.bincount(np.minimum(nc, 32), minlength=33)
    return row
