"""All-pairs numpy reference for the pair counts of ``compute.RadialDistributionFunction`` (``azp_rdf_counts``).

``box`` is ``(L, tilt, periodic)``: three lengths, the tilt factors (xy, xz, yz) and three flags. The minimum image is
the device's (``min_image`` of ``csrc/azp_device.hpp``: the rint form, z then y then x), in plain IEEE operations: the
device contracts some of them into FMAs, so a distance can differ from the one here in its last bits. ``edge_pairs``
counts the pairs for which that could change a bin; a fixture with none has the same integer counts under either
rounding."""

import numpy as np

CHUNK = 512


def _distances(pos, rows, box):
    """r^2 (len(rows), n_total) of the minimum-image separations r_i - r_j."""
    L, tilt, periodic = box
    L = [float(x) for x in L]
    xy, xz, yz = (float(t) for t in tilt)
    d = pos[rows, None, :3] - pos[None, :, :3]
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
    return x * x + y * y + z * z


def _groups(types, mask_a, mask_b, n_own):
    types = np.asarray(types, dtype=np.int64)
    n_total = types.shape[0]
    in_a = np.ones(n_total, dtype=bool) if mask_a is None else np.asarray(mask_a, dtype=bool)[types]
    in_b = np.ones(n_total, dtype=bool) if mask_b is None else np.asarray(mask_b, dtype=bool)[types]
    in_a = in_a & (np.arange(n_total) < n_own)
    return in_a, in_b


def counts(pos, types, box, mask_a, mask_b, r_max, num_bins, n_own=None):
    """The row of ``azp_rdf_counts`` as int64 (num_bins + 4,): ordered pairs (i in A below ``n_own``, j in B, i != j) with
    r^2 < r_max^2 in bin min(int(sqrt(r^2) * (num_bins / r_max)), num_bins - 1), then N_A, N_B, N_AB over the rows below
    ``n_own`` (default: all rows), then 0. ``mask_a`` / ``mask_b``: one flag per type, or None for every particle."""
    pos = np.asarray(pos, dtype=np.float64)
    n_total = pos.shape[0]
    n_own = n_total if n_own is None else int(n_own)
    in_a, in_b = _groups(types, mask_a, mask_b, n_own)
    scale = num_bins / float(r_max)
    rmaxsq = float(r_max) * float(r_max)
    out = np.zeros(num_bins + 4, dtype=np.int64)
    rows_a = np.nonzero(in_a)[0]
    for c0 in range(0, rows_a.size, CHUNK):
        rows = rows_a[c0:c0 + CHUNK]
        rsq = _distances(pos, rows, box)
        ok = (rsq < rmaxsq) & in_b[None, :] & (rows[:, None] != np.arange(n_total)[None, :])
        k = np.minimum((np.sqrt(rsq[ok]) * scale).astype(np.int64), num_bins - 1)
        out[:num_bins] += np.bincount(k, minlength=num_bins)
    own = np.arange(n_total) < n_own
    out[num_bins] = np.count_nonzero(in_a)
    out[num_bins + 1] = np.count_nonzero(in_b & own)
    out[num_bins + 2] = np.count_nonzero(in_a & in_b)
    return out


def edge_pairs(pos, types, box, mask_a, mask_b, r_max, num_bins, n_own=None, tol=1e-11):
    """Number of counted or nearly counted pairs whose bin could depend on the last bits of the distance: r * scale
    within ``tol`` of an integer, or r within ``tol * r_max`` of r_max."""
    pos = np.asarray(pos, dtype=np.float64)
    n_total = pos.shape[0]
    n_own = n_total if n_own is None else int(n_own)
    in_a, in_b = _groups(types, mask_a, mask_b, n_own)
    scale = num_bins / float(r_max)
    reach = (float(r_max) * (1.0 + 2.0 * tol)) ** 2
    n = 0
    rows_a = np.nonzero(in_a)[0]
    for c0 in range(0, rows_a.size, CHUNK):
        rows = rows_a[c0:c0 + CHUNK]
        rsq = _distances(pos, rows, box)
        ok = (rsq < reach) & in_b[None, :] & (rows[:, None] != np.arange(n_total)[None, :])
        r = np.sqrt(rsq[ok])
        s = r * scale
        n += int(np.count_nonzero((np.abs(s - np.rint(s)) <= tol) | (np.abs(r - r_max) <= tol * r_max)))
    return n
