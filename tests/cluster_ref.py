"""All-pairs reference for ``compute.Cluster`` (``azp_cluster_compute``): every pair in float64 through the
device's minimum image (the helper of tests/steinhardt_ref.py), ``rsq < r_max^2``, then
``scipy.sparse.csgraph.connected_components``. Keys are the smallest tag of a component, everything else follows from
keys and sizes. ``box`` is ``(L, tilt, periodic)``; ``member`` is an optional bool array that restricts the group
further (the solid particles of ``Cluster(solid=...)``)."""

import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components

import steinhardt_ref

NONE = 0xFFFFFFFF


def group(types, mask, member=None):
    g = steinhardt_ref._group(types, mask)
    return g if member is None else g & np.asarray(member, dtype=bool)


def _rsq(xyz, box):
    d = steinhardt_ref._separations(xyz, box)
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]


def edge_gap(xyz, types, box, mask, r_max, member=None, tol=1e-9):
    """Asserts that no pair of the group has |rsq - r_max^2| < tol and returns the smallest such distance."""
    g = group(types, mask, member)
    both = g[:, None] & g[None, :] & ~np.eye(g.shape[0], dtype=bool)
    gap = float(np.abs(_rsq(xyz, box)[both] - float(r_max) ** 2).min()) if both.any() else np.inf
    assert gap >= tol, "a pair sits %g from r_max^2" % gap
    return gap


def summary(keys, sizes, num_edges, size_bins):
    """The summary row from the per-row keys and sizes and the number of edges."""
    keys = np.asarray(keys, dtype=np.int64)
    sizes = np.asarray(sizes, dtype=np.int64)
    row = np.zeros(6 + size_bins, dtype=np.int64)
    inside = keys != NONE
    uniq, first = np.unique(keys[inside], return_index=True)
    csize = sizes[inside][first]
    row[0] = inside.sum()
    row[1] = uniq.shape[0]
    row[2] = csize.max() if uniq.size else 0
    row[3] = uniq[csize == csize.max()].min() if uniq.size else -1
    row[4] = (csize * csize).sum()
    row[5] = num_edges
    row[6:] = np.bincount(np.minimum(csize, size_bins) - 1, minlength=size_bins)
    return row


def indices(keys, sizes):
    """freud's numbering, written out: clusters sorted by descending size and then ascending key; -1 outside the group."""
    clusters = sorted({(int(k), int(s)) for k, s in zip(keys, sizes) if int(k) != NONE}, key=lambda c: (-c[1], c[0]))
    rank = {k: i for i, (k, _) in enumerate(clusters)}
    return np.array([rank.get(int(k), -1) for k in keys], dtype=np.int64)


def reference(xyz, types, box, mask, r_max, tags=None, member=None, size_bins=64):
    """Everything the device reports. Returns a dict: ``in_group`` (n,) bool, ``keys`` (n,) uint32, ``sizes`` (n,)
    uint32, ``num_edges``, ``num_clusters``, ``row`` (6 + size_bins,) int64 and ``idx`` (n,) int64."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    n = xyz.shape[0]
    tags = np.arange(n, dtype=np.int64) if tags is None else np.asarray(tags, dtype=np.int64)
    g = group(types, mask, member)
    adj = g[:, None] & g[None, :] & ~np.eye(n, dtype=bool) & (_rsq(xyz, box) < float(r_max) * float(r_max))
    assert np.array_equal(adj, adj.T)
    _, label = connected_components(csr_matrix(adj), directed=False)
    keys = np.full(n, NONE, dtype=np.int64)
    sizes = np.zeros(n, dtype=np.int64)
    for c in np.unique(label[g]):
        members = g & (label == c)
        keys[members] = tags[members].min()
        sizes[members] = members.sum()
    num_edges = int(adj.sum()) // 2
    return dict(in_group=g, keys=keys.astype(np.uint32), sizes=sizes.astype(np.uint32), num_edges=num_edges,
                num_clusters=int(np.unique(label[g]).shape[0]), row=summary(keys, sizes, num_edges, size_bins),
                idx=indices(keys, sizes))
