"""Two independent references for ``compute.ClusterProperties`` (``azp_cluster_properties``), both on the
keys and sizes of tests/cluster_ref.py. ``box`` is ``(L, tilt, periodic)``.

``by_edges``  unwraps each cluster by a breadth-first walk over its edges with the minimum-image separations of
              tests/steinhardt_ref.py, then takes the mean and the covariance of the unwrapped positions in float64. It is
              the truth for a compact cluster, and it defines ``compact``: the unwrapped cluster extends over less than
              half the box along every periodic lattice vector.
``by_formula`` is DESIGN 4.30 restated in float64: the circular mean of the fractional coordinates as the reference
              point, the offsets from it wrapped into [-1/2, 1/2], their moments.

Both return a dict keyed by the cluster's key: ``size``, ``center`` (3,), ``gyration`` (3, 3), ``rg2``, ``extent`` (3,),
``compact``; ``by_formula`` also ``resultant`` (3,: the length of (C, S) per axis, inf on a non-periodic one) and
``edge_gap`` (the smallest distance of a wrapped offset from +-1/2 over the periodic axes)."""

import numpy as np

import steinhardt_ref

NONE = 0xFFFFFFFF


def lattice(box):
    """H (columns: the lattice vectors) and the origin (the box's lower corner)."""
    L, tilt, _ = box
    xy, xz, yz = (float(t) for t in tilt)
    H = np.array([[L[0], xy * L[1], xz * L[2]], [0.0, L[1], yz * L[2]], [0.0, 0.0, L[2]]], dtype=np.float64)
    return H, -H @ np.full(3, 0.5)


def fractional(xyz, box):
    """s in [0, 1) for a wrapped particle, by the expressions of the tilted cell list."""
    L, tilt, _ = box
    xy, xz, yz = (float(t) for t in tilt)
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    fx = (x - xy * y - (xz - xy * yz) * z) * (1.0 / L[0])
    fy = (y - yz * z) * (1.0 / L[1])
    fz = z * (1.0 / L[2])
    return np.stack([fx, fy, fz], axis=1) + 0.5


def wrap_center(c, box):
    """A Cartesian point brought into the box on the periodic axes."""
    H, origin = lattice(box)
    s = np.linalg.solve(H, np.asarray(c, dtype=np.float64) - origin)
    per = np.asarray(box[2], dtype=bool)
    s[per] -= np.floor(s[per])
    return origin + H @ s


def center_distance(a, b, box):
    """|a - b| through the minimum image."""
    d = steinhardt_ref._separations(np.stack([np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)]), box)[0, 1]
    return float(np.sqrt((d * d).sum()))


def _members(keys):
    keys = np.asarray(keys).astype(np.int64)
    return {int(k): np.flatnonzero(keys == k) for k in np.unique(keys) if k != NONE}


def _entry(u, box):
    """Mean, covariance and fractional extents of unwrapped Cartesian positions u (n, 3)."""
    H, origin = lattice(box)
    per = np.asarray(box[2], dtype=bool)
    mean = u.mean(axis=0)
    d = u - mean
    G = d.T @ d / u.shape[0]
    f = np.linalg.solve(H, (u - origin).T).T
    extent = f.max(axis=0) - f.min(axis=0)
    return dict(size=int(u.shape[0]), center=wrap_center(mean, box), gyration=G, rg2=float(np.trace(G)), extent=extent,
                compact=bool(np.all(extent[per] < 0.5)))


def by_edges(xyz, box, keys, r_max):
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    out = {}
    for key, rows in _members(keys).items():
        sep = steinhardt_ref._separations(xyz[rows], box)  # sep[i, j] = r_i - r_j
        adj = (sep * sep).sum(axis=-1) < float(r_max) ** 2
        n = rows.shape[0]
        u = np.zeros((n, 3))
        seen = np.zeros(n, dtype=bool)
        seen[0] = True
        u[0] = xyz[rows[0]]
        queue = [0]
        while queue:
            i = queue.pop(0)
            for j in np.flatnonzero(adj[i] & ~seen):
                u[j] = u[i] - sep[i, j]
                seen[j] = True
                queue.append(int(j))
        assert seen.all(), "cluster %d is not connected at r_max = %g" % (key, r_max)
        out[key] = _entry(u, box)
    return out


def by_formula(xyz, box, keys):
    H, origin = lattice(box)
    per = np.asarray(box[2], dtype=bool)
    s = fractional(xyz, box)
    out = {}
    for key, rows in _members(keys).items():
        sk = s[rows]
        n = rows.shape[0]
        C = np.cos(2.0 * np.pi * sk).sum(axis=0)
        S = np.sin(2.0 * np.pi * sk).sum(axis=0)
        s0 = np.where(per, np.mod(np.arctan2(S, C) / (2.0 * np.pi), 1.0), 0.5)
        ds = sk - s0
        ds[:, per] -= np.rint(ds[:, per])
        m = ds.mean(axis=0)
        cov = ds.T @ ds / n - np.outer(m, m)
        c = s0 + m
        c[per] -= np.floor(c[per])
        G = H @ cov @ H.T
        extent = ds.max(axis=0) - ds.min(axis=0)
        gap = float((0.5 - np.abs(ds[:, per])).min()) if per.any() else np.inf
        out[key] = dict(size=n, center=origin + H @ c, gyration=G, rg2=float(np.trace(G)), extent=extent,
                        compact=bool(np.all(extent[per] < 0.5)), resultant=np.where(per, np.hypot(C, S), np.inf), edge_gap=gap)
    return out


def eligible(entry):
    """Whether ``by_formula`` pins a non-compact cluster's numbers: no member within 1e-9 of the wrap edge and, on every
    periodic axis, a resultant longer than 1e-6 n. Otherwise the device's rounding may take another image or another
    reference point, and the cluster is pinned by its flag and by reproducibility only."""
    return entry["edge_gap"] >= 1e-9 and bool(np.all(entry["resultant"] > 1e-6 * entry["size"]))
