"""float64 numpy restatement of the velocity-field semantics (the test reference for azplugins_amd.compute; not
product code): wrap into the box with one shift per axis (csrc/azp_device.hpp wrap_into_box, HOOMD BoxDim::wrap),
bin as floor(((x - lo) / (hi - lo)) * n) (src/BinningOperation.h), Cartesian momentum as it is or cylindrical
(z, theta = atan2(y, x) in [0, 2 pi), r; momentum rotated by (x / r, y / r)), ravel z + nz (y + ny x), then
momentum / mass per bin, 0 where the mass is 0."""

import numpy as np

import box_ref


def wrap(xyz, L, tilt=(0.0, 0.0, 0.0), periodic=(True, True, True)):
    return box_ref.wrap(xyz, None, L, tilt, periodic)[0]


def _bin_1d(x, lo, hi, n):
    f = np.floor(((x - lo) / (hi - lo)) * float(n))
    ok = (f >= 0.0) & (f < float(n))
    return np.where(ok, f, 0.0).astype(np.int64), ok


def bin_particles(xyz, mom, num_bins, lower, upper, cylindrical):
    """(raveled bin per particle, included mask, transformed momentum) of wrapped positions ``xyz``."""
    n = xyz.shape[0]
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    ok = np.ones(n, dtype=bool)
    b = [np.zeros(n, dtype=np.int64) for _ in range(3)]
    mom = np.array(mom, dtype=np.float64)
    if not cylindrical:
        coords = (x, y, z)
        for d in range(3):
            if num_bins[d] > 0:
                b[d], o = _bin_1d(coords[d], lower[d], upper[d], num_bins[d])
                ok &= o
    else:
        if num_bins[2] > 0:
            b[2], o = _bin_1d(z, lower[2], upper[2], num_bins[2])
            ok &= o
        if num_bins[1] > 0:
            theta = np.arctan2(y, x)
            theta = np.where(theta < 0.0, theta + 2.0 * np.pi, theta)
            b[1], o = _bin_1d(theta, lower[1], upper[1], num_bins[1])
            ok &= o
        r = np.sqrt(x * x + y * y)
        if num_bins[0] > 0:
            b[0], o = _bin_1d(r, lower[0], upper[0], num_bins[0])
            ok &= o
        safe = np.where(r > 0.0, r, 1.0)
        c = np.where(r > 0.0, x / safe, 1.0)
        s = np.where(r > 0.0, y / safe, 0.0)
        px, py = mom[:, 0].copy(), mom[:, 1].copy()
        mom[:, 0] = c * px + s * py
        mom[:, 1] = -s * px + c * py
    ny = num_bins[1] if num_bins[1] > 0 else 1
    nz = num_bins[2] if num_bins[2] > 0 else 1
    return b[2] + nz * (b[1] + ny * b[0]), ok, mom


def sums(pos, vel, mass, num_bins, lower=(0, 0, 0), upper=(0, 0, 0), cylindrical=False, L=(1, 1, 1), tilt=(0, 0, 0),
         periodic=(True, True, True), include=None):
    """Per-bin (mass, px, py, pz) sums (bins x 4) and the per-bin sum of |m v| (bins, for tolerances)."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    vel = np.asarray(vel, dtype=np.float64).reshape(-1, 3)
    mass = np.asarray(mass, dtype=np.float64).reshape(-1)
    n_bins = int(np.prod([k for k in num_bins if k > 0])) if any(k > 0 for k in num_bins) else 1
    out = np.zeros((n_bins, 4))
    scale = np.zeros(n_bins)
    if pos.shape[0] == 0:
        return out, scale
    xyz = wrap(pos, L, tilt, periodic)
    mom = vel * mass[:, None]
    idx, ok, tmom = bin_particles(xyz, mom, num_bins, lower, upper, cylindrical)
    if include is not None:
        ok &= np.asarray(include, dtype=bool)
    idx, m, tmom = idx[ok], mass[ok], tmom[ok]
    np.add.at(out[:, 0], idx, m)
    for k in range(3):
        np.add.at(out[:, 1 + k], idx, tmom[:, k])
    np.add.at(scale, idx, np.abs(tmom).sum(axis=1) + np.abs(m))
    return out, scale


def normalize(s):
    v = np.zeros((s.shape[0], 3))
    m = s[:, 0]
    pos = m > 0.0
    v[pos] = s[pos, 1:] / m[pos, None]
    return v


def velocities(*args, **kwargs):
    """Mass-averaged velocity per bin (bins x 3)."""
    return normalize(sums(*args, **kwargs)[0])


def compact_shape(num_bins):
    return tuple(k for k in num_bins if k > 0) + (3,)
