"""float64 numpy restatement of the box of csrc/azp_device.hpp (HOOMD BoxDim, centred on the origin, tilt factors xy, xz,
yz, per-axis periodic flags): ``wrap`` with one shift per axis in the branch structure of ``wrap_into_box``, the image
counters taken from the branch that was taken (``wrap_with_image`` reconstructs them; this does not), and the box matrix,
fractional coordinates and unwrapped positions that the tests build their reference-free checks on.

pos (N, 3), image (N, 3) int or None, L three edges (or one), tilt (xy, xz, yz), periodic three flags. Plain float64 in
the order the formulas are written: a tilted shift is a product and a sum here, one FMA in the kernels."""

import numpy as np


def _box(L, tilt, periodic):
    L = np.broadcast_to(np.asarray(L, dtype=np.float64), (3,))
    return [float(v) for v in L], [float(v) for v in tilt], [bool(p) for p in periodic]


def box_matrix(L, tilt=(0.0, 0.0, 0.0)):
    """The lattice vectors as columns: r = H f with f the fractional coordinates in [-0.5, 0.5)."""
    (Lx, Ly, Lz), (xy, xz, yz), _ = _box(L, tilt, (1, 1, 1))
    return np.array([[Lx, xy * Ly, xz * Lz], [0.0, Ly, yz * Lz], [0.0, 0.0, Lz]])


def fractional(pos, L, tilt=(0.0, 0.0, 0.0)):
    """Fractional coordinates (N, 3) by back substitution, 0 at the centre of the box."""
    (Lx, Ly, Lz), (xy, xz, yz), _ = _box(L, tilt, (1, 1, 1))
    pos = np.asarray(pos, dtype=np.float64)
    fz = pos[:, 2] / Lz
    fy = (pos[:, 1] - yz * pos[:, 2]) / Ly
    fx = (pos[:, 0] - xy * pos[:, 1] - (xz - xy * yz) * pos[:, 2]) / Lx
    return np.stack([fx, fy, fz], axis=1)


def unwrapped(pos, image, L, tilt=(0.0, 0.0, 0.0)):
    """pos + H image: the position the particle would have without periodic boundaries."""
    return np.asarray(pos, dtype=np.float64) + np.asarray(image, dtype=np.float64) @ box_matrix(L, tilt).T


def wrap(pos, image=None, L=(1.0, 1.0, 1.0), tilt=(0.0, 0.0, 0.0), periodic=(1, 1, 1)):
    """BoxDim::wrap for one shift per axis: z first (carrying Lz yz into y and Lz xz into x), then y against
    +-Ly / 2 + z yz (carrying Ly xy into x), then x against +-Lx / 2 + y xy + z (xz - xy yz). A non-periodic axis is not
    shifted; its tilt is still carried by the shifts of the others. Returns (pos, image), image None if None was given."""
    (Lx, Ly, Lz), (xy, xz, yz), (px, py, pz) = _box(L, tilt, periodic)
    pos = np.asarray(pos, dtype=np.float64)
    x, y, z = pos[:, 0].copy(), pos[:, 1].copy(), pos[:, 2].copy()
    shift = np.zeros(pos.shape, dtype=np.int64)
    if pz:
        h = 0.5 * Lz
        up, dn = z >= h, z < -h
        z[up] -= Lz
        z[dn] += Lz
        y[up] -= Lz * yz
        y[dn] += Lz * yz
        x[up] -= Lz * xz
        x[dn] += Lz * xz
        shift[:, 2] = up.astype(np.int64) - dn.astype(np.int64)
    if py:
        h, s = 0.5 * Ly, z * yz
        up, dn = y >= h + s, y < -h + s
        y[up] -= Ly
        y[dn] += Ly
        x[up] -= Ly * xy
        x[dn] += Ly * xy
        shift[:, 1] = up.astype(np.int64) - dn.astype(np.int64)
    if px:
        h, s = 0.5 * Lx, y * xy + z * (xz - xy * yz)
        up, dn = x >= h + s, x < -h + s
        x[up] -= Lx
        x[dn] += Lx
        shift[:, 0] = up.astype(np.int64) - dn.astype(np.int64)
    out = np.stack([x, y, z], axis=1)
    if image is None:
        return out, None
    image = np.asarray(image)
    return out, image + shift.astype(image.dtype)
