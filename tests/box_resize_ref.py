"""float64 numpy reference of ``azp_box_resize`` (csrc/box_resize.hip, include/azp.h) on tests/box_ref.py, and the seeded
cases of tests/test_box_resize.py and tests/test_gpu_box_resize.py.

The map: M comes from the host function the updater itself uses (``update.box_resize_matrix``), so the six numbers are
the kernel's; it is applied with plain products and sums (the kernel: nested FMAs). The wrap: a shift count per periodic
axis from the fractional coordinate in the new box -- z first, then y, then x, carrying the tilts as ``box_ref.wrap``
does, each shift a product and a difference (the kernel: one FMA) -- followed by ``box_ref.wrap``, which moves nothing
unless a row was left on a face.

A box is the tuple (L, tilt, periodic) of tests/box_cases.py."""

import functools
import zlib

import numpy as np

import box_ref

SEED = 20261019
FACE_MARGIN = 1e-9   # fractional: no reference end point may lie this close to a face of the new box
DRAW_MARGIN = 1e-6   # what the rows near a face are drawn with
NEAR = 1e-3          # "near a face"
PER_GROUP = 12       # rows per (axis, face, side of the face)
MIN_NEAR = 20

# (old box, new box): a cube into a smaller cuboid, an orthorhombic box sheared to xy = 0.4, a triply tilted box into
# another, and a slab whose z is not periodic
PAIRS = {
    "cube_to_cuboid": (((10.0, 10.0, 10.0), (0.0, 0.0, 0.0), (1, 1, 1)), ((9.5, 9.1, 8.7), (0.0, 0.0, 0.0), (1, 1, 1))),
    "ortho_to_xy": (((6.0, 7.0, 8.0), (0.0, 0.0, 0.0), (1, 1, 1)), ((6.0, 7.0, 8.0), (0.4, 0.0, 0.0), (1, 1, 1))),
    "tilt3_to_tilt3": (((6.1, 7.3, 8.7), (0.5, 0.3, -0.4), (1, 1, 1)), ((5.7, 7.9, 8.2), (0.35, -0.2, 0.45), (1, 1, 1))),
    "slab_open_z": (((6.0, 7.0, 8.0), (-0.35, 0.0, 0.0), (1, 1, 0)), ((5.5, 7.4, 6.9), (-0.2, 0.0, 0.0), (1, 1, 0))),
}
# for the type mask: boxes shrunk to 0.3 of their widths, so that a row that keeps its position needs up to two shifts
SHRUNK = {
    "cube_x0.3": (((12.0, 12.0, 12.0), (0.0, 0.0, 0.0), (1, 1, 1)), ((3.6, 3.6, 3.6), (0.0, 0.0, 0.0), (1, 1, 1))),
    "tilt3_x0.3": (((12.0, 13.0, 14.0), (0.5, 0.3, -0.4), (1, 1, 1)), ((3.6, 3.9, 4.2), (0.5, 0.3, -0.4), (1, 1, 1))),
    "slab_x0.3": (((12.0, 13.0, 14.0), (-0.35, 0.0, 0.0), (1, 1, 0)), ((3.6, 3.9, 4.2), (-0.35, 0.0, 0.0), (1, 1, 0))),
}
ALL_PAIRS = dict(PAIRS, **SHRUNK)
MASK = np.array([0, 1, 0], dtype=np.uint8)  # the Type filter of the tests: the middle one of three types


def as_box(box):
    """The ``state.Box`` of a (L, tilt, periodic) tuple."""
    from azplugins_amd.state import Box

    L, tilt, periodic = box
    return Box(L[0], L[1], L[2], *tilt, periodic=periodic)


def matrix(old, new):
    """M = H_new H_old^-1 as a (3, 3) array, from ``update.box_resize_matrix``: the numbers the kernel gets."""
    from azplugins_amd.update import box_resize_matrix

    m00, m01, m02, m11, m12, m22 = box_resize_matrix(as_box(old), as_box(new))
    return np.array([[m00, m01, m02], [0.0, m11, m12], [0.0, 0.0, m22]])


def affine(pos, M):
    """r' = M r with plain products and sums, in the order the formula is written."""
    x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
    return np.stack([M[0, 0] * x + M[0, 1] * y + M[0, 2] * z, M[1, 1] * y + M[1, 2] * z, M[2, 2] * z], axis=1)


def multi_wrap(pos, image, box):
    """Wrap rows that may lie several images outside ``box``. Returns (pos, image)."""
    (Lx, Ly, Lz), (xy, xz, yz), (px, py, pz) = box_ref._box(*box)
    pos = np.asarray(pos, dtype=np.float64)
    x, y, z = pos[:, 0].copy(), pos[:, 1].copy(), pos[:, 2].copy()
    shift = np.zeros(pos.shape, dtype=np.int64)
    if pz:
        k = np.rint(z / Lz)
        z -= k * Lz
        y -= k * (Lz * yz)
        x -= k * (Lz * xz)
        shift[:, 2] = k
    if py:
        k = np.rint((y - yz * z) / Ly)
        y -= k * Ly
        x -= k * (Ly * xy)
        shift[:, 1] = k
    if px:
        k = np.rint((x - xy * y - (xz - xy * yz) * z) / Lx)
        x -= k * Lx
        shift[:, 0] = k
    image = None if image is None else np.asarray(image) + shift.astype(np.asarray(image).dtype)
    return box_ref.wrap(np.stack([x, y, z], axis=1), image, *box)


def resize(pos, image, typeid, mask, old, new):
    """The reference of one ``azp_box_resize``: rows whose type is set in ``mask`` (None: all) are mapped with M, the
    others keep their positions, every row is wrapped into ``new``. Returns (pos, image, selected)."""
    pos = np.asarray(pos, dtype=np.float64)
    selected = np.ones(pos.shape[0], bool) if mask is None else np.asarray(mask)[np.asarray(typeid)].astype(bool)
    moved = np.where(selected[:, None], affine(pos, matrix(old, new)), pos)
    out, image = multi_wrap(moved, image, new)
    return out, image, selected


def face_distance(pos, box):
    """Smallest distance, in fractional coordinates, of any position from a face of a periodic axis of ``box``."""
    L, tilt, periodic = box
    f = box_ref.fractional(pos, L, tilt)[:, [d for d in range(3) if periodic[d]]]
    return float(np.minimum(np.abs(f - 0.5), np.abs(f + 0.5)).min()) if f.size else 1.0


def near_face_counts(pos, box):
    """{(axis, +1 / -1): rows within NEAR (fractional) of that face} for the periodic axes of ``box``."""
    L, tilt, periodic = box
    f = box_ref.fractional(pos, L, tilt)
    return {(d, s): int((np.abs(f[:, d] - 0.5 * s) < NEAR).sum()) for d in range(3) if periodic[d] for s in (1, -1)}


@functools.lru_cache(maxsize=None)
def case(pair_id, N, masked, seed=SEED):
    """dict(pos (N, 3), image (N, 3) int32 in [-3, 3], typeid (N,) in 0..2, vel (N, 4)), read-only.

    A row the resize selects is drawn by its fractional coordinates in the OLD box, uniform in [-0.499, 0.499]; a row it
    does not select (``masked``: types 0 and 2) by its fractional coordinates in the NEW box, uniform in [-1.6, 1.6] (the
    old box reaches to 0.5 / 0.3). The first rows are put next to a face along one periodic axis: PER_GROUP rows per axis,
    face and side, DRAW_MARGIN to NEAR from it -- a selected row just inside or just outside a face of the old box, an
    unselected one on either side of the new box's faces and of their images at +-1.5 -- so that, wrapped, at least
    2 PER_GROUP >= MIN_NEAR rows end next to each face (as many as fit when N is smaller)."""
    old, new = ALL_PAIRS[pair_id]
    rng = np.random.default_rng([seed, N, int(masked), zlib.crc32(pair_id.encode())])
    typeid = rng.integers(0, 3, N)
    selected = MASK[typeid].astype(bool) if masked else np.ones(N, bool)
    f = np.where(selected[:, None], rng.uniform(-0.499, 0.499, (N, 3)), rng.uniform(-1.6, 1.6, (N, 3)))
    groups = [(d, s, side) for d in range(3) if old[2][d] for s in (1, -1) for side in (1, -1)]
    u = rng.uniform(DRAW_MARGIN, NEAR, N)
    cell = rng.integers(-2, 2, N)  # the image of the new box an unselected row lies in: faces at cell + 0.5
    for j in range(min(N, PER_GROUP * len(groups))):
        d, s, side = groups[j % len(groups)]
        f[j, d] = s * (0.5 - side * u[j]) if selected[j] else (cell[j] + 0.5) - side * u[j]
    h_old, h_new = box_ref.box_matrix(old[0], old[1]), box_ref.box_matrix(new[0], new[1])
    pos = np.where(selected[:, None], f @ h_old.T, f @ h_new.T)
    out = dict(pos=pos, image=rng.integers(-3, 4, (N, 3)).astype(np.int32), typeid=typeid,
               vel=np.c_[rng.normal(0.0, 2.0, (N, 3)), rng.uniform(0.5, 2.0, N)])
    for v in out.values():
        v.setflags(write=False)
    return out
