"""Seeded moves for the wrap tests (NumPy only; imports nothing of the project): the five boxes of
tests/test_gpu_box_wrap.py and, per box, start positions, displacements and start images built so that every shift
combination the box allows occurs, with no end point near a face. tests/test_box_ref.py checks these conditions on the
CPU for the seed below; the GPU tests assert them again on the reference of each kernel."""

import functools
import itertools
import zlib

import numpy as np

import box_ref

L678 = (6.0, 7.0, 8.0)
BOXES = {
    "tilt3": (L678, (0.5, 0.3, -0.4), (1, 1, 1)),
    "tilt_yz": (L678, (0.0, 0.0, 0.45), (1, 1, 1)),
    "tilt_xy_slab": (L678, (-0.35, 0.0, 0.0), (1, 1, 0)),
    "tilt3_open_y": (L678, (0.5, 0.3, -0.4), (1, 0, 1)),
    "ortho_open_xz": (L678, (0.0, 0.0, 0.0), (0, 1, 0)),
    # In the boxes above Lz yz and Lz xz are exact (Lz is a power of two), and so is Ly xy in all but tilt_xy_slab: an FMA
    # and a product followed by a sum then give the same bits, and the shifts cannot depend on how the compiler contracts.
    # Here all three products round.
    "tilt3_inexact": ((6.1, 7.3, 8.7), (0.5, 0.3, -0.4), (1, 1, 1)),
}
INEXACT = ("tilt_xy_slab", "tilt3_inexact")  # boxes in which a product of an edge and a tilt factor rounds
SEED = 20260119
N_LARGE, N_SMALL = 5000, 65
MAX_MOVE = 0.45        # of an edge, along each lattice direction
FACE_MARGIN = 1e-9     # fractional: no pre-wrap position may lie this close to a face plane
DRAW_MARGIN = 1e-6     # what the end points are drawn with
MIN_PER_COMBINATION = 20


def combinations(periodic):
    """The shift combinations (ix, iy, iz) a box with these flags allows: 27, 9 or 3."""
    return list(itertools.product(*[(-1, 0, 1) if p else (0,) for p in periodic]))


@functools.lru_cache(maxsize=None)
def moves(box_id, N=N_LARGE, seed=SEED):
    """dict(pos (N, 3) uniform in fractional coordinates, disp (N, 3) with |fractional| <= MAX_MOVE per lattice
    direction, image (N, 3) int32 in [-3, 3], mass (N,), force (N, 3), typeid (N,) in 0..2) -- the masses and forces as
    the thermostat and FIRE tests draw them. Along a periodic axis a particle that starts more than 0.06 from the centre
    crosses the face on its side two times out of three, except every eighth particle, which stays inside (rows that are
    not shifted at any N); every end point keeps DRAW_MARGIN from the faces."""
    L, tilt, periodic = BOXES[box_id]
    rng = np.random.default_rng([seed, N, zlib.crc32(box_id.encode())])
    f0 = rng.uniform(-0.5, 0.5, (N, 3))
    cross = rng.uniform(size=(N, 3)) < 2.0 / 3.0
    cross[::8] = False
    u = rng.uniform(size=(N, 3))
    f1 = np.empty_like(f0)
    m = DRAW_MARGIN
    for d in range(3):
        a = f0[:, d]
        if not periodic[d]:
            f1[:, d] = a + MAX_MOVE * (2.0 * u[:, d] - 1.0)
            continue
        up = cross[:, d] & (a > 0.06)
        dn = cross[:, d] & (a < -0.06)
        lo = np.where(up, 0.5 + m, np.where(dn, a - MAX_MOVE, np.maximum(-0.5 + m, a - MAX_MOVE)))
        hi = np.where(up, a + MAX_MOVE, np.where(dn, -0.5 - m, np.minimum(0.5 - m, a + MAX_MOVE)))
        f1[:, d] = lo + (hi - lo) * u[:, d]
    h = box_ref.box_matrix(L, tilt)
    out = dict(pos=f0 @ h.T, disp=(f1 - f0) @ h.T, image=rng.integers(-3, 4, (N, 3)).astype(np.int32),
               mass=rng.uniform(0.5, 2.0, N), force=rng.normal(0.0, 5.0, (N, 3)), typeid=rng.integers(0, 3, N))
    for v in out.values():
        v.setflags(write=False)
    return out


def face_distance(pos, L, tilt, periodic):
    """Smallest distance, in fractional coordinates, of any position from a face plane of a periodic axis."""
    f = box_ref.fractional(pos, L, tilt)[:, [d for d in range(3) if periodic[d]]]
    return float(np.minimum(np.abs(f - 0.5), np.abs(f + 0.5)).min())


def shift_counts(shift, periodic):
    """How often each allowed combination occurs among the rows of ``shift`` (N, 3); every row must be an allowed one."""
    counts = {c: 0 for c in combinations(periodic)}
    for row, n in zip(*np.unique(np.asarray(shift), axis=0, return_counts=True)):
        counts[tuple(int(v) for v in row)] += int(n)   # (KeyError: a shift the box does not allow)
    return counts
