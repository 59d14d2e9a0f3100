"""numpy reference for compute.MeanSquaredDisplacement and compute.SelfIntermediateScattering (tests/test_displacement.py,
tests/test_gpu_displacement.py): displacements, moments, the histogram of |d| and the self amplitudes in extended
precision, the kernel's own order of operations in float64 (for the tests that compare bits), and the error bounds.

A box is (L, tilt) = ((Lx, Ly, Lz), (xy, xz, yz)). Everything is indexed BY TAG: row j of every array is the particle with
tag j.

Displacement (include/azp.h): dn = n - n0 as integers, d = (r - r0) + H dn, H the lattice matrix of
``box_ref.box_matrix``. ``displacements`` evaluates that in np.longdouble (u_ld = 2^-64: exact for the purposes of a
bound in units of u = 2^-53); ``displacements_f64`` restates the kernel operation by operation.

THE BOUND OF THE MOMENTS. In float64 the kernel makes, for d_x,
    (x - x0) + ((Lx dn_x + h_xy dn_y) + h_xz dn_z),   h_xy = xy Ly and h_xz = xz Lz rounded on the host,
that is one rounding for the difference, one per product (three), one per rounded h (two), and one per addition (three):
nine roundings, each of a quantity that is at most
    A_x = |x - x0| + |Lx dn_x| + |h_xy dn_y| + |h_xz dn_z|
in magnitude, but not all of A_x each: the difference rounds |x - x0|, a product and its h round their own summand (at
most 2 u of it), the two inner additions round partial sums of the three shifts and the last addition rounds at most
A_x. Grouped by summand that is at most (1 + 1) u |x - x0| + (2 + 3) u |shifts|, so  |error of d_x| <= 6 u A_x  holds
with room (second-order terms included); d_y and d_z make fewer operations and are covered by the same count with
their own A. A is what the error is relative to, NOT |d|: a particle that crossed a face has r - r0 close to -H dn,
and the small d that is left carries the roundings of the large summands. The bound therefore takes the magnitude of
every term from A in place of |d| (A_a >= |d_a|):
    slot           term          roundings per term c_k                              magnitude M
    N_g            1             0 (integers below 2^53 add exactly)                 -
    S_a            d_a           6                                                   A_a
    S_ab           d_a d_b       6 + 6 (the factors) + 1 (the product) = 13          A_a A_b
    S_4            r2 r2         r2 = (d_x^2 + d_y^2) + d_z^2: each square 13, and two additions: at most 15 relative to
                                 R2 = A_x^2 + A_y^2 + A_z^2; the square of r2: 2 x 15 + 1 = 31     R2^2
and a term then passes through at most ``depth(N)`` additions of the reproducible sum (csrc/azp_reduce.hpp: no addition
ahead of the lane's accumulator, so per_lane + 6 + 3 + ceil(n_blocks / 64) + 6), each rounding a partial sum that is at
most sum_j M_j. In all
    bound_k = (c_k + depth) 2^-53 sum_j M_jk       over the particles of the group,
and per particle |d_a - reference| <= 6 2^-53 A_a for ``displacements``. Nothing here is fitted to what the kernel gives.

THE BOUND OF F_s is ``structure_factor_ref.bound`` with another argument constant. The term is exp(-2 pi i t),
t = fma(l, df_z, fma(k, df_y, h df_x)), df = f - f0 with both f from fractional(): each f is off by e_f u (e_f of
structure_factor_ref: its statement about fractional() is used, not restated), the subtraction rounds a number below 1
by at most u / 2 (counted as u), so df is off by (2 e_f + 1) u; |df| < 1 (not 1/2), so the three roundings of t round
partial sums of at most |m|_1: 3 |m|_1 u. The angle is off by 2 pi (2 e_f + 4) |m|_1 u, and with the prefactor 2^-52 = 2 u
    bound = N_G 2^-52 (c |m|_1 + c_trig + D),   c = pi (2 e_f + 4),
c_trig = 4 and D as there. c may not exceed 32, twice the cap of the static constant (asserted in ``fs_c_arg``)."""

import numpy as np

import box_ref
import reduction_ref
import structure_factor_ref as sref

assert np.finfo(np.longdouble).eps < 2.0 ** -60

LD = np.longdouble
U = 2.0 ** -53
NSUMS = 12
C_TERM = np.array([0.0, 6.0, 6.0, 6.0, 13.0, 13.0, 13.0, 13.0, 13.0, 13.0, 31.0])  # per-term roundings of slots 0 .. 10
C_DISPLACEMENT = 6.0
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))  # S_xx S_yy S_zz S_xy S_xz S_yz
EDGE_GUARD = 2.0 ** -40


def _h(box):
    (L, tilt) = box
    return box_ref.box_matrix(L, tilt)


def displacements(pos, image, pos0, image0, box):
    """d (N, 3) in np.longdouble: (r - r0) + H (n - n0), the images subtracted as integers."""
    dn = np.asarray(image, dtype=np.int64) - np.asarray(image0, dtype=np.int64)
    h = _h(box).astype(LD)
    return (np.asarray(pos, dtype=np.float64).astype(LD) - np.asarray(pos0, dtype=np.float64).astype(LD)) + dn.astype(LD) @ h.T


def magnitudes(pos, image, pos0, image0, box):
    """A (N, 3) float64: |r_a - r0_a| + sum_b |H_ab dn_b|, what the roundings of d_a are relative to."""
    dn = np.abs(np.asarray(image, dtype=np.int64) - np.asarray(image0, dtype=np.int64)).astype(np.float64)
    return np.abs(np.asarray(pos, dtype=np.float64) - np.asarray(pos0, dtype=np.float64)) + dn @ np.abs(_h(box)).T


def displacements_f64(pos, image, pos0, image0, box):
    """The kernel's operations in its order, in float64 (numpy contracts nothing)."""
    (Lx, Ly, Lz), (xy, xz, yz) = box
    hxy, hxz, hyz = xy * Ly, xz * Lz, yz * Lz
    pos, pos0 = np.asarray(pos, dtype=np.float64), np.asarray(pos0, dtype=np.float64)
    dn = (np.asarray(image, dtype=np.int64) - np.asarray(image0, dtype=np.int64)).astype(np.float64)
    dx = (pos[:, 0] - pos0[:, 0]) + ((Lx * dn[:, 0] + hxy * dn[:, 1]) + hxz * dn[:, 2])
    dy = (pos[:, 1] - pos0[:, 1]) + (Ly * dn[:, 1] + hyz * dn[:, 2])
    dz = (pos[:, 2] - pos0[:, 2]) + Lz * dn[:, 2]
    return np.stack([dx, dy, dz], axis=1)


def terms(d, member=None):
    """The eleven per-particle terms (11, N) of a (N, 3) array of displacements, in its dtype and in the kernel's order
    of operations; a particle outside the group adds +0.0."""
    d = np.asarray(d)
    one = np.ones(len(d), dtype=d.dtype)
    r2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    t = np.stack([one, d[:, 0], d[:, 1], d[:, 2]] + [d[:, a] * d[:, b] for a, b in PAIRS] + [r2 * r2])
    if member is not None:
        t = np.where(np.asarray(member, dtype=bool)[None, :], t, np.zeros((), dtype=d.dtype))
    return t


def moments(d, member=None):
    """The 12 doubles of the row (the pad included) from extended-precision displacements, rounded once at the end."""
    s = terms(np.asarray(d, dtype=LD), member).sum(axis=1)
    return np.concatenate([s.astype(np.float64), [0.0]])


def tree_moments(d64, member=None):
    """The 12 doubles as the kernel adds them: ``reduction_ref.tree_sum`` over the float64 terms in tag order."""
    return np.concatenate([reduction_ref.tree_sum(terms(np.asarray(d64, dtype=np.float64), member)), [0.0]])


def depth(N):
    """Addition depth of the moments: per_lane + 6 + 3 + ceil(n_blocks / 64) + 6."""
    per_lane, n_blocks = reduction_ref.shape(N)
    return per_lane + 6 + 3 + -(-n_blocks // 64) + 6


def moments_bound(A, member=None):
    """(c_k + depth) 2^-53 sum_j M_jk for the eleven live slots and 0 for the pad, (12,) float64."""
    A = np.asarray(A, dtype=np.float64)
    if member is not None:
        A = A[np.asarray(member, dtype=bool)]
    R2 = (A * A).sum(axis=1)
    M = np.array([0.0] + [A[:, a].sum() for a in range(3)] + [(A[:, a] * A[:, b]).sum() for a, b in PAIRS] + [(R2 * R2).sum()])
    # (N_g: exact, its magnitude is left at 0)
    return np.concatenate([(C_TERM + depth(max(len(A), 1))) * U * M, [0.0]])


def displacement_bound(A):
    """6 2^-53 A per component."""
    return C_DISPLACEMENT * U * np.asarray(A, dtype=np.float64)


def histogram(d, num_bins, r_max, member=None, exact=False):
    """(counts (num_bins,) int64, outside) of r = |d| in extended precision: r >= r_max is outside, else bin
    int(r num_bins / r_max). ASSERTS that the float64 kernel cannot land in another bin: no sample within relative 2^-40
    of a bin edge (r_max included). With ``exact`` a sample may sit ON an edge (every operation of the kernel is exact
    there, the square root of a perfect square included), but not near one."""
    d = np.asarray(d, dtype=LD)
    if member is not None:
        d = d[np.asarray(member, dtype=bool)]
    r = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    x = r * LD(num_bins) / LD(r_max)
    nearest = np.rint(x)
    off = np.abs(x - nearest)
    near = off <= EDGE_GUARD * np.maximum(nearest, LD(1))
    if exact:
        near &= off != 0
    else:
        near &= ~((nearest == 0) & (off == 0))  # (r == 0, a particle that did not move: bin 0 whatever the rounding)
    assert not near.any(), "a sample within 2^-40 of a bin edge: %r" % (np.asarray(x[near], dtype=np.float64),)
    inside = r < LD(r_max)
    k = np.minimum(np.floor(x[inside]).astype(np.int64), num_bins - 1)
    return np.bincount(k, minlength=num_bins).astype(np.int64), int((~inside).sum())


def self_amplitudes(pos, pos0, box, m, member=None):
    """rho_s(m) = sum_j exp(-2 pi i m . (f_j - f0_j)) over the group: (Re, Im) float64, rounded from extended-precision
    sums. m . df is reduced mod 1 before the trigonometry, as ``structure_factor_ref.amplitudes`` does."""
    df = sref.fractional(pos, box) - sref.fractional(pos0, box)
    if member is not None:
        df = df[np.asarray(member, dtype=bool)]
    m = np.asarray(m, dtype=np.int64).reshape(-1, 3)
    re, im = np.zeros(len(m), dtype=LD), np.zeros(len(m), dtype=LD)
    two_pi = 2 * np.arccos(LD(-1))
    for c0 in range(0, len(m), 256):
        t = df @ m[c0:c0 + 256].astype(LD).T
        t = t - np.rint(t)
        re[c0:c0 + 256] = np.cos(two_pi * t).sum(axis=0)
        im[c0:c0 + 256] = -np.sin(two_pi * t).sum(axis=0)
    return re.astype(np.float64), im.astype(np.float64)


def fs_c_arg(box):
    """pi (2 e_f + 4), e_f taken from structure_factor_ref.c_arg = pi (e_f + 1.5)."""
    e_f = sref.c_arg(box) / np.pi - 1.5
    c = np.pi * (2.0 * e_f + 4.0)
    assert c <= 32.0 and sref.C_TRIG <= 16.0  # (the cap the bound may not exceed)
    return c


def fs_bound(m, n_g, D, box):
    """N_G 2^-52 (c |m|_1 + c_trig + D) for every vector of ``m``."""
    m1 = np.abs(np.asarray(m, dtype=np.int64).reshape(-1, 3)).sum(axis=1).astype(np.float64)
    return float(n_g) * 2.0 ** -52 * (fs_c_arg(box) * m1 + sref.C_TRIG + float(D))
