"""compute.PressureProfile in numpy and Python integers: the definition of include/azp.h ("pressure profile") restated.

All pairs O(N^2). A pair (i, j) is taken once, with i the member with the smaller tag; d = minimum image of r_i - r_j in
the arithmetic of azp_device.hpp's min_image (exact for the dyadic coordinates and box lengths the tests use),
rsq = d.x d.x + d.y d.y + d.z d.z without contraction. force_divr comes from the CPU oracle's evaluators (rsq handed over
as it is, not through a square root), from closed forms (special-pair LJ) or from table_ref (tabulated potentials);
XPLOR is HOOMD's smoothing around the oracle's unsmoothed pair. The weights follow the header's expressions operation
by operation in IEEE doubles; a term goes through ONE round-half-even conversion to a Python integer in units of
2^-shift, so the sums are exact.

`profile` returns the integer row (6 bins + 4 words) and, per bin and component, the sum of the |terms| and their number:
what the tolerance of the GPU tests is made of."""

import ctypes as C
import math

import numpy as np

import table_ref as TR

U_ROUND = 2.0 ** -53


# ---------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------
def min_image(d, L, tilt=(0.0, 0.0, 0.0), periodic=(True, True, True)):
    """min_image of azp_device.hpp on an (..., 3) array (z, then y, then x; a tilted box shifts the lower axes along)."""
    d = np.array(d, dtype=np.float64)
    xy, xz, yz = tilt
    if xy == 0.0 and xz == 0.0 and yz == 0.0:
        for k in (2, 1, 0):
            if periodic[k]:
                d[..., k] = d[..., k] - L[k] * np.rint(d[..., k] * (1.0 / L[k]))
        return d
    if periodic[2]:
        img = np.rint(d[..., 2] * (1.0 / L[2]))
        d[..., 2] = d[..., 2] - L[2] * img
        d[..., 1] = d[..., 1] - L[2] * yz * img
        d[..., 0] = d[..., 0] - L[2] * xz * img
    if periodic[1]:
        img = np.rint(d[..., 1] * (1.0 / L[1]))
        d[..., 1] = d[..., 1] - L[1] * img
        d[..., 0] = d[..., 0] - L[1] * xy * img
    if periodic[0]:
        d[..., 0] = d[..., 0] - L[0] * np.rint(d[..., 0] * (1.0 / L[0]))
    return d


def weights(z1, da, lower, scale, num_bins, wrap):
    """[(bin, lambda)] of the segment from z1 to z1 - da: the header's expressions, one rounding per operation. None
    where the bin coordinates are out of every range (the kernel counts the pair's six words as overflow)."""
    s1 = (z1 - lower) * scale
    s0 = ((z1 - da) - lower) * scale
    lo, hi = min(s0, s1), max(s0, s1)
    if not (abs(lo) < 1.0e9 and abs(hi) < 1.0e9):
        return None
    flo, fhi = math.floor(lo), math.floor(hi)
    k0, k1 = flo, fhi
    if not wrap:
        k0, k1 = max(k0, 0), min(k1, num_bins - 1)
    out = []
    length = hi - lo
    for k in range(k0, k1 + 1):
        lam = 1.0 if flo == fhi else (min(hi, k + 1.0) - max(lo, float(k))) / length
        if not lam > 0.0:
            continue
        out.append((k % num_bins if wrap else k, lam))
    return out


# ---------------------------------------------------------------------------
# evaluators: f(rsq, key) -> (evaluated, force_divr)
# ---------------------------------------------------------------------------
def _xplor(rsq, ronsq, rcutsq, f, e):
    """HOOMD's XPLOR smoothing of an evaluated pair (force_divr, energy)."""
    if rsq >= ronsq and rsq < rcutsq:
        d = rcutsq - ronsq
        inv = 1.0 / (d * d * d)
        m = rsq - rcutsq
        s = m * m * (rcutsq + 2.0 * rsq - 3.0 * ronsq) * inv
        ds = 12.0 * (rsq - ronsq) * m * inv
        return s * f - ds * e
    return f


def oracle_pair(oracle, name, params, r_cut, r_on=None, mode="none"):
    """Pair evaluator over type pairs: ``params[ti][tj]`` dicts of the reference's keys, ``r_cut`` / ``r_on`` (T, T)."""
    r_cut = np.asarray(r_cut, dtype=np.float64)
    r_on = np.zeros_like(r_cut) if r_on is None else np.broadcast_to(np.asarray(r_on, dtype=np.float64), r_cut.shape)
    packed = [[oracle.pack_pair_params(name, p) for p in row] for row in params]
    lib, pid = oracle.lib(), oracle.PAIR_IDS[name]

    def f(rsq, key):
        ti, tj = key
        rcutsq, ronsq = r_cut[ti, tj] ** 2, r_on[ti, tj] ** 2
        shift = mode == "shift" or (mode == "xplor" and ronsq > rcutsq)
        fd, e = C.c_double(0), C.c_double(0)
        p = packed[ti][tj]
        ok = lib.azo_pair_eval_by_id(pid, p.ctypes.data_as(C.c_void_p), float(rsq), float(rcutsq), int(shift), C.byref(fd), C.byref(e))
        if not ok:
            return False, 0.0
        return True, (_xplor(rsq, ronsq, rcutsq, fd.value, e.value) if mode == "xplor" else fd.value)

    return f


def oracle_bond(oracle, name, params):
    """Bond evaluator over bond types: ``params[t]`` dicts."""
    packed = [oracle.pack_bond_params(name, p) for p in params]
    lib, bid = oracle.lib(), oracle.BOND_IDS[name]

    def f(rsq, t):
        fd, e = C.c_double(0), C.c_double(0)
        ok = lib.azo_bond_eval_by_id(bid, packed[t].ctypes.data_as(C.c_void_p), float(rsq), C.byref(fd), C.byref(e))
        return bool(ok), fd.value

    return f


def special_pair_lj(params):
    """``params[t] = dict(epsilon, sigma, r_cut)``: F / r = r^-2 r^-6 (12 lj1 r^-6 - 6 lj2) inside r_cut, lj1 = 4 eps sigma^12,
    lj2 = 4 eps sigma^6; always evaluated (0 from r_cut on)."""
    def f(rsq, t):
        p = params[t]
        s6 = p["sigma"] ** 6
        lj1, lj2 = 4.0 * p["epsilon"] * s6 * s6, 4.0 * p["epsilon"] * s6
        if not rsq < p["r_cut"] ** 2:
            return True, 0.0
        r2inv = 1.0 / rsq
        r6inv = r2inv * r2inv * r2inv
        return True, r2inv * r6inv * (12.0 * lj1 * r6inv - 6.0 * lj2)

    return f


def table_pair(tables, r_cut):
    """``tables[ti][tj]`` of table_ref.pair_table; nothing below r_min or from r_cut on."""
    def f(rsq, key):
        ti, tj = key
        t = tables[ti][tj]
        if not rsq < r_cut[ti][tj] ** 2:
            return False, 0.0
        r = math.sqrt(rsq)
        if not r >= t["r_min"]:
            return False, 0.0
        F = TR.interpolate(t["rows"], t["r_min"], t["dr"], np.array([r]))[1][0]
        return True, F / r

    return f


def table_bond(tables):
    """``tables[t]`` of table_ref.bond_table; a bond outside [r_min, r_max) is rejected."""
    def f(rsq, t):
        tb = tables[t]
        r = math.sqrt(rsq)
        if not (r >= tb["r_min"] and r < tb["r_end"]):
            return False, 0.0
        return True, TR.interpolate(tb["rows"], tb["r_min"], tb["dr"], np.array([r]))[1][0] / r

    return f


# ---------------------------------------------------------------------------
# the profile
# ---------------------------------------------------------------------------
class Accumulator:
    def __init__(self, num_bins, shift, max_term):
        self.nb, self.shift, self.max_term = num_bins, shift, max_term
        self.words = [0] * (6 * num_bins)
        self.abs_terms = np.zeros((num_bins, 6))
        self.n_terms = np.zeros((num_bins, 6), dtype=np.int64)
        self.pairs = self.terms = self.over = 0
        self.w_total = [0.0] * 6      # sum over the pairs of w, in Python floats (for the sum rule)
        self.lambda_sums = []

    def pair(self, d, fdivr, z1, axis, lower, scale, wrap):
        self.pairs += 1
        fx, fy, fz = fdivr * d[0], fdivr * d[1], fdivr * d[2]
        w = (fx * d[0], fx * d[1], fx * d[2], fy * d[1], fy * d[2], fz * d[2])
        bins = weights(z1, d[axis], lower, scale, self.nb, wrap)
        if bins is None:
            self.over += 6
            return
        self.lambda_sums.append(sum(lam for _, lam in bins))
        for c in range(6):
            self.w_total[c] += w[c]
        for k, lam in bins:
            for c in range(6):
                t = lam * w[c]
                if abs(t) < self.max_term:
                    self.words[6 * k + c] += int(round(t * 2.0 ** self.shift))  # (exact product; round half to even)
                    self.abs_terms[k, c] += abs(t)
                    self.n_terms[k, c] += 1
                    self.terms += 1
                else:
                    self.over += 1

    def row(self):
        return self.words + [self.pairs, self.terms, self.over, self.shift]


def profile(pos, types, tags, L, axis, num_bins, shift, max_term, pair_forces=(), listed_forces=(), lower=None, upper=None,
            tilt=(0.0, 0.0, 0.0), periodic=(True, True, True)):
    """``pair_forces``: dicts ``eval`` (an evaluator over type pairs), ``r_max`` (the radius of the walk) and ``excluded``
    (a set of frozensets of particle indices, may be missing). ``listed_forces``: dicts ``eval`` (over group types) and
    ``groups`` ([(i, j, type)]). Returns the ``Accumulator``."""
    pos = np.asarray(pos, dtype=np.float64)
    n = pos.shape[0]
    wrap = lower is None and bool(periodic[axis])
    if lower is None:
        lower, upper = -0.5 * L[axis], 0.5 * L[axis]
    scale = num_bins / (upper - lower)
    acc = Accumulator(num_bins, shift, max_term)

    def oriented(i, j):
        return (i, j) if tags[i] < tags[j] else (j, i)

    for force in pair_forces:
        excluded = force.get("excluded", ())
        i, j = np.triu_indices(n, 1)
        d = min_image(pos[i] - pos[j], L, tilt, periodic)
        rsq = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        for k in np.nonzero(rsq < force["r_max"] ** 2)[0]:
            a, b = oriented(int(i[k]), int(j[k]))
            if frozenset((a, b)) in excluded:
                continue
            dd = min_image(pos[a] - pos[b], L, tilt, periodic)
            r2 = dd[0] * dd[0] + dd[1] * dd[1] + dd[2] * dd[2]
            ok, fd = force["eval"](r2, (int(types[a]), int(types[b])))
            if ok:
                acc.pair(dd, fd, pos[a, axis], axis, lower, scale, wrap)
    for force in listed_forces:
        for i, j, t in force["groups"]:
            if i == j:
                continue
            a, b = oriented(int(i), int(j))
            dd = min_image(pos[a] - pos[b], L, tilt, periodic)
            r2 = dd[0] * dd[0] + dd[1] * dd[1] + dd[2] * dd[2]
            ok, fd = force["eval"](r2, int(t))
            if ok:
                acc.pair(dd, fd, pos[a, axis], axis, lower, scale, wrap)
    return acc


def tolerance(acc, K):
    """Per bin and component, in units of 2^-shift: K u sum |terms| + one unit per term (each side rounds once to the
    grid, and a term that differs by less than a unit can land one grid point apart)."""
    return K * U_ROUND * acc.abs_terms * 2.0 ** acc.shift + acc.n_terms
