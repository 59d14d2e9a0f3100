"""Writes tests/golden/evaluator_cases.npz: every pair and bond evaluator in closed form at 60 digits (mpmath).

    python tests/golden/make_evaluator_cases.py           # rewrite the fixture
    python tests/golden/make_evaluator_cases.py --check   # recompute, compare byte for byte, print the oracle's constants

Written from the published definitions alone (the potentials' documented formulas; HOOMD's documentation
for the shift and the XPLOR smoothing); no statement of the evaluators under test is restated here. Every potential is a
list of additive terms T_k(r), exactly as its definition is written, and every force is mp.diff of the sum: a wrong
hand derivative cannot be in both the fixture and a kernel.

Per point the fixture holds r, U, F = -U' and the two scales

    cond_U = sum_k |T_k| + |r U'|        cond_F = sum_k |T_k'| + |r U''|

The first summand is what rounding each term once costs; the second is the best any float64 code can do once r (here
r^2, which is what an evaluator is given) has been rounded. A test then asks |got - mp| <= B u cond with u = 2^-53
and a small B: a bar per point that follows the well, the zero of the force and the tail through every decade.

Modes. shift: U - U(r_cut), the scale gains |U(r_cut)| (not stored: cU + |ecut|). xplor (HOOMD):
S(r) = (r_c^2 - r^2)^2 (r_c^2 + 2 r^2 - 3 r_on^2) / (r_c^2 - r_on^2)^3 for r_on <= r < r_c, U_x = S U, F_x = -(S U)'
by mp.diff. Scales of the smoothed function: cUx = S sum|T_k| + |r U_x'| and cFx = S cond_F + |S' U| + |r U_x''|.
The last summand of cFx is the general definition's input-rounding term applied to U_x; without it no float64 code
can meet the bar next to the cutoff, where S cond_F + |S' U| vanishes like (r_c - r) but r S'' U does not.

A point is "evaluated" when r < r_cut and the pair interacts at all (A, epsilon != 0); everything else is exact zeros.
r < r_cut and r^2 < r_cut^2 in float64 agree for every r here (the double below r_cut squares to at least one ulp
below r_cut^2).

TwoPatchMorse: U = U_Morse(r) Omega(gamma_i) Omega(gamma_j), gamma = rhat . n, n = q e_x q*, Omega(g) =
1 / (1 + exp(-omega (g^2 - alpha))), U_Morse = M_d ((1 - exp(-(r - r_eq) / M_r))^2 - 1), and -M_d inside r_eq without
repulsion. The energy is (U_Morse - U_Morse(r_cut)) Omega_i Omega_j with shift; the force is -grad_{r_i} of the
UNSHIFTED U_Morse Omega_i Omega_j in both modes -- the reference's convention (AnisoPairEvaluatorTwoPatchMorse.h:176-207:
the shift is subtracted from the energy after the force has been formed), not the gradient of the shifted energy. The
torque on i is -d/dtheta of the same function with q_i rotated by theta about each space axis, the torque on j
likewise, all by mp.diff. The anisotropic evaluator includes r = r_cut itself (it rejects r^2 > r_cut^2 only).
Its scales are the absolute chain-rule terms (U_Morse counted as its two terms M_d (1 - e)^2 and -M_d) plus the rounding
of the inputs: dr relative to itself, the components of n relative to |q|^2 = 1 (see tpm_set).

Clusters: 32 isolated PerturbedLJ groups of 5 to 9 particles; per-particle sums of the pair terms, the group's virial as
W_ab = -dU_group / d eps_ab under r -> (1 + eps) r (mp.diff; from the physics alone: sign, the 1/2 per particle and the
order xx, xy, xz, yy, yz, zz follow), and the per-particle split 1/2 sum_j dr_a dr_b F / r.
"""

import io
import json
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "evaluator_cases.npz")
DPS = 60
N_SWEEP = 128
U_ROUND = 2.0 ** -53


def _mp():
    import mpmath as mp

    mp.mp.dps = DPS
    return mp


# ---------------------------------------------------------------------------
# parameter sets: (r_cut, r_min, params); SWEEPS of make_golden.py plus the edges
# ---------------------------------------------------------------------------
def _cc(a_1, a_2, sigma, r_cut, A=100.0):
    return (r_cut, a_1 + a_2 + 0.3 * sigma, dict(A=A, a_1=a_1, a_2=a_2, sigma=sigma))


PAIR_SETS = {
    "PerturbedLennardJones": [
        (3.0, 0.8, dict(epsilon=1.0, sigma=1.0, attraction_scale_factor=0.5)),
        (3.0, 0.8, dict(epsilon=2.0, sigma=1.05, attraction_scale_factor=0.0)),
        (3.0, 2.3, dict(epsilon=0.7, sigma=2.9, attraction_scale_factor=1.0)),  # r_cut < 2^(1/6) sigma: the wca_rsq clamp
    ],
    "Hertz": [(1.5, 0.05, dict(epsilon=2.0)), (1.5, 0.05, dict(epsilon=0.5)), (1.5, 0.05, dict(epsilon=0.0))],
    "ExpandedYukawa": [
        (3.0, 0.55, dict(epsilon=1.0, kappa=1.0, delta=0.5)),  # r - delta from 0.05
        (3.0, 0.55, dict(epsilon=3.0, kappa=3.0, delta=0.0)),
        (3.0, 0.55, dict(epsilon=1.0, kappa=0.1, delta=0.2)),
    ],
    "Colloid": [
        (6.0, 1.8, dict(A=100.0, a_1=0.0, a_2=0.0, sigma=2.0)),
        (6.0, 1.5 + 0.3 * 1.05, dict(A=100.0, a_1=1.5, a_2=0.0, sigma=1.05)),
        (14.0, 10.3, dict(A=100.0, a_1=0.0, a_2=10.0, sigma=1.0)),
        _cc(1.5, 0.75, 1.05, 6.0),
        _cc(0.15, 0.19, 0.35, 2.5),
        _cc(10.0, 10.0, 1.0, 25.0),  # D = 0
        _cc(5.0, 1.0, 1.0, 10.0),
        _cc(1.5, 0.75, 1.05, 6.0, A=0.0),
    ],
    "DPDConservative": [(1.0, 0.05, dict(A=25.0, gamma=4.5, s=0.5)), (1.0, 0.05, dict(A=2.0, gamma=1.0, s=2.0)),
                        (1.0, 0.05, dict(A=0.0, gamma=4.5, s=2.0))],
}
SHIFT_MATTERS = {"PerturbedLennardJones": True, "Hertz": False, "ExpandedYukawa": True, "Colloid": True,
                 "DPDConservative": False}
BOND_SETS = {
    "DoubleWell": [dict(r_0=1.0, r_1=2.0, U_1=1.0, U_tilt=0.5), dict(r_0=0.5, r_1=2.5, U_1=5.0, U_tilt=0.0)],
    "Quartic": [dict(k=1434.3, r_0=1.5, b_1=-0.7589, b_2=0.0, U_0=67.2234, sigma=1.0, epsilon=1.0, delta=0.0),
                dict(k=1434.3, r_0=1.5, b_1=-0.7589, b_2=0.0, U_0=67.2234, sigma=1.0, epsilon=1.0, delta=0.5)],
}
TPM_RCUT = 1.3
TPM_SETS = [dict(M_d=1.8341, M_r=0.0302, r_eq=1.0043, omega=5.0, alpha=0.40, repulsion=False),
            dict(M_d=1.8341, M_r=0.0302, r_eq=1.0043, omega=5.0, alpha=0.40, repulsion=True)]
CLUSTER = dict(r_cut=3.0, params=dict(epsilon=1.0, sigma=1.0, attraction_scale_factor=0.5), groups=32, gap=40.0)


def _r_on(r_cut, r_min):
    return float(np.round(r_min + 0.6 * (r_cut - r_min), 3))


# ---------------------------------------------------------------------------
# the definitions: each returns the additive terms of U as smooth functions of r, on the branch that r0 lies on
# ---------------------------------------------------------------------------
def _f(mp, x):
    return mp.mpf(float(x))


def terms_plj(mp, p, r0):
    """4 eps ((s/r)^12 - (s/r)^6) + (1 - lam) eps for r <= 2^(1/6) s; lam 4 eps ((s/r)^12 - (s/r)^6) beyond."""
    eps, s, lam = _f(mp, p["epsilon"]), _f(mp, p["sigma"]), _f(mp, p["attraction_scale_factor"])
    if eps == 0:
        return None
    if r0 <= mp.root(2, 6) * s:
        return [lambda r: 4 * eps * (s / r) ** 12, lambda r: -4 * eps * (s / r) ** 6, lambda r: (1 - lam) * eps]
    return [lambda r: lam * 4 * eps * (s / r) ** 12, lambda r: -lam * 4 * eps * (s / r) ** 6]


def terms_hertz(mp, p, r0, r_cut):
    eps, rc = _f(mp, p["epsilon"]), _f(mp, r_cut)
    if eps == 0:
        return None
    return [lambda r: eps * (1 - r / rc) ** (mp.mpf(5) / 2)]


def terms_yukawa(mp, p, r0):
    eps, kappa, delta = _f(mp, p["epsilon"]), _f(mp, p["kappa"]), _f(mp, p["delta"])
    if eps == 0:
        return None
    return [lambda r: eps * mp.exp(-kappa * (r - delta)) / (r - delta)]


def terms_colloid(mp, p, r0):
    """Everaers and Ejtehadi's integrated Lennard-Jones potentials, as LAMMPS' pair_style colloid documents them."""
    A, a1, a2, s = (_f(mp, p[k]) for k in ("A", "a_1", "a_2", "sigma"))
    if A == 0:
        return None
    if a1 == 0 and a2 == 0:
        return [lambda r: A / 36 * (s / r) ** 12, lambda r: -A / 36 * (s / r) ** 6]
    if a1 == 0 or a2 == 0:
        a = max(a1, a2)

        def pre(r):
            return 2 * a ** 3 * s ** 3 * A / (9 * (a * a - r * r) ** 3)

        def rep(r):
            return -pre(r) * ((5 * a ** 6 + 45 * a ** 4 * r ** 2 + 63 * a ** 2 * r ** 4 + 15 * r ** 6) * s ** 6
                              / (15 * (a - r) ** 6 * (a + r) ** 6))

        return [pre, rep]
    S, D, P = a1 + a2, a1 - a2, a1 * a2
    c = A * s ** 6 / 37800
    return [
        lambda r: -A / 6 * 2 * P / (r * r - S * S),
        lambda r: -A / 6 * 2 * P / (r * r - D * D),
        lambda r: -A / 6 * mp.log((r * r - S * S) / (r * r - D * D)),
        lambda r: c / r * (r * r - 7 * r * S + 6 * (a1 * a1 + 7 * P + a2 * a2)) / (r - S) ** 7,
        lambda r: c / r * (r * r + 7 * r * S + 6 * (a1 * a1 + 7 * P + a2 * a2)) / (r + S) ** 7,
        lambda r: -c / r * (r * r + 7 * r * D + 6 * (a1 * a1 - 7 * P + a2 * a2)) / (r + D) ** 7,
        lambda r: -c / r * (r * r - 7 * r * D + 6 * (a1 * a1 - 7 * P + a2 * a2)) / (r - D) ** 7,
    ]


def terms_dpd(mp, p, r0, r_cut):
    """A (r_c - r) - (A / (2 r_c)) (r_c^2 - r^2); not guarded by A != 0 (an A = 0 pair is evaluated, to zeros)."""
    A, rc = _f(mp, p["A"]), _f(mp, r_cut)
    return [lambda r: A * (rc - r), lambda r: -A / (2 * rc) * (rc * rc - r * r)]


def pair_terms(mp, name, p, r0, r_cut):
    if name == "PerturbedLennardJones":
        return terms_plj(mp, p, r0)
    if name == "Hertz":
        return terms_hertz(mp, p, r0, r_cut)
    if name == "ExpandedYukawa":
        return terms_yukawa(mp, p, r0)
    if name == "Colloid":
        return terms_colloid(mp, p, r0)
    return terms_dpd(mp, p, r0, r_cut)


def terms_double_well(mp, p, r0):
    """U_1 ((r - r_1)^2 - (r_1 - r_0)^2)^2 / (r_1 - r_0)^4
    + U_tilt (1 + (r - r_1) / (r_1 - r_0) - ((r - r_1)^2 - (r_1 - r_0)^2)^2 / (r_1 - r_0)^4)."""
    q0, q1, U1, Ut = (_f(mp, p[k]) for k in ("r_0", "r_1", "U_1", "U_tilt"))
    d = q1 - q0

    def w(r):
        return ((r - q1) ** 2 - d * d) ** 2 / d ** 4

    return [lambda r: U1 * w(r), lambda r: Ut, lambda r: Ut * (r - q1) / d, lambda r: -Ut * w(r)]


def terms_quartic(mp, p, r0):
    """k (x - b_1) (x - b_2) x^2 + U_0, x = r - delta - r_0, for r - delta < r_0 and U_0 beyond; plus the WCA core
    4 eps ((s / (r - delta))^12 - (s / (r - delta))^6) + eps for r - delta < 2^(1/6) s."""
    k, q0, b1, b2, U0, s, eps, delta = (_f(mp, p[n]) for n in ("k", "r_0", "b_1", "b_2", "U_0", "sigma", "epsilon", "delta"))
    t = [lambda r: U0]
    if r0 - delta < q0:
        t.append(lambda r: k * (r - delta - q0 - b1) * (r - delta - q0 - b2) * (r - delta - q0) ** 2)
    if r0 - delta < mp.root(2, 6) * s:
        t += [lambda r: 4 * eps * (s / (r - delta)) ** 12, lambda r: -4 * eps * (s / (r - delta)) ** 6, lambda r: eps]
    return t


def bond_terms(mp, name, p, r0):
    return terms_double_well(mp, p, r0) if name == "DoubleWell" else terms_quartic(mp, p, r0)


def point(mp, terms, r):
    """(U, F, cond_U, cond_F) of sum(terms) at r."""
    def U(x):
        return mp.fsum(t(x) for t in terms)

    d1 = mp.diff(U, r)
    d2 = mp.diff(U, r, 2)
    cU = mp.fsum(abs(t(r)) for t in terms) + abs(r * d1)
    cF = mp.fsum(abs(mp.diff(t, r)) for t in terms) + abs(r * d2)
    return U(r), -d1, cU, cF


def xplor_point(mp, terms, r, r_on, r_cut, plain):
    """(U_x, F_x, cUx, cFx) of S U at r; ``plain`` = point(...) of the unsmoothed potential."""
    if r < r_on:
        return plain
    rc2, ro2 = r_cut * r_cut, r_on * r_on

    def S(x):
        return (rc2 - x * x) ** 2 * (rc2 + 2 * x * x - 3 * ro2) / (rc2 - ro2) ** 3

    def Ux(x):
        return S(x) * mp.fsum(t(x) for t in terms)

    U, _, cU, cF = plain
    d1, d2 = mp.diff(Ux, r), mp.diff(Ux, r, 2)
    s, ds = S(r), mp.diff(S, r)
    abs_terms = mp.fsum(abs(t(r)) for t in terms)
    return Ux(r), -d1, s * abs_terms + abs(r * d1), s * cF + abs(ds * U) + abs(r * d2)


def _ulp_down(x):
    return float(np.nextafter(x, -np.inf))


def _ulp_up(x):
    return float(np.nextafter(x, np.inf))


def pack_scale(x):
    """A scale as the high 32-bit word of its float64 (rounded down by less than 2^-20): four bytes, the full range."""
    return (np.ascontiguousarray(x, dtype=np.float64).view(np.uint64) >> np.uint64(32)).astype(np.uint32)


def unpack_scale(w):
    return (w.astype(np.uint64) << np.uint64(32)).view(np.float64)


def sweep_r(name, p, r_cut, r_min):
    r = np.linspace(r_min, 1.05 * r_cut, N_SWEEP, endpoint=False)
    if name == "PerturbedLennardJones":  # at, one ulp below and one ulp above 2^(1/6) sigma (three sweep points moved)
        rw = 2.0 ** (1.0 / 6.0) * p["sigma"]
        if rw < r[-1]:  # (beyond the sweep when r_cut < 2^(1/6) sigma: nothing is evaluated there)
            k = min(int(np.searchsorted(r, rw)), N_SWEEP - 3)
            r[k:k + 3] = (_ulp_down(rw), rw, _ulp_up(rw))
    return np.concatenate([r, [r_cut * (1.0 - 1e-9), _ulp_down(r_cut), r_cut]])


def pair_set(mp, name, p, r_cut, r_min):
    r = sweep_r(name, p, r_cut, r_min)
    r_on = _r_on(r_cut, r_min)
    n = r.size
    out = {k: np.zeros(n) for k in ("U", "F", "Ush", "Ux", "Fx")}
    out.update({k: np.zeros(n) for k in ("cU", "cF", "cUx", "cFx")})
    out["r"] = r
    out["ev"] = np.zeros(n, dtype=np.uint8)
    rc, ro = _f(mp, r_cut), _f(mp, r_on)
    at_cut = pair_terms(mp, name, p, rc, r_cut)
    ecut = mp.fsum(t(rc) for t in at_cut) if at_cut is not None else mp.mpf(0)
    for i, x in enumerate(r):
        rr = _f(mp, x)
        terms = pair_terms(mp, name, p, rr, r_cut)
        if terms is None or not rr < rc:
            continue
        plain = point(mp, terms, rr)
        sm = xplor_point(mp, terms, rr, ro, rc, plain)
        out["ev"][i] = 1
        out["U"][i], out["F"][i], out["cU"][i], out["cF"][i] = (float(v) for v in plain)
        out["Ush"][i] = float(plain[0] - ecut)
        out["Ux"][i], out["Fx"][i], out["cUx"][i], out["cFx"][i] = (float(v) for v in sm)
    if not SHIFT_MATTERS[name]:
        del out["Ush"]
    smooth = r >= r_on  # below r_on the xplor values are the plain ones and are not stored twice
    for key in ("Ux", "Fx", "cUx", "cFx"):
        out[key] = out[key][smooth]
    for key in ("cU", "cF", "cUx", "cFx"):
        out[key] = pack_scale(out[key])
    meta = dict(params=p, r_cut=r_cut, r_on=r_on, r_min=r_min, ecut=float(ecut))
    return out, meta


def bond_r(name, p):
    r = np.linspace(0.6, 2.6, N_SWEEP)
    extra = [p["r_0"], p["r_1"]] if name == "DoubleWell" else []
    if name == "Quartic":
        edge = p["r_0"] + p["delta"]
        wca = 2.0 ** (1.0 / 6.0) * p["sigma"] + p["delta"]
        extra = [p["r_0"] * (1.0 - 1e-9) + p["delta"], _ulp_down(edge), edge, _ulp_up(edge), _ulp_down(wca), wca, _ulp_up(wca)]
    return np.concatenate([r, extra])


def bond_set(mp, name, p):
    r = bond_r(name, p)
    out = dict(r=r, U=np.zeros(r.size), F=np.zeros(r.size), cU=np.zeros(r.size), cF=np.zeros(r.size))
    for i, x in enumerate(r):
        rr = _f(mp, x)
        out["U"][i], out["F"][i], out["cU"][i], out["cF"][i] = (float(v) for v in point(mp, bond_terms(mp, name, p, rr), rr))
    out["cU"], out["cF"] = pack_scale(out["cU"]), pack_scale(out["cF"])
    return out, dict(params=p)


# ---------------------------------------------------------------------------
# TwoPatchMorse
# ---------------------------------------------------------------------------
GRID = 2.0 ** -30  # coordinates are multiples of it: differences and the offsets of isolated groups are exact in float64


def _quant(x):
    return np.round(np.asarray(x) / GRID) * GRID


def tpm_inputs():
    """64 pairs: dr = r_i - r_j, q_i, q_j (scalar part first). 52 generic ones (seeded) with r across r_eq up to r_cut;
    12 special ones along x: gamma = +1, -1, ~0 and gamma^2 ~ alpha, each at r < r_eq, r > r_eq and r = r_cut exactly."""
    rng = np.random.default_rng(20260117)
    dr, qi, qj = [], [], []
    for k in range(52):
        d = rng.normal(size=3)
        d *= rng.uniform(0.93, TPM_RCUT - 1e-3) / np.linalg.norm(d)
        dr.append(_quant(d))
        for q in (qi, qj):
            v = rng.normal(size=4)
            q.append(v / np.linalg.norm(v))
    ident = np.array([1.0, 0.0, 0.0, 0.0])

    def about_z(phi):
        return np.array([np.cos(0.5 * phi), 0.0, 0.0, np.sin(0.5 * phi)])

    generic = about_z(0.7)
    for r in (0.96, 1.1, TPM_RCUT):
        r = float(_quant(r)) if r != TPM_RCUT else r
        for d, q in (((r, 0, 0), ident), ((-r, 0, 0), ident), ((r, 0, 0), about_z(0.5 * np.pi)),
                     ((r, 0, 0), about_z(np.arccos(np.sqrt(0.40))))):
            dr.append(np.array(d, dtype=np.float64))
            qi.append(q)
            qj.append(generic)
    return np.array(dr), np.array(qi), np.array(qj)


def _rot_ex(q):
    """q e_x q* for q = (s, u): (s^2 - |u|^2) e_x + 2 s (u x e_x) + 2 (u . e_x) u."""
    s, ux, uy, uz = q
    return [s * s - (ux * ux + uy * uy + uz * uz) + 2 * ux * ux, 2 * s * uz + 2 * ux * uy, -2 * s * uy + 2 * ux * uz]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def tpm_set(mp, p, dr_all, qi_all, qj_all):
    Md, Mr, req, om, al = (_f(mp, p[k]) for k in ("M_d", "M_r", "r_eq", "omega", "alpha"))
    rc = _f(mp, TPM_RCUT)
    rep = bool(p["repulsion"])
    n = dr_all.shape[0]
    out = dict(E=np.zeros(n), Esh=np.zeros(n), F=np.zeros((n, 3)), Ti=np.zeros((n, 3)), Tj=np.zeros((n, 3)),
               cE=np.zeros(n), cEsh=np.zeros(n), cF=np.zeros((n, 3)), cTi=np.zeros((n, 3)), cTj=np.zeros((n, 3)))
    for k in range(n):
        d0 = [_f(mp, v) for v in dr_all[k]]
        qi = [_f(mp, v) for v in qi_all[k]]
        qj = [_f(mp, v) for v in qj_all[k]]
        r0 = mp.sqrt(mp.fsum(v * v for v in d0))
        flat = (not rep) and not (r0 > req)  # U_Morse = -M_d: the branch of this pair, fixed before differentiating

        def morse(r):
            if flat:
                return -Md + 0 * r
            return Md * ((1 - mp.exp(-(r - req) / Mr)) ** 2 - 1)

        def omega(g):
            return 1 / (1 + mp.exp(-om * (g * g - al)))

        def U9(*x):  # U as a function of dr, n_i, n_j (nine variables; n need not be a unit vector)
            d, ni, nj = x[0:3], x[3:6], x[6:9]
            r = mp.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
            gi = (d[0] * ni[0] + d[1] * ni[1] + d[2] * ni[2]) / r
            gj = (d[0] * nj[0] + d[1] * nj[1] + d[2] * nj[2]) / r
            return morse(r) * omega(gi) * omega(gj)

        def rotated(q, axis, th):  # q turned by th about a space axis: n -> R n
            h = [mp.cos(th / 2)] + [mp.sin(th / 2) if a == axis else mp.mpf(0) for a in range(3)]
            s1, v1, s2, v2 = h[0], h[1:], q[0], q[1:]
            c = _cross(v1, v2)
            return [s1 * s2 - (v1[0] * v2[0] + v1[1] * v2[1] + v1[2] * v2[2])] + [s1 * v2[a] + s2 * v1[a] + c[a] for a in range(3)]

        ni0, nj0 = _rot_ex(qi), _rot_ex(qj)
        x0 = d0 + ni0 + nj0
        U0 = U9(*x0)
        om_ij = omega(mp.fsum(d0[a] * ni0[a] for a in range(3)) / r0) * omega(mp.fsum(d0[a] * nj0[a] for a in range(3)) / r0)
        ush = Md * ((1 - mp.exp(-(rc - req) / Mr)) ** 2 - 1) * om_ij

        def order(*idx):
            o = [0] * 9
            for i in idx:
                o[i] += 1
            return tuple(o)

        grad = [mp.diff(U9, tuple(x0), order(i)) for i in range(9)]
        hess = [[None] * 9 for _ in range(9)]
        for i in range(9):
            for j in range(i, 9):
                hess[i][j] = hess[j][i] = mp.diff(U9, tuple(x0), order(i, j))
        # values: force by the gradient with respect to r_i (dr = r_i - r_j), torques by rotating the quaternions
        F = [-grad[a] for a in range(3)]
        Ti = [-mp.diff(lambda th, a=a: U9(*(d0 + _rot_ex(rotated(qi, a, th)) + nj0)), 0) for a in range(3)]
        Tj = [-mp.diff(lambda th, a=a: U9(*(d0 + ni0 + _rot_ex(rotated(qj, a, th)))), 0) for a in range(3)]
        # scales: the absolute chain-rule terms (U through r, gamma_i, gamma_j) plus the rounding of the nine inputs.
        # dr is rounded relative to itself; a component of n = q e_x q* is a sum of products of size |q|^2 = 1 and is
        # rounded relative to 1, however small it is (gamma ~ 0). U_Morse is two terms, M_d (1 - e)^2 and -M_d: where
        # they cancel (r >> r_eq) every quantity proportional to U_Morse carries their sum, not their difference.
        weight = [abs(v) for v in d0] + [mp.mpf(1)] * 6
        inputs = lambda row: mp.fsum(weight[j] * abs(row[j]) for j in range(9))  # noqa: E731
        amp = mp.mpf(1) if flat else (Md * (1 - mp.exp(-(r0 - req) / Mr)) ** 2 + Md) / abs(morse(r0))
        cE = amp * abs(U0) + inputs(grad)
        u = [v / r0 for v in d0]

        def chain_force(a):  # dU/dr u_a + sum over i, j of dU/dgamma (n_a - gamma u_a) / r, term by term
            dUdr = mp.fsum(grad[b] * u[b] for b in range(3))  # (includes the gamma part along u, which is zero)
            tot = abs(dUdr * u[a])
            for off in (3, 6):
                nn = x0[off:off + 3]
                g = mp.fsum(u[b] * nn[b] for b in range(3))
                # dU/dgamma = grad_n U . (r / d) ... from U(gamma = d . n / r): grad_n U = dU/dgamma u
                dUdg = mp.fsum(grad[off + b] * u[b] for b in range(3))
                tot += amp * (abs(dUdg * nn[a]) + abs(dUdg * g * u[a])) / r0
            return tot

        def chain_torque(off, a):  # T = -n x grad_n U
            nn, g = x0[off:off + 3], grad[off:off + 3]
            b, c = (a + 1) % 3, (a + 2) % 3
            return amp * (abs(nn[b] * g[c]) + abs(nn[c] * g[b]))

        def torque_inputs(off, a):
            nn = x0[off:off + 3]
            b, c = (a + 1) % 3, (a + 2) % 3
            return mp.fsum(weight[j] * abs(nn[b] * hess[off + c][j] - nn[c] * hess[off + b][j]) for j in range(9))

        out["E"][k], out["Esh"][k] = float(U0), float(U0 - ush)
        out["cE"][k], out["cEsh"][k] = float(cE), float(cE + (Md * (1 - mp.exp(-(rc - req) / Mr)) ** 2 + Md) * om_ij)
        for a in range(3):
            out["F"][k, a], out["Ti"][k, a], out["Tj"][k, a] = float(F[a]), float(Ti[a]), float(Tj[a])
            out["cF"][k, a] = float(chain_force(a) + inputs(hess[a]))
            out["cTi"][k, a] = float(chain_torque(3, a) + torque_inputs(3, a))
            out["cTj"][k, a] = float(chain_torque(6, a) + torque_inputs(6, a))
            # the rotation derivative and -n x grad_n U are the same torque
            assert abs(Ti[a] + (ni0[(a + 1) % 3] * grad[3 + (a + 2) % 3] - ni0[(a + 2) % 3] * grad[3 + (a + 1) % 3])) <= mp.mpf(10) ** -40 * (1 + abs(Ti[a]))
    for key in ("cE", "cEsh", "cF", "cTi", "cTj"):
        out[key] = pack_scale(out[key])
    return out, dict(params=p, r_cut=TPM_RCUT)


# ---------------------------------------------------------------------------
# PerturbedLJ clusters and their virial
# ---------------------------------------------------------------------------
def cluster_positions():
    """32 groups of 5 to 9 particles inside a ball of diameter 1.05 r_cut. Groups 0..15: every separation beyond
    2^(1/6) sigma (>= 1.13; a whole wave takes the tail-only form); groups 16..31: separations from 0.85 (mixed), one
    pair placed at 0.85. Every group holds one pair placed across the ball at a separation in [r_cut, 1.05 r_cut), so
    that every family meets listed neighbours just beyond the cutoff in batches with live pairs: along x at r_cut
    exactly in the first group of each family (r^2 == r_cut^2 in float64), in a seeded direction in the others."""
    rng = np.random.default_rng(20260118)
    r_cut, half = CLUSTER["r_cut"], CLUSTER["groups"] // 2
    R = 0.5 * 1.05 * r_cut
    xyz, group = [], []
    for g in range(CLUSTER["groups"]):
        size = 5 + (g * 3) % 5  # 5..9, every size in both families
        dmin = 1.13 if g < half else 0.85
        across = r_cut + 0.049 * r_cut * (g % half) / half  # r_cut ... 1.046 r_cut
        axis = rng.normal(size=3)
        axis = np.array([1.0, 0.0, 0.0]) if g % half == 0 else axis / np.linalg.norm(axis)
        pts = [_quant(-0.5 * across * axis), _quant(0.5 * across * axis)]
        if dmin == 0.85:  # one pair at the closest separation, about the centre and normal to the pair across the ball
            n = np.cross(axis, [0.0, 0.6, 0.8])
            n /= np.linalg.norm(n)
            pts += [_quant(-0.425 * n), _quant(0.425 * n)]
        while len(pts) < size:
            v = rng.uniform(-R, R, size=3)
            if np.linalg.norm(v) <= R and all(np.linalg.norm(v - q) >= dmin for q in pts):
                pts.append(_quant(v))
        xyz += pts
        group += [g] * size
    return np.array(xyz), np.array(group)


def cluster_set(mp):
    xyz, group = cluster_positions()
    p, r_cut = CLUSTER["params"], CLUSTER["r_cut"]
    rc = _f(mp, r_cut)
    n, ng = xyz.shape[0], CLUSTER["groups"]
    ecut = mp.fsum(t(rc) for t in terms_plj(mp, p, rc))
    F, cF = [[mp.mpf(0)] * 3 for _ in range(n)], [mp.mpf(0)] * n
    E, Esh, cE, cEsh = ([mp.mpf(0)] * n for _ in range(4))
    W, cW = [[mp.mpf(0)] * 6 for _ in range(n)], [mp.mpf(0)] * n
    Wg = np.zeros((ng, 6))
    comp = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    for g in range(ng):
        idx = np.flatnonzero(group == g)
        pairs = []
        for ii, i in enumerate(idx):
            for j in idx[ii + 1:]:
                d = [_f(mp, xyz[i, a]) - _f(mp, xyz[j, a]) for a in range(3)]
                r = mp.sqrt(mp.fsum(v * v for v in d))
                if not r < rc:
                    continue
                terms = terms_plj(mp, p, r)
                U, Fr, cu, cf = point(mp, terms, r)
                pairs.append((d, terms))
                for me, sign in ((i, 1), (j, -1)):
                    for a in range(3):
                        F[me][a] += sign * Fr * d[a] / r
                    cF[me] += cf
                    E[me] += U / 2
                    Esh[me] += (U - ecut) / 2
                    cE[me] += cu / 2
                    cEsh[me] += (cu + abs(ecut)) / 2
                    cW[me] += cf * r / 2
                    for c, (a, b) in enumerate(comp):
                        W[me][c] += d[a] * d[b] * Fr / r / 2
        for c, (a, b) in enumerate(comp):
            def strained(e, a=a, b=b):  # the group's energy under r_a -> r_a + e r_b (pairs keep their branch)
                tot = mp.mpf(0)
                for d, terms in pairs:
                    dd = list(d)
                    dd[a] = dd[a] + e * d[b]
                    r = mp.sqrt(mp.fsum(v * v for v in dd))
                    tot += mp.fsum(t(r) for t in terms)
                return tot
            Wg[g, c] = float(-mp.diff(strained, 0))
    tof = lambda v: np.array([[float(x) for x in row] if isinstance(row, list) else float(row) for row in v])  # noqa: E731
    out = dict(xyz=xyz, group=group.astype(np.uint8), F=tof(F), E=tof(E), Esh=tof(Esh), W=tof(W), Wg=Wg,
               cF=pack_scale(tof(cF)), cE=pack_scale(tof(cE)), cEsh=pack_scale(tof(cEsh)), cW=pack_scale(tof(cW)))
    return out, dict(params=p, r_cut=r_cut, gap=CLUSTER["gap"], ecut=float(ecut))


# ---------------------------------------------------------------------------
# the file
# ---------------------------------------------------------------------------
def build():
    mp = _mp()
    arrays, meta = {}, dict(pair={}, bond={}, tpm=[], cluster=None, dps=DPS)
    for name, sets in PAIR_SETS.items():
        meta["pair"][name] = []
        for k, (r_cut, r_min, p) in enumerate(sets):
            out, m = pair_set(mp, name, p, r_cut, r_min)
            arrays.update({"%s.%d.%s" % (name, k, key): v for key, v in out.items()})
            meta["pair"][name].append(m)
    for name, sets in BOND_SETS.items():
        meta["bond"][name] = []
        for k, p in enumerate(sets):
            out, m = bond_set(mp, name, p)
            arrays.update({"%s.%d.%s" % (name, k, key): v for key, v in out.items()})
            meta["bond"][name].append(m)
    dr, qi, qj = tpm_inputs()
    arrays.update({"tpm.dr": dr, "tpm.qi": qi, "tpm.qj": qj})
    for k, p in enumerate(TPM_SETS):
        out, m = tpm_set(mp, p, dr, qi, qj)
        arrays.update({"tpm.%d.%s" % (k, key): v for key, v in out.items()})
        meta["tpm"].append(m)
    out, meta["cluster"] = cluster_set(mp)
    arrays.update({"cluster." + key: v for key, v in out.items()})
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    return arrays


def to_bytes(arrays):
    """An .npz with fixed member dates and order: the same arrays give the same bytes."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w") as z:
        for key in sorted(arrays):
            member = io.BytesIO()
            np.lib.format.write_array(member, np.ascontiguousarray(arrays[key]), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, member.getvalue(), compresslevel=9)
    return buf.getvalue()


def load(path=OUT):
    """(arrays, meta) of the committed fixture."""
    with np.load(path) as z:
        arrays = {k: z[k] for k in z.files}
    meta = json.loads(arrays.pop("meta").tobytes().decode())
    return arrays, meta


# ---------------------------------------------------------------------------
# --check: the oracle's constants, max |x_oracle - x_mp| / cond in units of u
# ---------------------------------------------------------------------------
def pair_expect(arrays, m, name, k, mode):
    """(U, F, cU, cF, evaluated) of a pair set in a mode, from the stored arrays."""
    g = lambda key: arrays["%s.%d.%s" % (name, k, key)]  # noqa: E731
    ev = g("ev").astype(bool)
    U, F, cU, cF = g("U"), g("F"), unpack_scale(g("cU")), unpack_scale(g("cF"))
    if mode == "xplor":
        smooth = g("r") >= m["r_on"]
        U, F, cU, cF = U.copy(), F.copy(), cU.copy(), cF.copy()
        U[smooth], F[smooth], cU[smooth], cF[smooth] = g("Ux"), g("Fx"), unpack_scale(g("cUx")), unpack_scale(g("cFx"))
    if mode == "shift" and SHIFT_MATTERS[name]:
        U, cU = g("Ush"), np.where(ev, cU + abs(m["ecut"]), 0.0)
    return U, F, cU, cF, ev


def dpd_cutoff_allowance(m, r, mode):
    """Absolute allowances (dU, dF) for DPDConservative at the cutoff points, where the scale of the energy says nothing:
    U = A (r_c - r) - A (r_c^2 - r^2) / (2 r_c) is written as two terms that cancel, with r and r_c each formed from a
    reciprocal square root and one more rounded operation (<= 2 u each, relative to r_c), then the subtraction and the
    product with A: at most 8 A r_c u in all (the second term's inputs r^2 and r_c^2 are exact). So per point
    |dU| <= 8 u cond_U + S 8 A r_c u and, through F_x = S F - S' U, |dF| <= 8 u cond_F + |S'| 8 A r_c u, with S = 1
    and S' = 0 outside xplor. A kernel that is wrong at the cutoff by more than a few A r_c u fails this."""
    r = np.asarray(r, dtype=np.float64)
    e = 8.0 * abs(m["params"]["A"]) * m["r_cut"] * U_ROUND
    S, dS = np.ones_like(r), np.zeros_like(r)
    if mode == "xplor":
        rc2, ro2 = m["r_cut"] ** 2, m["r_on"] ** 2
        sm = (r >= m["r_on"]) & (r < m["r_cut"])
        S[sm] = (rc2 - r[sm] ** 2) ** 2 * (rc2 + 2 * r[sm] ** 2 - 3 * ro2) / (rc2 - ro2) ** 3
        dS[sm] = 12 * r[sm] * (r[sm] ** 2 - ro2) * (r[sm] ** 2 - rc2) / (rc2 - ro2) ** 3
    return S * e, np.abs(dS) * e


def _k(got, want, cond):
    """max |got - want| / (u cond); points whose scale is zero must be exact."""
    got, want, cond = np.broadcast_arrays(np.asarray(got, dtype=np.float64), want, cond)
    live = cond > 0
    assert np.array_equal(got[~live], want[~live]), "a point without a scale is not exact"
    return float((np.abs(got[live] - want[live]) / (U_ROUND * cond[live])).max()) if live.any() else 0.0


def oracle_xplor(oracle, name, p, r, r_cut, r_on):
    """The oracle's pair loop on one isolated pair in xplor mode: (F, U)."""
    pos = oracle.pos4(np.array([[-0.5 * r, 0, 0], [0.5 * r, 0, 0]]))
    nl = (np.ones(2, dtype=np.uint32), np.arange(2, dtype=np.uint64), np.array([1, 0], dtype=np.uint32))
    f = oracle.pair_forces(name, pos, oracle.make_box(200.0, periodic=(0, 0, 0)), nl, oracle.pack_pair_params(name, p),
                           r_cut, r_on, "xplor")
    return f[1, 0], 2.0 * f[1, 3]


def oracle_constants(arrays, meta):
    """{(evaluator, set, mode or quantity): (K_E, K_F, ...)} of the CPU oracle on the fixture."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import oracle

    res = {}
    for name, sets in meta["pair"].items():
        for k, m in enumerate(sets):
            r = arrays["%s.%d.r" % (name, k)]
            for mode in ("none", "shift", "xplor"):
                U, F, cU, cF, ev = pair_expect(arrays, m, name, k, mode)
                got = np.zeros((r.size, 2))
                for i, x in enumerate(r):
                    if mode == "xplor":
                        got[i] = oracle_xplor(oracle, name, m["params"], x, m["r_cut"], m["r_on"])
                    else:
                        ok, fdr, e = oracle.eval_pair(name, m["params"], x, m["r_cut"], mode == "shift")
                        got[i] = (fdr * x, e) if ok else (0.0, 0.0)
                        assert bool(ok) == bool(ev[i]) or name == "DPDConservative", (name, k, i)
                sw, ed = slice(0, N_SWEEP), slice(N_SWEEP, None)  # the sweep; the three points at the cutoff
                res[(name, k, mode)] = (_k(got[sw, 1], U[sw], cU[sw]), _k(got[sw, 0], F[sw], cF[sw]),
                                        _k(got[ed, 1], U[ed], cU[ed]), _k(got[ed, 0], F[ed], cF[ed]))
    for name, sets in meta["bond"].items():
        for k, m in enumerate(sets):
            r = arrays["%s.%d.r" % (name, k)]
            got = np.array([oracle.eval_bond(name, m["params"], x) for x in r])
            res[(name, k, "bond")] = (_k(got[:, 2], arrays["%s.%d.U" % (name, k)], unpack_scale(arrays["%s.%d.cU" % (name, k)])),
                                      _k(got[:, 1] * r, arrays["%s.%d.F" % (name, k)], unpack_scale(arrays["%s.%d.cF" % (name, k)])))
    for k, m in enumerate(meta["tpm"]):
        def g(key, k=k):
            a = arrays["tpm.%d.%s" % (k, key)]
            return unpack_scale(a) if key.startswith("c") else a

        for shift in (False, True):
            rows = [oracle.eval_tpm(m["params"], arrays["tpm.dr"][i], arrays["tpm.qi"][i], arrays["tpm.qj"][i], m["r_cut"], shift)
                    for i in range(arrays["tpm.dr"].shape[0])]
            assert all(row[0] for row in rows)
            res[("TwoPatchMorse", k, "shift" if shift else "none")] = (
                _k([row[2] for row in rows], g("Esh" if shift else "E"), g("cEsh" if shift else "cE")),
                _k([row[1] for row in rows], g("F"), g("cF")), _k([row[3] for row in rows], g("Ti"), g("cTi")),
                _k([row[4] for row in rows], g("Tj"), g("cTj")))
    c = cluster_case(arrays, meta)
    for mode in ("none", "shift"):
        f, v = oracle.pair_forces("PerturbedLennardJones", c["pos"], oracle.make_box(c["L"], periodic=(0, 0, 0)), c["nl"],
                                  oracle.pack_pair_params("PerturbedLennardJones", c["params"]), c["r_cut"], mode=mode, virial=True)
        res[("clusters", 0, mode)] = cluster_constants(c, f, v, mode)
    return res


def cluster_case(arrays, meta):
    """The clusters as a system: positions (group g at y = (g - 16) gap), full lists within a group, expectations."""
    m = meta["cluster"]
    xyz, group = arrays["cluster.xyz"].copy(), arrays["cluster.group"].astype(np.int64)
    ng = int(group.max()) + 1
    xyz[:, 1] += (group - ng // 2) * m["gap"]
    n = xyz.shape[0]
    rows = [np.flatnonzero((group == group[i]) & (np.arange(n) != i)) for i in range(n)]
    n_neigh = np.array([len(x) for x in rows], dtype=np.uint32)
    head = (np.cumsum(n_neigh) - n_neigh).astype(np.uint64)
    pos = np.zeros((n, 4))
    pos[:, :3] = xyz
    c = dict(pos=pos, L=np.array([200.0, (ng + 2) * m["gap"], 200.0]), nl=(n_neigh, head, np.concatenate(rows).astype(np.uint32)),
             params=m["params"], r_cut=m["r_cut"], group=group, n_neigh=n_neigh.astype(np.float64))
    for key in ("F", "E", "Esh", "W", "Wg"):
        c[key] = arrays["cluster." + key]
    for key in ("cF", "cE", "cEsh", "cW"):
        c[key] = unpack_scale(arrays["cluster." + key])
    return c


def cluster_constants(c, f, v, mode, extra=None):
    """(K_E, K_F, K_W per particle, K_W per group) of forces f (n, 4) and virials v (6, n); ``extra`` (per particle) is
    subtracted from each particle's ratio before the maximum (a test's allowance per neighbour; never below zero)."""
    extra = np.zeros(f.shape[0]) if extra is None else extra
    E, cE = (c["Esh"], c["cEsh"]) if mode == "shift" else (c["E"], c["cE"])
    ratio = lambda got, want, cond: np.abs(got - want) / (U_ROUND * cond)  # noqa: E731
    kE = max((ratio(f[:, 3], E, cE) - extra).max(), 0.0)
    kF = max((ratio(f[:, :3], c["F"], c["cF"][:, None]) - extra[:, None]).max(), 0.0)
    kW = max((ratio(v.T, c["W"], c["cW"][:, None]) - extra[:, None]).max(), 0.0)
    ng = c["Wg"].shape[0]
    tot = np.array([v[:, c["group"] == g].sum(axis=1) for g in range(ng)])
    cond = np.array([c["cW"][c["group"] == g].sum() for g in range(ng)])
    gextra = np.array([extra[c["group"] == g].max() for g in range(ng)])
    kWg = max((ratio(tot, c["Wg"], cond[:, None]) - gextra[:, None]).max(), 0.0)
    return float(kE), float(kF), float(kW), float(kWg)


if __name__ == "__main__":
    data = to_bytes(build())
    if "--check" in sys.argv:
        with open(OUT, "rb") as fh:
            same = fh.read() == data
        print("regenerated fixture is byte-identical: %s (%d bytes)" % (same, len(data)))
        arrays, meta = load()
        for key, ks in oracle_constants(arrays, meta).items():
            print("%-22s %d %-6s " % key + "  ".join("%8.2f" % x for x in ks))
        sys.exit(0 if same else 1)
    with open(OUT, "wb") as fh:
        fh.write(data)
    print("wrote %s (%d bytes)" % (OUT, len(data)))
