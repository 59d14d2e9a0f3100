"""The CPU oracle against the arbitrary-precision closed forms of tests/golden/evaluator_cases.npz.

Every other evaluator test compares a kernel with the oracle; this one is the oracle's own independent pin. The fixture
(tests/golden/make_evaluator_cases.py) holds every evaluator's U and F = -U' from the published definitions at 60 digits,
with a scale per point, cond = sum |T_k| + |r U'| (and the same one derivative up for the force): what rounding every
additive term once and rounding r costs. K is max |oracle - mp| / (u cond) over a set, u = 2^-53.

K_REF holds the constants measured with `make_evaluator_cases.py --check`, each rounded up to the next power of two;
the oracle must stay inside them. Isotropic pairs have four per set and mode: energy and force over the 128-point sweep,
then over the three points at the cutoff (r_cut (1 - 1e-9), the double below r_cut, r_cut itself), kept apart so that
what a formula loses next to its cutoff does not widen the bar of the well and the tail. Bonds: energy, force.
TwoPatchMorse: energy, force, torque on i, torque on j. Clusters: energy, force, virial per particle, virial per group.

What the constants say (nothing here disagrees on a convention; the fixture and the oracle agree on the sign of the
TwoPatchMorse torques, on the force of the unshifted energy, on the virial's sign, its 1/2 per particle and its
component order, and on HOOMD's XPLOR form):
* Colloid colloid-colloid loses digits in the reference's own arrangement: K ~ 9 for a = 1.5 / 0.75 and ~ 55 for
  a = 0.15 / 0.19, sigma = 0.35 (the four repulsive quotients cancel among themselves).
* XPLOR forces of the colloid sets reach K ~ 1800: S' multiplies the energy's ERROR, which follows sum |T_k|, while the
  scale carries |S' U| with the much smaller U.
* DPDConservative's energy, A (r_c - r) - A (r_c^2 - r^2) / (2 r_c) with r = 1 / (1 / sqrt(r^2)), keeps an absolute
  error of A r u while U vanishes like (r_c - r)^2: K ~ 30 over the sweep and unbounded (2^52) at the double below
  r_cut. The scale carries |r U'|, not sum |r T_k'|, so this is the reference formula's own loss and sits in K_REF.

Each cap is the measured constant rounded up to the next power of two, so a few sit within a few percent of it
(Colloid.0 force 0.97 / 1, Quartic.0 force 3.91 / 4, ExpandedYukawa.0 energy 0.50 / 0.5). The oracle calls the host
libm's exp, log and pow: on another libm a constant can cross its cap without any change here. Re-measure with --check
before suspecting the code.

The closed forms themselves are checked against a second source: the reference's known answers
(tests/golden/reference_cases.json) to the digits the reference asserts them with."""

import importlib.util
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def generator():
    spec = importlib.util.spec_from_file_location("make_evaluator_cases", os.path.join(GOLDEN, "make_evaluator_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


K_REF = {
    "Colloid.0.none": (1.0, 1.0, 1.0, 1.0),
    "Colloid.0.shift": (1.0, 1.0, 1.0, 1.0),
    "Colloid.0.xplor": (1.0, 1.0, 0.5, 0.5),
    "Colloid.1.none": (1.0, 1.0, 0.5, 1.0),
    "Colloid.1.shift": (1.0, 1.0, 0.5, 1.0),
    "Colloid.1.xplor": (1.0, 1.0, 0.5, 0.5),
    "Colloid.2.none": (0.5, 0.5, 0.25, 0.25),
    "Colloid.2.shift": (0.5, 0.5, 0.25, 0.25),
    "Colloid.2.xplor": (1.0, 0.5, 0.25, 0.25),
    "Colloid.3.none": (8.0, 8.0, 16.0, 16.0),
    "Colloid.3.shift": (8.0, 8.0, 16.0, 16.0),
    "Colloid.3.xplor": (8.0, 64.0, 0.5, 0.5),
    "Colloid.4.none": (64.0, 64.0, 32.0, 64.0),
    "Colloid.4.shift": (64.0, 64.0, 32.0, 64.0),
    "Colloid.4.xplor": (64.0, 2048.0, 0.5, 0.5),
    "Colloid.5.none": (1.0, 2.0, 1.0, 0.0),
    "Colloid.5.shift": (1.0, 2.0, 0.25, 0.0),
    "Colloid.5.xplor": (0.5, 2.0, 0.5, 0.5),
    "Colloid.6.none": (4.0, 4.0, 4.0, 4.0),
    "Colloid.6.shift": (4.0, 4.0, 4.0, 4.0),
    "Colloid.6.xplor": (4.0, 16.0, 0.5, 0.5),
    "Colloid.7.none": (0.0, 0.0, 0.0, 0.0),
    "Colloid.7.shift": (0.0, 0.0, 0.0, 0.0),
    "Colloid.7.xplor": (0.0, 0.0, 0.0, 0.0),
    "DPDConservative.0.none": (32.0, 2.0, 4503599627370496.0, 0.5),
    "DPDConservative.0.shift": (32.0, 2.0, 4503599627370496.0, 0.5),
    "DPDConservative.0.xplor": (32.0, 32.0, 4503599627370496.0, 2251799813685248.0),
    "DPDConservative.1.none": (32.0, 1.0, 4503599627370496.0, 0.5),
    "DPDConservative.1.shift": (32.0, 1.0, 4503599627370496.0, 0.5),
    "DPDConservative.1.xplor": (32.0, 32.0, 4503599627370496.0, 2251799813685248.0),
    "DPDConservative.2.none": (0.0, 0.0, 0.0, 0.0),
    "DPDConservative.2.shift": (0.0, 0.0, 0.0, 0.0),
    "DPDConservative.2.xplor": (0.0, 0.0, 0.0, 0.0),
    "DoubleWell.0.bond": (2.0, 1.0),
    "DoubleWell.1.bond": (2.0, 2.0),
    "ExpandedYukawa.0.none": (0.5, 1.0, 0.0, 0.25),
    "ExpandedYukawa.0.shift": (0.5, 1.0, 0.125, 0.25),
    "ExpandedYukawa.0.xplor": (2.0, 2.0, 0.5, 0.5),
    "ExpandedYukawa.1.none": (1.0, 2.0, 1.0, 1.0),
    "ExpandedYukawa.1.shift": (1.0, 2.0, 0.5, 1.0),
    "ExpandedYukawa.1.xplor": (2.0, 2.0, 0.5, 0.5),
    "ExpandedYukawa.2.none": (1.0, 2.0, 1.0, 1.0),
    "ExpandedYukawa.2.shift": (2.0, 2.0, 1.0, 1.0),
    "ExpandedYukawa.2.xplor": (4.0, 4.0, 0.5, 0.5),
    "Hertz.0.none": (4.0, 4.0, 0.5, 0.5),
    "Hertz.0.shift": (4.0, 4.0, 0.5, 0.5),
    "Hertz.0.xplor": (4.0, 4.0, 0.25, 0.25),
    "Hertz.1.none": (4.0, 4.0, 0.5, 0.5),
    "Hertz.1.shift": (4.0, 4.0, 0.5, 0.5),
    "Hertz.1.xplor": (4.0, 4.0, 0.25, 0.25),
    "Hertz.2.none": (0.0, 0.0, 0.0, 0.0),
    "Hertz.2.shift": (0.0, 0.0, 0.0, 0.0),
    "Hertz.2.xplor": (0.0, 0.0, 0.0, 0.0),
    "PerturbedLennardJones.0.none": (1.0, 1.0, 1.0, 1.0),
    "PerturbedLennardJones.0.shift": (1.0, 1.0, 0.5, 1.0),
    "PerturbedLennardJones.0.xplor": (1.0, 1.0, 0.5, 0.5),
    "PerturbedLennardJones.1.none": (2.0, 1.0, 0.0, 0.0),
    "PerturbedLennardJones.1.shift": (2.0, 1.0, 0.0, 0.0),
    "PerturbedLennardJones.1.xplor": (2.0, 1.0, 0.0, 0.0),
    "PerturbedLennardJones.2.none": (1.0, 1.0, 0.25, 0.5),
    "PerturbedLennardJones.2.shift": (1.0, 1.0, 0.25, 0.5),
    "PerturbedLennardJones.2.xplor": (1.0, 1.0, 0.5, 0.5),
    "Quartic.0.bond": (1.0, 4.0),
    "Quartic.1.bond": (0.5, 4.0),
    "TwoPatchMorse.0.none": (1.0, 2.0, 2.0, 2.0),
    "TwoPatchMorse.0.shift": (1.0, 2.0, 2.0, 2.0),
    "TwoPatchMorse.1.none": (2.0, 2.0, 2.0, 2.0),
    "TwoPatchMorse.1.shift": (2.0, 2.0, 2.0, 2.0),
    "clusters.0.none": (1.0, 1.0, 1.0, 0.5),
    "clusters.0.shift": (1.0, 1.0, 1.0, 0.5),
}


def k_ref(key):
    return K_REF["%s.%d.%s" % key]


def next_pow2(k):
    return 0.0 if k == 0 else 2.0 ** np.ceil(np.log2(k))


@pytest.fixture(scope="module")
def measured(oracle):
    G = generator()
    arrays, meta = G.load()
    return G.oracle_constants(arrays, meta)


def test_k_ref_covers_every_set(measured):
    assert sorted("%s.%d.%s" % key for key in measured) == sorted(K_REF)
    for ks in K_REF.values():
        assert all(k == next_pow2(k) for k in ks)


def test_oracle_within_k_ref(measured):
    """Every evaluator of the oracle (eval_pair, the pair loop in xplor mode, eval_bond, eval_tpm, pair_forces with the
    virial on the clusters) stays within its committed constant on every set, mode and quantity."""
    bad = []
    for key, ks in sorted(measured.items()):
        ref = k_ref(key)
        print("%-22s %d %-6s " % key + "  ".join("%10.3g / %-8.3g" % (k, r) for k, r in zip(ks, ref)))
        if any(k > r for k, r in zip(ks, ref)):
            bad.append((key, ks, ref))
    assert not bad, bad


def test_fixture_shape():
    """128 sweep points and the three cutoff points per pair set; what is not evaluated is exact zeros; below 200 KB."""
    G = generator()
    arrays, meta = G.load()
    assert os.path.getsize(G.OUT) < 200 * 1000
    for name, sets in meta["pair"].items():
        for k, m in enumerate(sets):
            r = arrays["%s.%d.r" % (name, k)]
            assert r.size == G.N_SWEEP + 3 and r[-1] == m["r_cut"] and r[-2] == np.nextafter(m["r_cut"], 0.0)
            assert r[:G.N_SWEEP].min() == m["r_min"] and r[:G.N_SWEEP].max() < 1.05 * m["r_cut"]
            for mode in ("none", "shift", "xplor"):
                U, F, cU, cF, ev = G.pair_expect(arrays, m, name, k, mode)
                assert not U[~ev].any() and not F[~ev].any() and not ev[r >= m["r_cut"]].any()
                assert ev[r < m["r_cut"]].all() or not ev.any()  # (A = 0, epsilon = 0: never evaluated)
    c = G.cluster_case(arrays, meta)
    assert c["n_neigh"].min() == 4 and c["n_neigh"].max() == 8 and c["Wg"].shape == (32, 6)
    # separations span [0.85, 1.05 r_cut): every group lists a pair in [r_cut, 1.05 r_cut), the first group at r_cut exactly
    xyz, r_cut, seps = c["pos"][:, :3], c["r_cut"], []
    for g in range(32):
        p = xyz[c["group"] == g]
        d = np.sqrt(((p[:, None] - p[None]) ** 2).sum(axis=2))[np.triu_indices(len(p), 1)]
        assert r_cut <= d.max() < 1.05 * r_cut and d.min() >= (1.13 if g < 16 else 0.8499)
        seps.append(d)
    assert seps[0].max() == r_cut and max(d.max() for d in seps) > 1.04 * r_cut
    assert min(d.min() for d in seps[:16]) > 2.0 ** (1.0 / 6.0) and abs(min(d.min() for d in seps[16:]) - 0.85) < 1e-8


def test_dpd_cutoff_points_absolute(oracle):
    """K_REF of DPDConservative's energy at the cutoff is 2^52 (the two-term formula's own loss), which leaves those
    three points unchecked; an absolute allowance reasoned from the formula (make_evaluator_cases.dpd_cutoff_allowance)
    checks them: 8 u cond + 8 A r_c u, through S and S' in xplor mode."""
    G = generator()
    arrays, meta = G.load()
    for k, m in enumerate(meta["pair"]["DPDConservative"]):
        r = arrays["DPDConservative.%d.r" % k][G.N_SWEEP:]
        for mode in ("none", "shift", "xplor"):
            U, F, cU, cF, ev = (a[G.N_SWEEP:] for a in G.pair_expect(arrays, m, "DPDConservative", k, mode))
            dU, dF = G.dpd_cutoff_allowance(m, r, mode)
            for i, x in enumerate(r):
                if mode == "xplor":
                    f, e = G.oracle_xplor(oracle, "DPDConservative", m["params"], x, m["r_cut"], m["r_on"])
                else:
                    ok, fdr, e = oracle.eval_pair("DPDConservative", m["params"], x, m["r_cut"], mode == "shift")
                    f = fdr * x
                assert abs(e - U[i]) <= 8 * G.U_ROUND * cU[i] + dU[i], (k, mode, x, e, U[i])
                assert abs(f - F[i]) <= 8 * G.U_ROUND * cF[i] + dF[i], (k, mode, x, f, F[i])


def test_closed_forms_match_reference_known_answers(reference_cases):
    """The second source: the fixture's closed forms give the reference's own known answers to the four decimals the
    reference asserts them with (and to 1e-9 relative where the reference quotes full doubles)."""
    G = generator()
    mp = G._mp()

    def close(got, want):
        got, want = float(got), float(want)
        tol = 1.5e-4 if len(repr(abs(want))) < 12 else 1e-9 * abs(want)
        assert abs(got - want) <= tol, (got, want)

    n = 0
    for case in reference_cases["pair"]:
        name = "DPDConservative" if case["potential"] == "DPDGeneralWeight" else case["potential"]
        r, rc = mp.mpf(case["distance"]), mp.mpf(case["r_cut"])
        terms = G.pair_terms(mp, name, case["params"], r, case["r_cut"])
        if terms is None or not r < rc:
            assert case["energy"] == 0 and case["force"] == 0
            continue
        U, F, _, _ = G.point(mp, terms, r)
        if case["shift"]:
            U -= mp.fsum(t(rc) for t in G.pair_terms(mp, name, case["params"], rc, case["r_cut"]))
        close(U, case["energy"])
        close(F, case["force"])
        n += 1
    for case in reference_cases["bond"]:
        r = mp.mpf(case["distance"])
        U, F, _, _ = G.point(mp, G.bond_terms(mp, case["potential"], case["params"], r), r)
        close(U, case["energy"])
        close(F, case["force"])
        n += 1
    assert n >= 30
    case = reference_cases["aniso"][0]
    x = np.array(reference_cases["aniso_setup"]["positions"], dtype=np.float64)
    q = np.array(reference_cases["aniso_setup"]["orientations"], dtype=np.float64)
    out, _ = G.tpm_set(mp, case["params"], (x[1] - x[0])[None], q[1:2], q[0:1])  # i = the second particle: forces == [-f, f]
    close(out["E"][0], case["energy"])
    for a in range(3):
        close(out["F"][0, a], case["force"][a])
        close(out["Ti"][0, a], case["torque"][a])
        close(out["Tj"][0, a], case["torque"][a])
