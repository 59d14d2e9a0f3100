"""Every evaluator path on the GPU against the arbitrary-precision closed forms of tests/golden/evaluator_cases.npz.

The fixture (tests/golden/make_evaluator_cases.py) gives per point U, F = -U' and a scale cond = sum |T_k| + |r U'| (one
derivative up for the force). Every point runs through every path that evaluates it, and per point

    |got - mp| <= B u cond,   u = 2^-53,   B = max(4 K_REF, 8) + R

* K_REF (tests/test_evaluator_cases.py) is the CPU oracle's own constant on the same set, mode and quantity -- the
  reference formula's loss. The factor 4 covers what legitimately differs in the kernels: FMA contraction, refined
  v_rcp_f64 / v_rsq_f64 (<= 1 ulp each, azp_device.hpp) instead of IEEE division and square root, another factorisation;
  each adds a rounding or two on a term and stays far below a lost digit.
* The floor 8 is the number of rounded operations on the dominant term of the short evaluators (evaluators.hpp:
  EvalPLJ::eval's r^-12 term: rcp, two products for r^-6, the fma with c12, two products with r^-2 r^-6, the scale,
  then the product with dx -- eight).
* R is non-zero only where the code documents a single-Newton reciprocal: the tile kernel's single-type PerturbedLJ
  path without xplor (EvalPLJ::rcp4 / fast_rcp1, relative error 2e-15 ~ 18 u by the code's own statement), which enters
  at the 7th power in the force and the 6th in the energy: R = 126 and 108.
* Sums over a cluster's neighbours add the neighbour count to B.

* DPDConservative at its three cutoff points, where K_REF is the two-term energy formula's own 2^52, is held to an
  absolute allowance reasoned from the formula as well (make_evaluator_cases.dpd_cutoff_allowance: 8 A r_c u).
* Every planned launch asserts from the plan info and the launch record that a tile instance ran.

Points the fixture marks as not evaluated (r >= r_cut, A = 0, epsilon = 0) must be exact zeros. No point is skipped.
Run with -s to see the measured constants next to K_REF (recorded in DESIGN.md)."""

import numpy as np
import pytest

import helpers as H
from azplugins_amd import _lib
from azplugins_amd import synthetic as syn
from test_evaluator_cases import K_REF, generator
from test_gpu_kernel_instances import _tile_lds, _xtiled_lds

pytestmark = pytest.mark.gpu

G = generator()
ARR, META = G.load()
ISO = ["PerturbedLennardJones", "Hertz", "ExpandedYukawa", "Colloid", "DPDConservative"]
MODES = ["none", "shift", "xplor"]
HOW = {"tpp1": dict(tpp=1), "tpp8": dict(tpp=8), "planned": dict(planned=True)}
R_SINGLE_NEWTON = (108.0, 126.0)  # energy (6th power of the reciprocal), force (7th)
SW, ED = slice(0, G.N_SWEEP), slice(G.N_SWEEP, None)


def bar(k_ref, r=0.0):
    return max(4.0 * k_ref, 8.0) + r


def report(what, got, bars, refs, fails):
    """Print the measured constants of one launch; a miss is recorded, and the test fails once all its launches ran."""
    print("%-46s " % what + "  ".join("%9.3g (K_REF %-8.3g B %-6.3g)" % t for t in zip(got, refs, bars)))
    if not all(g <= b for g, b in zip(got, bars)):
        fails.append((what, tuple(float("%.4g" % g) for g in got), tuple(bars)))


def assert_tile_ran(info, lds_bytes):
    """A *_planned entry point runs the generic kernel when its plan is invalid: the plan must be valid and the launch
    record's dynamic LDS must be the tile instance's layout, or the test would repeat the generic one."""
    launch = _lib.last_launch()
    assert info["valid"] == 1 and launch["lds_bytes"] == lds_bytes, (info, launch, lds_bytes)


def launch_pairs(oracle, name, ks, mode, how):
    """Sets ``ks`` of an evaluator in one launch (several: one type per set); returns the (2 * 131, 4) block per set."""
    sets = [META["pair"][name][k] for k in ks]
    T = len(ks)
    r = np.concatenate([ARR["%s.%d.r" % (name, k)] for k in ks])
    pos, L, nl = H._isolated_pairs(r)
    n = G.N_SWEEP + 3
    assert pos.shape[0] == 2 * n * T and 2 * n <= 2 * 131
    pos = syn.pos4(pos[:, :3], np.repeat(np.arange(T), 2 * n))
    packed = [oracle.pack_pair_params(name, m["params"]) for m in sets]
    params = np.array([packed[i if i == j else 0] for i in range(T) for j in range(T)])
    r_cut = np.array([[sets[i if i == j else 0]["r_cut"] for j in range(T)] for i in range(T)])
    r_on = np.array([[sets[i if i == j else 0]["r_on"] for j in range(T)] for i in range(T)]) if mode == "xplor" else 0.0
    info = {}
    f = H.gpu_pair_forces(name, pos, (L, (0, 0, 0), (0, 0, 0)), nl, params, r_cut, r_on, mode, ntypes=T,
                          r_list_max=1.06 * r_cut.max(), plan_info=info, **HOW[how])
    if how == "planned":
        assert_tile_ran(info, _tile_lds(info["lds_slots"], T, name))
    return [f[2 * n * i:2 * n * (i + 1)] for i in range(T)]


def check_pair_set(name, k, mode, how, f, single, fails):
    m = META["pair"][name][k]
    U, F, cU, cF, ev = G.pair_expect(ARR, m, name, k, mode)
    assert not f[np.repeat(~ev, 2)].any(), (name, k, mode, how, "not evaluated, not zero")
    assert not f[:, 1:3].any()
    got_f = np.stack([-f[0::2, 0], f[1::2, 0]])  # the particle at -r/2 has dx = -r
    got_u = 2.0 * np.stack([f[0::2, 3], f[1::2, 3]])
    got = (G._k(got_u[:, SW], U[SW], cU[SW]), G._k(got_f[:, SW], F[SW], cF[SW]),
           G._k(got_u[:, ED], U[ED], cU[ED]), G._k(got_f[:, ED], F[ED], cF[ED]))
    if name == "DPDConservative":  # K_REF at the cutoff is the two-term formula's 2^52: an absolute allowance instead
        dU, dF = G.dpd_cutoff_allowance(m, ARR["%s.%d.r" % (name, k)][ED], mode)
        assert (np.abs(got_u[:, ED] - U[ED]) <= 8 * G.U_ROUND * cU[ED] + dU).all(), (name, k, mode, how, "energy at the cutoff")
        assert (np.abs(got_f[:, ED] - F[ED]) <= 8 * G.U_ROUND * cF[ED] + dF).all(), (name, k, mode, how, "force at the cutoff")
    refs = K_REF["%s.%d.%s" % (name, k, mode)]
    newton = name == "PerturbedLennardJones" and how == "planned" and single and mode != "xplor"
    rr = R_SINGLE_NEWTON * 2 if newton else (0.0,) * 4
    report("%s.%d %s %s%s" % (name, k, mode, how, "" if single else " types"), got, [bar(a, b) for a, b in zip(refs, rr)], refs, fails)


@pytest.mark.parametrize("how", list(HOW))
@pytest.mark.parametrize("name", ISO)
def test_isotropic_sets(oracle, name, how):
    """Each parameter set on its own (one type: coefficients in registers; planned PerturbedLJ: the split-energy path)
    in modes none, shift and xplor: 131 isolated pairs, both particles of each."""
    fails = []
    for k in range(len(META["pair"][name])):
        for mode in MODES:
            check_pair_set(name, k, mode, how, launch_pairs(oracle, name, [k], mode, how)[0], True, fails)
    assert not fails, fails


@pytest.mark.parametrize("how", ["tpp1", "planned"])
@pytest.mark.parametrize("name", ISO)
def test_isotropic_sets_as_types(oracle, name, how):
    """All parameter sets of an evaluator in one launch, one type per set: the coefficient table in LDS, per-type-pair
    cutoffs and r_on."""
    ks = list(range(len(META["pair"][name])))
    fails = []
    for mode in MODES:
        for k, f in zip(ks, launch_pairs(oracle, name, ks, mode, how)):
            check_pair_set(name, k, mode, how, f, False, fails)
    assert not fails, fails


@pytest.mark.parametrize("how", list(HOW))
def test_plj_clusters(oracle, how):
    """32 isolated groups of 5 to 9 particles (4 to 8 neighbours per row: full and partly padded batches of four; groups
    0..15 lie wholly beyond 2^(1/6) sigma): per-particle force and energy sums, the virial per particle and its total
    per group (-dU / d strain, from the physics alone: sign, the 1/2 per particle, the order xx xy xz yy yz zz)."""
    c = G.cluster_case(ARR, META)
    params = oracle.pack_pair_params("PerturbedLennardJones", c["params"])
    fails = []
    for mode in ("none", "shift"):
        info = {}
        f, v = H.gpu_pair_forces("PerturbedLennardJones", c["pos"], (c["L"], (0, 0, 0), (0, 0, 0)), c["nl"], params, c["r_cut"],
                                 mode=mode, virial=True, r_list_max=1.06 * c["r_cut"], plan_info=info, **HOW[how])
        rr = (0.0,) * 4
        if how == "planned":
            assert_tile_ran(info, _tile_lds(info["lds_slots"], 1, "PerturbedLennardJones"))
            rr = (R_SINGLE_NEWTON[0],) + (R_SINGLE_NEWTON[1],) * 3
        print("clusters %s %s: constants before the neighbour count is taken off: " % (mode, how)
              + "  ".join("%.3g" % x for x in G.cluster_constants(c, f, v, mode)))
        got = G.cluster_constants(c, f, v, mode, extra=c["n_neigh"])  # per particle: ratio - neighbours, at least 0
        refs = K_REF["clusters.0.%s" % mode]
        report("clusters %s %s" % (mode, how), got, [bar(a, b) for a, b in zip(refs, rr)], refs, fails)
    assert not fails, fails


@pytest.mark.parametrize("how", ["tpp1", "planned"])
def test_two_patch_morse(oracle, how):
    """64 pairs, repulsion off and on, modes none and shift: energy, force and the torques on both particles, on both
    rows of each pair. The pairs along x include r = r_cut exactly, which the anisotropic evaluator evaluates."""
    dr, qi, qj = ARR["tpm.dr"], ARR["tpm.qi"], ARR["tpm.qj"]
    n = dr.shape[0]
    xyz = np.zeros((2 * n, 3))
    xyz[0::2, 1] = xyz[1::2, 1] = (np.arange(n) - n // 2) * 40.0  # j at (0, y_k, 0), i = j + dr: differences are exact
    xyz[0::2] += dr
    q = np.empty((2 * n, 4))
    q[0::2], q[1::2] = qi, qj
    nl = (np.ones(2 * n, dtype=np.uint32), np.arange(2 * n, dtype=np.uint64), np.arange(2 * n, dtype=np.uint32) ^ 1)
    L = np.array([200.0, (n + 2) * 40.0, 200.0])
    assert np.array_equal(xyz[0::2] - xyz[1::2], dr)
    fails = []
    for k, m in enumerate(META["tpm"]):
        params = oracle.pack_pair_params("TwoPatchMorse", m["params"])
        g = lambda key: (G.unpack_scale if key[0] == "c" else np.asarray)(ARR["tpm.%d.%s" % (k, key)])  # noqa: E731
        for mode in ("none", "shift"):
            info = {}
            f, tq = H.gpu_aniso_forces(syn.pos4(xyz), q, (L, (0, 0, 0), (0, 0, 0)), nl, params, m["r_cut"], mode=mode,
                                       r_list_max=1.06 * m["r_cut"], plan_info=info, **HOW[how])
            if how == "planned":  # (1,664 staged slots run the 2,048-slot instance)
                assert_tile_ran(info, _xtiled_lds("tpm", 2048 if info["lds_slots"] == 1664 else info["lds_slots"], 1))
            E, cE = (g("Esh"), g("cEsh")) if mode == "shift" else (g("E"), g("cE"))
            got = (G._k(2.0 * np.stack([f[0::2, 3], f[1::2, 3]]), E, cE),
                   G._k(np.stack([f[0::2, :3], -f[1::2, :3]]), g("F"), g("cF")),
                   G._k(tq[0::2, :3], g("Ti"), g("cTi")), G._k(tq[1::2, :3], g("Tj"), g("cTj")))
            refs = K_REF["TwoPatchMorse.%d.%s" % (k, mode)]
            report("TwoPatchMorse.%d %s %s" % (k, mode, how), got, [bar(a) for a in refs], refs, fails)
    assert not fails, fails


@pytest.mark.parametrize("name", ["DoubleWell", "Quartic"])
def test_bonds(oracle, name):
    """Both parameter sets of each bond potential (Quartic: delta = 0 and delta != 0), with r at the WCA edge and at r_0."""
    fails = []
    for k, m in enumerate(META["bond"][name]):
        r = ARR["%s.%d.r" % (name, k)]
        pos, L, _ = H._isolated_pairs(r)
        bonds = np.arange(2 * r.size).reshape(-1, 2)
        f, flag = H.gpu_bond_forces(name, pos, (L, (0, 0, 0), (0, 0, 0)), bonds, np.zeros(r.size, dtype=np.uint32),
                                    oracle.pack_bond_params(name, m["params"]))
        assert flag == 0 and not f[:, 1:3].any()
        got = (G._k(2.0 * np.stack([f[0::2, 3], f[1::2, 3]]), ARR["%s.%d.U" % (name, k)], G.unpack_scale(ARR["%s.%d.cU" % (name, k)])),
               G._k(np.stack([-f[0::2, 0], f[1::2, 0]]), ARR["%s.%d.F" % (name, k)], G.unpack_scale(ARR["%s.%d.cF" % (name, k)])))
        refs = K_REF["%s.%d.bond" % (name, k)]
        report("%s.%d" % (name, k), got, [bar(a) for a in refs], refs, fails)
    assert not fails, fails
