"""compute.PressureProfile without a GPU: the numpy restatement against its own rules and against hand cases, the host
function pressure_profile_quantities, and the argument checks.

The restatement (tests/pressure_profile_ref.py) is what tests/test_gpu_pressure_profile.py holds the kernels to, so it is
pinned here first: the weights of a pair sum to 1, the integer row sums to the pairs' virials, two-particle cases with
the bins and weights worked out by hand, and the translation rule (one bin width on dyadic coordinates rotates the
profile by one bin, exactly)."""

from fractions import Fraction

import numpy as np
import pytest

import pressure_profile_ref as R
from azplugins_amd import _lib, angle, compute, dihedral, external, nlist, pair

GRID = 2.0 ** -12
UNIT = {"eval": lambda rsq, key: (True, 1.0), "r_max": 100.0}  # force_divr = 1: w_ab = d_a d_b


def dyadic_points(n, L, seed):
    rng = np.random.default_rng(seed)
    return np.round((rng.random((n, 3)) - 0.5) * np.asarray(L) / GRID) * GRID


def plj(oracle, r_cut=2.5, mode="none", r_on=2.0):
    p = dict(epsilon=1.0, sigma=1.0, attraction_scale_factor=0.5)
    return {"eval": R.oracle_pair(oracle, "PerturbedLennardJones", [[p]], [[r_cut]], [[r_on]], mode), "r_max": r_cut}


@pytest.fixture(scope="module")
def configurations(oracle):
    """(Accumulator, description) of a few random configurations: every axis, wrapped and explicit ranges, a tilt."""
    out = []
    L = (8.0, 8.0, 8.0)
    max_term = 2.0 ** 40  # (random points come close: nothing is to be refused here)
    shift, _ = compute.pressure_profile_shift(24, max_term)
    for seed, axis, nb, kw in ((1, 2, 16, {}), (2, 0, 7, {}), (3, 1, 64, {}), (4, 2, 5, dict(lower=-1.0, upper=2.5)),
                               (5, 2, 16, dict(tilt=(0.25, -0.5, 0.125))), (6, 2, 3, dict(periodic=(True, True, False)))):
        pos = dyadic_points(24, L, seed)
        tags = np.random.default_rng(seed).permutation(24)
        acc = R.profile(pos, np.zeros(24, dtype=int), tags, L, axis, nb, shift, max_term, [plj(oracle)], **kw)
        assert acc.pairs > 20 and acc.over == 0
        out.append((acc, kw))
    return out


def test_weights_sum_to_one(configurations):
    """Every pair of the wrapped configurations: sum_k lambda_k = 1 to the rounding of the quotients and of the sum."""
    seen = 0
    for acc, kw in configurations:
        if "lower" in kw or "periodic" in kw:
            continue  # (parts of a line outside the range are dropped there)
        for s in acc.lambda_sums:
            assert abs(s - 1.0) <= 70 * 2.0 ** -52
            seen += 1
    assert seen > 100


def test_row_sums_to_the_pair_virials(configurations):
    """sum_k row_k 2^-shift against sum_pairs w_ab, per component: within (terms) 2^-(shift + 1)."""
    for acc, kw in configurations:
        if "lower" in kw or "periodic" in kw:
            continue
        row = acc.row()
        for c in range(6):
            total = Fraction(sum(row[c:6 * acc.nb:6]), 2 ** acc.shift)
            assert abs(total - Fraction(acc.w_total[c])) <= Fraction(int(acc.n_terms[:, c].sum()), 2 ** (acc.shift + 1))
        assert row[-4] == acc.pairs and row[-3] == acc.terms == int(acc.n_terms.sum()) and row[-1] == acc.shift


def two(z_i, z_j, nb=8, L=8.0, x=0.5, tags=(0, 1), **kw):
    """Two particles at (0, 0, z_i) and (x, 0, z_j), force_divr = 1, profile along z on [-L/2, L/2)."""
    pos = np.array([[0.0, 0.0, z_i], [x, 0.0, z_j]])
    return R.profile(pos, [0, 0], tags, (L, L, L), 2, nb, 40, 1024.0, [UNIT], **kw)


def zz(acc):
    return np.array(acc.row()[5:6 * acc.nb:6], dtype=np.float64) * 2.0 ** -acc.shift


def test_pair_inside_one_bin():
    acc = two(0.25, 0.75)
    assert acc.pairs == 1 and acc.terms == 6
    np.testing.assert_array_equal(zz(acc), [0, 0, 0, 0, 0.25, 0, 0, 0])
    # xx, xz of the same bin: d = r_0 - r_1 = (-0.5, 0, -0.5)
    assert acc.row()[6 * 4 + 0] == 2 ** 38 and acc.row()[6 * 4 + 2] == 2 ** 38 and acc.row()[6 * 4 + 1] == 0


def test_pair_across_three_bins():
    acc = two(-0.5, 1.5)  # from -0.5 to 1.5: half of bin 3, bin 4, half of bin 5; d_z = -2, w_zz = 4
    np.testing.assert_array_equal(zz(acc), [0, 0, 0, 1.0, 2.0, 1.0, 0, 0])
    assert acc.terms == 18


def test_pair_across_the_periodic_face():
    acc = two(3.5, -3.75)  # minimum image d_z = -0.75: from 3.5 over the face to 4.25 = -3.75
    assert acc.pairs == 1
    w = 0.75 * 0.75
    np.testing.assert_allclose(zz(acc), [w / 3, 0, 0, 0, 0, 0, 0, 2 * w / 3], rtol=4 * 2.0 ** -52, atol=2.0 ** -40)
    # the same pair seen from the other particle (the tags swapped): the segment starts at -3.75 and leaves downwards
    np.testing.assert_allclose(zz(two(3.5, -3.75, tags=(1, 0))), zz(acc), rtol=4 * 2.0 ** -52, atol=2.0 ** -40)
    # an explicit range drops what lies outside it
    cut = two(3.5, -3.75, lower=-4.0, upper=4.0)
    np.testing.assert_allclose(zz(cut), [0, 0, 0, 0, 0, 0, 0, 2 * w / 3], rtol=4 * 2.0 ** -52, atol=2.0 ** -40)


def test_pair_with_no_extent_along_the_axis():
    acc = two(1.25, 1.25)  # d_z = 0 exactly: whole into the bin of z1, and w_zz = 0
    row = acc.row()
    assert acc.terms == 6 and row[6 * 5 + 0] == 2 ** 38 and row[6 * 5 + 5] == 0
    assert sum(abs(v) for v in row[:48]) == 2 ** 38


def test_end_point_on_an_edge():
    acc = two(0.5, 2.0)  # ends exactly on the edge between bins 5 and 6: bin 6 gets nothing
    np.testing.assert_allclose(zz(acc), [0, 0, 0, 0, 0.75, 1.5, 0, 0], rtol=4 * 2.0 ** -52)
    assert acc.terms == 12
    acc = two(1.0, 1.5)  # starts on an edge, inside one bin
    np.testing.assert_array_equal(zz(acc), [0, 0, 0, 0, 0, 0.25, 0, 0])


def test_refused_terms_are_counted():
    pos = np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.5]])
    acc = R.profile(pos, [0, 0], [0, 1], (8.0,) * 3, 2, 8, 40, 0.25, [UNIT])  # |w| = 0.25: not below max_term
    assert acc.over == 3 and acc.terms == 3 and acc.pairs == 1  # (xx, xz, zz are refused; xy, yy, yz are 0 and are added)
    assert not any(acc.row()[:48])


def test_translation_rotates_the_profile(oracle):
    """Every particle moved by one bin width (dyadic coordinates, wrapped back into the box): bin k becomes bin k + 1."""
    L, nb = (8.0, 8.0, 8.0), 16
    pos = dyadic_points(24, L, 11)
    tags = np.arange(24)
    shift, _ = compute.pressure_profile_shift(24, 1024.0)
    a = R.profile(pos, np.zeros(24, dtype=int), tags, L, 2, nb, shift, 1024.0, [plj(oracle)])
    moved = pos.copy()
    moved[:, 2] += 0.5
    moved[:, 2] = np.where(moved[:, 2] >= 4.0, moved[:, 2] - 8.0, moved[:, 2])
    b = R.profile(moved, np.zeros(24, dtype=int), tags, L, 2, nb, shift, 1024.0, [plj(oracle)])
    ra, rb = np.array(a.row()[:-4]).reshape(nb, 6), np.array(b.row()[:-4]).reshape(nb, 6)
    assert np.array_equal(np.roll(ra, 1, axis=0), rb) and a.row()[-4:] == b.row()[-4:]


def test_tags_not_rows_orient_a_pair(oracle):
    """A permutation of the rows that carries the tags leaves the row as it is."""
    L = (8.0, 8.0, 8.0)
    pos = dyadic_points(24, L, 12)
    tags = np.random.default_rng(3).permutation(24)
    shift, _ = compute.pressure_profile_shift(24, 1024.0)
    a = R.profile(pos, np.zeros(24, dtype=int), tags, L, 2, 16, shift, 1024.0, [plj(oracle, mode="xplor")])
    order = np.random.default_rng(4).permutation(24)
    b = R.profile(pos[order], np.zeros(24, dtype=int), tags[order], L, 2, 16, shift, 1024.0, [plj(oracle, mode="xplor")])
    assert a.row() == b.row()


# ---------------------------------------------------------------------------
# host function
# ---------------------------------------------------------------------------
def synthetic_rows(nb, shift, p_n, p_t, volume, n_types=1):
    """An integer row and kinetic rows of an ideal profile along z: P_zz = p_n, P_xx = P_yy = p_t per bin, a tenth of each
    kinetic (two particles of mass 1 per bin with velocities +-v: no streaming), the rest configurational."""
    row = np.zeros(6 * nb + 4, dtype=np.int64)
    kin = np.zeros((nb, _lib.THERMO_FIELD_NSUMS + n_types))
    for k in range(nb):
        for c, p in ((0, p_t[k]), (3, p_t[k]), (5, p_n[k])):
            row[6 * k + c] = int(round(0.9 * p * volume * 2.0 ** shift))
            kin[k, 5 + c] = 0.1 * p * volume
        kin[k, 0], kin[k, 1] = 2.0, 2.0
    row[-4:] = (10, 60, 0, shift)
    return row, kin


def test_quantities_of_a_synthetic_profile():
    nb, shift, volume, width = 8, 30, 2.0, 0.5
    p_t = np.array([1.0, 1.0, 0.5, 0.25, 0.25, 0.5, 1.0, 1.0])
    p_n = np.ones(nb)
    row, kin = synthetic_rows(nb, shift, p_n, p_t, volume)
    q = compute.pressure_profile_quantities(row, kin, np.full(nb, volume), 2, width, "subtract")
    np.testing.assert_allclose(q["normal_pressure"], p_n, rtol=1e-8)
    np.testing.assert_allclose(q["tangential_pressure"], p_t, rtol=1e-8)
    np.testing.assert_allclose(q["configurational_pressure_tensor"][:, 5], 0.9 * p_n, rtol=1e-8)
    np.testing.assert_allclose(q["kinetic_pressure_tensor"][:, 0], 0.1 * p_t, rtol=1e-12)
    np.testing.assert_allclose(q["pressure_tensor"], q["kinetic_pressure_tensor"] + q["configurational_pressure_tensor"])
    gamma = ((p_n - p_t) * width).sum()
    assert q["surface_tension"] == pytest.approx(gamma / 2, rel=1e-8)
    one = compute.pressure_profile_quantities(row, kin, np.full(nb, volume), 2, width, "subtract", interfaces=1)
    assert one["surface_tension"] == pytest.approx(gamma, rel=1e-8)
    assert (q["num_pairs"], q["num_terms"], q["overflow"]) == (10, 60, 0)
    # along x the roles change: P_N = P_xx = p_t
    x = compute.pressure_profile_quantities(row, kin, np.full(nb, volume), 0, width, "subtract")
    np.testing.assert_allclose(x["normal_pressure"], p_t, rtol=1e-8)
    np.testing.assert_allclose(x["tangential_pressure"], 0.5 * (p_t + p_n), rtol=1e-8)


def test_quantities_with_the_volumes_of_a_resized_box():
    """Rows recorded in boxes of different volume: each normalised with its own, and the sum with the summed volumes."""
    nb, shift = 4, 30
    row, kin = synthetic_rows(nb, shift, np.ones(nb), np.full(nb, 0.5), 2.0)
    rows, kins = np.stack([row, row]), np.stack([kin, kin])
    vols = np.array([np.full(nb, 2.0), np.full(nb, 4.0)])
    q = compute.pressure_profile_quantities(rows, kins, vols, 2, np.array([0.5, 1.0]), "keep")
    np.testing.assert_allclose(q["normal_pressure"][0], 1.0, rtol=1e-8)
    np.testing.assert_allclose(q["normal_pressure"][1], 0.5, rtol=1e-8)
    assert q["surface_tension"][0] == pytest.approx(0.5 * 0.5 * 4 / 2, rel=1e-8)
    assert q["surface_tension"][1] == pytest.approx(0.25 * 1.0 * 4 / 2, rel=1e-8)
    mean = compute.pressure_profile_quantities(rows.sum(axis=0), kins.sum(axis=0), vols.sum(axis=0), 2, 0.75, "keep", shift=shift)
    np.testing.assert_allclose(mean["normal_pressure"], 2.0 * 2.0 / 6.0, rtol=1e-8)


def test_quantities_refuse_bad_input():
    row, kin = synthetic_rows(4, 30, np.ones(4), np.ones(4), 1.0)
    for bad in (dict(axis=3), dict(interfaces=0), dict(interfaces=1.5), dict(streaming="drop")):
        kw = dict(axis=2, streaming="subtract", interfaces=2)
        kw.update(bad)
        with pytest.raises(_lib.AzpError):
            compute.pressure_profile_quantities(row, kin, np.ones(4), kw["axis"], 1.0, kw["streaming"], kw["interfaces"])
    with pytest.raises(_lib.AzpError):
        compute.pressure_profile_quantities(row[:-1], kin, np.ones(4), 2, 1.0)
    with pytest.raises(_lib.AzpError):
        compute.pressure_profile_quantities(row, kin[:3], np.ones(4), 2, 1.0)


def test_shift_leaves_room_for_the_stated_number_of_pairs():
    for n, max_term in ((2, 1024.0), (3, 1024.0), (65, 1024.0), (343, 1024.0), (2 ** 20, 1024.0), (2 ** 20 + 1, 1000.0), (100, 0.3)):
        shift, pair_bits = compute.pressure_profile_shift(n, max_term)
        assert 2 ** pair_bits >= 256 * n and 2 ** (pair_bits - 1) < 256 * max(n, 2)
        assert shift == 52 or max_term * 2.0 ** (shift + 1) * 2.0 ** pair_bits > 2.0 ** 63
        assert max_term * 2.0 ** shift * 2.0 ** pair_bits <= 2.0 ** 63
    assert compute.pressure_profile_shift(2 ** 20, 1024.0) == (25, 28)
    for bad in (0.0, -1.0, float("inf"), float("nan"), 2.0 ** 60):
        with pytest.raises(_lib.AzpError):
            compute.pressure_profile_shift(2 ** 20, bad)


# ---------------------------------------------------------------------------
# arguments
# ---------------------------------------------------------------------------
def test_constructor_checks():
    P = compute.PressureProfile
    for args, kw in ((("w", 8), {}), ((2, 8), {}), (("z", 0), {}), (("z", 8193), {}), (("z", 2.5), {}), (("z", True), {}),
                     (("z", 8), dict(lower=0.0)), (("z", 8), dict(upper=1.0)), (("z", 8), dict(lower=1.0, upper=1.0)),
                     (("z", 8), dict(lower=0.0, upper=float("inf"))), (("z", 8), dict(streaming="drop")),
                     (("z", 8), dict(max_term=0.0)), (("z", 8), dict(max_term=float("nan")))):
        with pytest.raises(_lib.AzpError):
            P(*args, **kw)
    p = P("x", 8192, lower=-1.0, upper=3.0, streaming="keep", max_term=64.0)
    assert (p.axis, p.num_bins, p.streaming, p.max_term, p.path) == ("x", 8192, "keep", 64.0, 0)
    np.testing.assert_array_equal(p.bin_edges, np.linspace(-1.0, 3.0, 8193))
    assert p.bin_centers[0] == 0.5 * (p.bin_edges[0] + p.bin_edges[1])
    p.path = 2
    with pytest.raises(_lib.AzpError):
        p.path = 3
    with pytest.raises(compute.DataAccessError):
        p.normal_pressure
    with pytest.raises(compute.DataAccessError):
        P("z", 8).bin_edges  # (the default range is the box's: no box yet)
    with pytest.raises(_lib.AzpError):
        compute.PressureProfileRecorder(compute.RadialDistributionFunction(compute.All(), compute.All(), 1.0, 8), 2)
    assert compute.PressureProfileRecorder(p, 2).table() == {}


def test_forces_that_are_refused_say_why():
    nl = nlist.Cell(buffer=0.4)
    cases = ((pair.DPDGeneralWeight(nl, kT=1.0, default_r_cut=1.0), "thermostat"),
             (pair.TwoPatchMorse(nl, default_r_cut=1.0), "anisotropic"),
             (angle.Harmonic(), "many-body"), (dihedral.Periodic(), "many-body"), (object(), "not a force"))
    for f, word in cases:
        with pytest.raises(_lib.AzpError, match=word):
            compute.PressureProfile("z", 8, forces=[f])
    # a one-body force is skipped silently, the accepted ones are accepted
    compute.PressureProfile("z", 8, forces=[external.PlanarHarmonicBarrier(1.0), pair.Hertz(nl, default_r_cut=1.0)])
