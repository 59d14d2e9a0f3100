"""compute.ThermodynamicField without a GPU: the restated tree against exact sums, the normalisation of raw rows
(``compute.thermo_field_quantities``), the bin volumes and the validation."""

import math
from types import SimpleNamespace

import numpy as np
import pytest

import thermo_field_ref as ref

import azplugins_amd as azp
from azplugins_amd import compute

SIZES = [1, 63, 64, 65, 4096, 4097]
SEEDS = {1: 11, 63: 12, 64: 13, 65: 14, 4096: 15, 4097: 16}
N_FORCES = 2


def _particles(n, seed, dyadic=False):
    rng = np.random.default_rng(seed)
    if dyadic:
        # small multiples of 2^-4: every product and every partial sum is exact in float64
        draw = lambda shape, lo, hi: rng.integers(lo, hi, size=shape).astype(np.float64) / 16.0
        vel = np.concatenate([draw((n, 3), -32, 33), draw((n, 1), 1, 33)], axis=1)
        forces = [np.concatenate([np.zeros((n, 3)), draw((n, 1), -64, 65)], axis=1) for _ in range(N_FORCES)]
        virials = [draw((6, n), -64, 65) for _ in range(N_FORCES)]
    else:
        vel = np.concatenate([rng.normal(size=(n, 3)) + np.array([3.0, -2.0, 0.5]), rng.uniform(0.5, 2.0, size=(n, 1))], axis=1)
        forces = [rng.normal(size=(n, 4)) * 10.0 ** f for f in range(N_FORCES)]
        virials = [rng.normal(size=(6, n)) * 10.0 ** f for f in range(N_FORCES)]
    return vel, forces, virials


def _exact(vel, forces, virials):
    """fsum of every slot over the rounded terms the kernels add (the virials and energies force by force), and the sum
    of their magnitudes."""
    t = ref.terms(vel)
    cols = [[t[:, k]] for k in range(11)]
    cols += [[v[c] for v in virials] for c in range(6)]
    cols += [[f[:, 3] for f in forces]]
    want = np.array([math.fsum(np.concatenate(c)) for c in cols])
    mag = np.array([math.fsum(np.abs(np.concatenate(c))) for c in cols])
    return want, mag


@pytest.mark.parametrize("n", SIZES)
def test_restated_tree_against_fsum(n):
    vel, forces, virials = _particles(n, SEEDS[n])
    got = ref.tree(ref.terms(vel, forces, virials))
    want, mag = _exact(vel, forces, virials)
    assert ref.levels(n) == (1 if n <= 64 else 2 if n <= 4096 else 3)
    err = np.abs(got - want)
    limit = ref.bound(mag, n, N_FORCES)
    print("n = %d: worst error / bound %.3g" % (n, (err / limit).max()))
    assert (err <= limit).all()


@pytest.mark.parametrize("n", SIZES)
def test_exact_on_dyadic_data(n):
    vel, forces, virials = _particles(n, 100 + SEEDS[n], dyadic=True)
    got = ref.tree(ref.terms(vel, forces, virials))
    want, _ = _exact(vel, forces, virials)
    assert got.tobytes() == want.tobytes()


def test_tree_depends_on_the_members_alone():
    rng = np.random.default_rng(5)
    x = rng.normal(size=200)
    assert ref.tree(x[:0]) == 0.0 and ref.tree(x[:1]) == x[0]
    # the first run of 64 is one butterfly whatever follows it
    assert ref.tree(np.r_[ref.tree(x[:64]), ref.tree(x[64:128]), ref.tree(x[128:192]), ref.tree(x[192:])]) == ref.tree(x)


def test_row_restatement_groups_by_bin_in_tag_order():
    rng = np.random.default_rng(6)
    n = 300
    vel = np.concatenate([rng.normal(size=(n, 3)), np.ones((n, 1))], axis=1)
    xyz = rng.uniform(-4.0, 4.0, size=(n, 3))
    tags = rng.permutation(n)
    types = rng.integers(0, 2, size=n)
    b = ref.bins(xyz, ref.CARTESIAN, (0, 0, 3), (0, 0, -4.0), (0, 0, 2.0))
    assert set(np.unique(b)) == {-1, 0, 1, 2}
    t = ref.terms(vel)
    row = ref.row(b, tags, None, t, types, 3, 3)
    for k in range(3):
        members = np.nonzero(b == k)[0]
        members = members[np.argsort(tags[members])]
        assert row[k, :18].tobytes() == ref.tree(t[members]).tobytes()
        assert row[k, 18:].tolist() == [np.sum(types[members] == ty) for ty in range(3)]
    perm = rng.permutation(n)
    assert ref.row(b[perm], tags[perm], None, t[perm], types[perm], 3, 3).tobytes() == row.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# normalisation
# ---------------------------------------------------------------------------------------------------------------------
def _rows():
    """Three bins of two types: an ordinary one, one particle, a massless pair; a fourth is empty."""
    rows = np.zeros((4, 20))
    vels = [np.array([[1.0, 2.0, -1.0, 2.0], [0.5, -1.0, 3.0, 1.0], [-2.0, 0.25, 0.5, 4.0]]), np.array([[1.5, -0.5, 2.0, 3.0]]),
            np.array([[1.0, 1.0, 1.0, 0.0], [2.0, 0.0, 1.0, 0.0]])]
    for k, v in enumerate(vels):
        rows[k, :18] = ref.terms(v).sum(axis=0)
        rows[k, 11:17] = np.arange(1.0, 7.0) * (k + 1)
        rows[k, 17] = -3.0 * (k + 1)
        rows[k, 18], rows[k, 19] = len(v) - 1, 1
    return rows, vels


def test_normalisation_subtract_and_keep():
    rows, vels = _rows()
    vol = np.array([2.0, 0.5, 1.0, 4.0])
    keep = compute.thermo_field_quantities(rows, vol, "keep")
    sub = compute.thermo_field_quantities(rows, vol, "subtract")
    assert keep["counts"].dtype == np.int64 and keep["counts"].tolist() == [[2, 1], [0, 1], [1, 1], [0, 0]]
    assert keep["num_particles"].tolist() == [3, 1, 2, 0]
    np.testing.assert_array_equal(keep["number_density"], keep["counts"] / vol[:, None])
    np.testing.assert_array_equal(keep["mass_density"], rows[:, 1] / vol)
    np.testing.assert_array_equal(keep["potential_energy_density"], rows[:, 17] / vol)
    np.testing.assert_array_equal(keep["sums"], rows)
    # a bin without mass has velocity 0; so has an empty one
    v0 = (vels[0][:, 3:4] * vels[0][:, :3]).sum(axis=0) / vels[0][:, 3].sum()
    np.testing.assert_allclose(keep["velocities"][0], v0, rtol=1e-15)
    assert not keep["velocities"][2].any() and not keep["velocities"][3].any()
    # keep: tr K / (3 n), 0 in the empty bin
    for k, v in enumerate(vels):
        trace = (v[:, 3] * (v[:, :3] ** 2).sum(axis=1)).sum()
        assert keep["kinetic_temperature"][k] == pytest.approx(trace / (3 * len(v)), rel=1e-15)
    assert keep["kinetic_temperature"][3] == 0.0
    np.testing.assert_allclose(keep["pressure_tensor"], (rows[:, 5:11] + rows[:, 11:17]) / vol[:, None], rtol=1e-15)
    # subtract: the peculiar velocities, 3 n - 3 degrees of freedom, 0 for n < 2
    v = vels[0]
    pec = v[:, :3] - v0
    kp = np.array([(v[:, 3] * pec[:, a] * pec[:, b]).sum() for a, b in compute._TENSOR_PAIRS])
    assert sub["kinetic_temperature"][0] == pytest.approx((kp[0] + kp[3] + kp[5]) / 6.0, rel=1e-13)
    np.testing.assert_allclose(sub["pressure_tensor"][0], (kp + rows[0, 11:17]) / vol[0], rtol=1e-13)
    assert sub["kinetic_temperature"][1] == 0.0 and sub["kinetic_temperature"][3] == 0.0
    # the massless bin keeps K (nothing to subtract) and has n = 2
    assert sub["kinetic_temperature"][2] == 0.0 and np.isfinite(sub["pressure_tensor"]).all()
    np.testing.assert_allclose(sub["pressure"], sub["pressure_tensor"][:, [0, 3, 5]].sum(axis=1) / 3.0, rtol=1e-15)
    # without volumes the quantities that divide by one are left out
    bare = compute.thermo_field_quantities(rows, None, "keep")
    assert "pressure" not in bare and "number_density" not in bare and "kinetic_temperature" in bare
    with pytest.raises(azp.AzpError, match="streaming"):
        compute.thermo_field_quantities(rows, vol, "remove")
    with pytest.raises(azp.AzpError, match="at least 18"):
        compute.thermo_field_quantities(rows[:, :10], vol, "keep")


def test_leading_axes_are_independent():
    rows, _ = _rows()
    vol = np.array([2.0, 0.5, 1.0, 4.0])
    stacked = np.stack([rows, 2.0 * rows])
    q = compute.thermo_field_quantities(stacked, np.stack([vol, 3.0 * vol]), "subtract")
    one = compute.thermo_field_quantities(2.0 * rows, 3.0 * vol, "subtract")
    for name in one:
        assert q[name][1].tobytes() == one[name].tobytes()


def test_cartesian_volumes_in_a_tilted_box():
    box = azp.Box(9.0, 10.0, 11.0, 0.3, -0.2, 0.4)
    f = compute.CartesianThermodynamicField((7, 0, 3), (-4.0, 0.0, -5.5), (3.0, 0.0, 2.75))
    v = f._bin_volumes(box)
    assert v.shape == (21,) and (v == v[0]).all()
    covered = (7.0 / 9.0) * (8.25 / 11.0)
    assert v.sum() == pytest.approx(covered * box.volume, rel=1e-14)
    assert box.volume == pytest.approx(9.0 * 10.0 * 11.0, rel=1e-15)
    f0 = compute.CartesianThermodynamicField((0, 0, 0), (0, 0, 0), (0, 0, 0))
    assert f0._bin_volumes(box).tolist() == [box.volume]


def test_cylindrical_volumes():
    box = azp.Box(9.0, 10.0, 11.0)
    f = compute.CylindricalThermodynamicField((5, 0, 0), (0.0, 0.0, 0.0), (4.0, 0.0, 0.0))
    v = f._bin_volumes(box)
    assert v.shape == (5,) and v.sum() == pytest.approx(math.pi * 16.0 * 11.0, rel=1e-14)
    g = compute.CylindricalThermodynamicField((5, 8, 4), (1.0, 0.0, -2.0), (4.0, 2.0 * math.pi, 2.0))
    w = g._bin_volumes(box)
    assert w.shape == (160,) and w.sum() == pytest.approx(math.pi * 15.0 * 4.0, rel=1e-14)
    assert w.reshape(5, 8, 4)[2].std() == pytest.approx(0.0, abs=1e-15) and w[0] < w[-1]
    h = compute.CylindricalThermodynamicField((0, 8, 0), (0.0, 0.0, 0.0), (0.0, 2.0 * math.pi, 0.0))
    assert h._bin_volumes(box) is None


# ---------------------------------------------------------------------------------------------------------------------
# validation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [compute.CartesianThermodynamicField, compute.CylindricalThermodynamicField])
def test_validation(cls):
    f = cls((4, 0, 2), (-1.0, 0.0, 0.0), (1.0, 0.0, 3.0))
    assert isinstance(f, compute.ThermodynamicField) and isinstance(f.filter, azp.All) and f.streaming == "subtract"
    assert f.num_bins == (4, 0, 2) and f.coordinates.shape == (4, 2, 2)
    v = compute.CartesianVelocityFieldCompute((4, 0, 2), (-1.0, 0.0, 0.0), (1.0, 0.0, 3.0))
    np.testing.assert_array_equal(f.coordinates, v.coordinates)
    with pytest.raises(azp.AzpError, match="upper_bounds"):
        cls((4, 0, 2), (-1.0, 0.0, 0.0), (-1.0, 0.0, 3.0))
    with pytest.raises(azp.AzpError, match="negative"):
        cls((4, -1, 2), (-1.0, 0.0, 0.0), (1.0, 0.0, 3.0))
    with pytest.raises(azp.AzpError, match="3 entries"):
        cls((4, 2), (-1.0, 0.0, 0.0), (1.0, 0.0, 3.0))
    with pytest.raises(azp.AzpError, match="2\\^31"):
        cls((2**11, 2**11, 2**11), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    with pytest.raises(azp.AzpError, match="filter"):
        cls((4, 0, 2), (-1.0, 0.0, 0.0), (1.0, 0.0, 3.0), filter="A")
    with pytest.raises(azp.AzpError, match="streaming"):
        cls((4, 0, 2), (-1.0, 0.0, 0.0), (1.0, 0.0, 3.0), streaming="remove")
    with pytest.raises(azp.AzpError, match="streaming"):
        f.streaming = "drop"
    f.streaming = "keep"
    f.upper_bounds = (1.0, 0.0, -3.0)
    with pytest.raises(azp.AzpError, match="upper_bounds"):
        f._check_bounds()
    t = cls((4, 0, 2), (-1.0, 0.0, 0.0), (1.0, 0.0, 3.0), filter=azp.Type(["B"]))
    assert isinstance(t.filter, azp.Type)
    for name in compute.THERMO_FIELD_PROPERTIES:
        with pytest.raises(compute.DataAccessError):
            getattr(t, name)
    with pytest.raises(azp.AzpError, match="ThermodynamicField"):
        compute.ThermodynamicFieldRecorder(v, 5)
    with pytest.raises(NotImplementedError):
        compute.ThermodynamicField((1, 0, 0), (0, 0, 0), (1, 0, 0))._bin_volumes(None)


def test_forces_limit_is_checked_before_a_run():
    sim = azp.Simulation(device="cpu", seed=1)
    sim.operations.integrator = azp.Integrator(dt=0.001, forces=[azp.bond.DoubleWell() for _ in range(9)])
    sim.operations.add(compute.CartesianThermodynamicField((0, 0, 4), (0, 0, -1.0), (0, 0, 1.0)))
    with pytest.raises(azp.AzpError, match="ThermodynamicField sums at most 8 forces"):
        sim._check_writers()


def test_recorder_refuses_a_table_beyond_2_30_bytes():
    rec_cls = compute.ThermodynamicFieldRecorder
    # the base class grows the table by doubling, to at least 64 rows
    assert rec_cls._grown_bytes(0, 0, 100) == 64 * 100 * 8
    assert rec_cls._grown_bytes(5, 64, 100) == 64 * 100 * 8
    assert rec_cls._grown_bytes(64, 64, 100) == 128 * 100 * 8
    types = ["A", "B", "C"]
    width_per_bin = 18 + len(types)

    def recorder(bins):
        f = compute.CartesianThermodynamicField((bins, 0, 0), (0.0, 0, 0), (1.0, 0, 0))
        f._sim = SimpleNamespace(state=SimpleNamespace(types=types, device="cpu"))
        return rec_cls(f, 5)

    # 64 rows x bins x 21 words x 8 bytes against 2^30
    fits = 2**30 // (64 * width_per_bin * 8)
    assert 64 * fits * width_per_bin * 8 <= 2**30 < 64 * (fits + 1) * width_per_bin * 8
    rec = recorder(fits + 1)
    with pytest.raises(azp.AzpError, match=str(64 * (fits + 1) * width_per_bin * 8)):
        rec._record(rec.field._sim, 5)
    assert rec.timesteps.size == 0 and rec.table == {} and rec.mean() == {}
