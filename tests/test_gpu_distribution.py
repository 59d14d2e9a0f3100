"""compute.BondedDistribution on the GPU: counts, outside and num_groups EQUAL to the NumPy reference
(tests/distribution_ref.py) for bonds, angles, dihedrals and special pairs, the exact edges of the bins, the
global-atomics path against the LDS path, the normalisation, the sorter and the in-run recorder.

A device coordinate can differ from NumPy's in its last bits (FMA contraction in the squared length, atan2), so every
exact comparison first asserts a guard on the reference alone: the index (x - lo) * scale of every group lies at least
1e-9 from an integer, seven orders above that rounding. No group is left out of a comparison."""

import numpy as np
import pytest

import azplugins_amd as azp
import bonded_table_ref as TR
import distribution_ref as R
from azplugins_amd import _lib, compute

pytestmark = pytest.mark.gpu

KINDS = ("bond", "angle", "dihedral", "pair")
BOND_PARAMS = dict(r_0=1.0, r_1=1.5, U_1=1.0, U_tilt=0.5)
GUARD = 1e-9


def _snapshot(s, velocity=None, extra_types=False):
    kw = {}
    for kind in KINDS:
        kw[kind + "s"], kw[kind + "_typeid"] = s[kind + "s"], s[kind + "_typeid"]
        kw[kind + "_types"] = ["T0", "T1"] + (["unused"] if extra_types else [])
    L, tilt = s["L"], s["tilt"]
    return azp.Snapshot.from_arrays(s["xyz"], azp.Box(L[0], L[1], L[2], *tilt), velocity=velocity, **kw)


def _sim(s, num_bins=64, kinds=KINDS, **snap_kw):
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(_snapshot(s, **snap_kw))
    sim.operations.tuners.clear()
    dists = {kind: compute.BondedDistribution(kind, num_bins, **R.ranges(kind)) for kind in kinds}
    for d in dists.values():
        sim.operations.add(d)
    return sim, dists


def _assert_equals_reference(d, ref, what):
    assert R.guard(ref["index"]) > GUARD, what
    counts, outside, total = d.counts, d.outside, d.num_groups
    assert counts.dtype == np.int64 and counts.shape == ref["counts"].shape, what
    print("%s: %d groups, %d outside, %d bins in use" % (what, total.sum(), outside.sum(), (counts > 0).sum()))
    assert np.array_equal(counts, ref["counts"]), what
    assert np.array_equal(outside, ref["outside"]) and np.array_equal(total, ref["num_groups"]), what
    assert np.array_equal(counts.sum(axis=1) + outside, total)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("box", ["triclinic", "cubic"])
def test_counts_equal_the_reference_for_all_four_kinds(box):
    """40 chains of 8 and a trimer (323 particles: two workgroups, the second partly filled), two group types per kind,
    64 bins, in a tilted and in an orthorhombic periodic box with groups across every face."""
    s = R.chain_system(box=box)
    sim, dists = _sim(s)
    for kind in KINDS:
        d = dists[kind]
        assert d.types == ["T0", "T1"]
        _assert_equals_reference(d, R.chain_reference(kind, 64, box=box), "%s, %s box" % (kind, box))
        assert _lib.last_launch()["lds_bytes"] == 2 * 66 * 4 and _lib.last_launch()["grid"] == 2
        again = d.counts
        assert np.array_equal(again, d.counts)                   # two reads, the same integers
    assert dists["bond"].outside.sum() > 0 and not dists["angle"].outside.any() and not dists["dihedral"].outside.any()


def test_exact_edges_of_the_bins():
    """Axis-aligned bonds of lengths 1.0, 1.25, 1.5 and 2.0 with [r_min, r_max) = [1, 2) and 4 bins: bins 0, 1, 2 (lower
    edges inclusive) and `outside` (r_max exclusive); a bond of 0.75 is outside as well. All lengths are exact in
    binary and have exact squares, so no guard is needed. A collinear angle and a planar trans dihedral (sin phi = +0)
    land in the last bin; the right angle and the planar cis dihedral sit in the middle of the fifth of 9 bins."""
    xyz = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.25, 0.0], [0.0, 0.0, 1.5], [-2.0, 0.0, 0.0], [0.0, -0.75, 0.0],
                    [5.0, 0.0, 0.0], [4.0, 0.0, 0.0], [4.0, 0.0, 1.0], [3.0, 0.0, 1.0], [5.0, 0.0, 1.0]])
    bonds = [(0, 1), (0, 2), (3, 0), (0, 4), (5, 0)]
    angles = [(1, 0, 4), (1, 0, 2)]                               # collinear on the x axis; a right angle
    dihedrals = [(6, 7, 8, 9), (6, 7, 8, 10)]                     # trans: phi = pi exactly; cis: phi = 0
    snap = azp.Snapshot.from_arrays(xyz, (20.0, 20.0, 20.0), bonds=bonds, angles=angles, dihedrals=dihedrals)
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(snap)
    b = compute.BondedDistribution("bond", 4, r_min=1.0, r_max=2.0)
    a = compute.BondedDistribution("angle", 9)
    d = compute.BondedDistribution("dihedral", 9)
    for c in (a, b, d):
        sim.operations.add(c)
    assert b.counts.tolist() == [[1, 1, 1, 0]] and b.outside.tolist() == [2] and b.num_groups.tolist() == [5]
    assert a.counts.tolist() == [[0, 0, 0, 0, 1, 0, 0, 0, 1]] and a.num_groups.tolist() == [2]
    assert d.counts.tolist() == [[0, 0, 0, 0, 1, 0, 0, 0, 1]] and d.outside.tolist() == [0]
    for c, ref in ((b, R.histogram("bond", xyz, bonds, [0] * 5, 1, 4, (20.0,) * 3, r_min=1.0, r_max=2.0)),
                   (a, R.histogram("angle", xyz, angles, [0] * 2, 1, 9, (20.0,) * 3)),
                   (d, R.histogram("dihedral", xyz, dihedrals, [0] * 2, 1, 9, (20.0,) * 3))):
        assert np.array_equal(c.counts, ref["counts"]) and np.array_equal(c.outside, ref["outside"])


@pytest.mark.parametrize("kind", KINDS)
def test_global_atomics_path_equals_the_lds_path(kind):
    """2 types x (8192 + 2) words are 16388, four more than fit into 64 KiB: the automatic path counts with global
    integer atomics. Its counts equal the reference, and re-binned by 128 they equal the 64-bin counts of the LDS path
    on the same state (the scale differs by a power of two, so each fine bin lies in one coarse bin exactly). Forced
    paths: 2 at 64 bins gives the LDS path's integers, 1 where the histogram does not fit is refused."""
    s = R.chain_system()
    sim, dists = _sim(s, kinds=(kind,))
    coarse = dists[kind]
    fine = compute.BondedDistribution(kind, 8192, **R.ranges(kind))
    sim.operations.add(fine)
    assert 2 * (8192 + 2) > _lib.BONDED_HISTOGRAM_LDS_WORDS >= 8192 + 2
    ref = R.chain_reference(kind, 8192)
    _assert_equals_reference(fine, ref, kind + ", 8192 bins")
    assert _lib.last_launch()["lds_bytes"] == 0
    lds_counts, lds_outside = coarse.counts, coarse.outside
    assert _lib.last_launch()["lds_bytes"] == 2 * 66 * 4
    assert np.array_equal(fine.counts.reshape(2, 64, 128).sum(axis=2), lds_counts) and np.array_equal(fine.outside, lds_outside)
    coarse.path = _lib.BONDED_HISTOGRAM_PATH_GLOBAL
    assert np.array_equal(coarse.counts, lds_counts) and _lib.last_launch()["lds_bytes"] == 0
    fine.path = _lib.BONDED_HISTOGRAM_PATH_LDS
    with pytest.raises(azp.AzpError):
        fine.counts


def test_distribution_integrates_to_one_and_is_zero_without_groups():
    s = R.chain_system()
    sim, dists = _sim(s, extra_types=True)
    for kind in KINDS:
        d = dists[kind]
        assert d.types == ["T0", "T1", "unused"]
        p, counts, total, outside = d.distribution, d.counts, d.num_groups, d.outside
        assert p.shape == (3, 64) and total[2] == 0 and not p[2].any() and not counts[2].any()
        inside = (total[:2] - outside[:2]) / total[:2]
        assert np.abs(p[:2].sum(axis=1) * d.bin_width - inside).max() < 1e-14
        if kind in ("angle", "dihedral"):
            assert np.array_equal(inside, [1.0, 1.0])
        assert np.array_equal(p, compute.distribution_from_counts(counts, total, d.bin_width))


def test_counts_are_identical_after_the_sorter():
    s = R.chain_system()
    sim, dists = _sim(s)
    before = {kind: (d.counts, d.outside, d.num_groups) for kind, d in dists.items()}
    order = azp.ParticleSorter(particles_per_block=16).sort(sim).cpu().numpy()
    assert (order != np.arange(order.size)).sum() > 250      # the sort did move the particles
    for kind, d in dists.items():
        for got, want in zip((d.counts, d.outside, d.num_groups), before[kind]):
            assert np.array_equal(got, want), kind
        assert np.array_equal(d.counts, R.chain_reference(kind, 64)["counts"])


# ---------------------------------------------------------------------------------------------------------------------
# in a run
# ---------------------------------------------------------------------------------------------------------------------
def _moving(recorder_period=None, method=None, angle_force=None):
    """The cubic chain system with velocities, DoubleWell bonds and an angle force under ``method``; angle and bond
    distributions, optionally with recorders."""
    s = R.chain_system(box="cubic")
    vel = np.random.default_rng(5).normal(size=s["xyz"].shape) * 0.5
    sim, dists = _sim(s, kinds=("angle", "bond"), velocity=vel - vel.mean(axis=0))
    dw = azp.bond.DoubleWell()
    dw.params["T0"], dw.params["T1"] = BOND_PARAMS, BOND_PARAMS
    if angle_force is None:
        angle_force = azp.angle.Harmonic()
        angle_force.params["T0"], angle_force.params["T1"] = dict(k=10.0, t0=2.0), dict(k=25.0, t0=2.8)
    sim.operations.integrator = azp.Integrator(dt=0.002, forces=[dw, angle_force], methods=[method or azp.ConstantVolume()])
    recs = {}
    if recorder_period:
        for kind, d in dists.items():
            recs[kind] = compute.BondedDistributionRecorder(d, recorder_period)
            sim.operations.add(recs[kind])
    return sim, dists, recs, angle_force


def _bits(t):
    return t.cpu().numpy().view(np.int64)


def test_recorder_rows_equal_the_compute_and_the_run_is_unchanged():
    sim, dists, recs, _ = _moving(recorder_period=5)
    sim.run(20)
    twin, twin_dists, _, _ = _moving()
    for k in range(4):
        twin.run(5)
        for kind in ("angle", "bond"):
            rec = recs[kind]
            assert np.array_equal(rec.counts[k], twin_dists[kind].counts), (kind, k)
            assert np.array_equal(rec.num_groups[k], twin_dists[kind].num_groups)
    for kind in ("angle", "bond"):
        rec = recs[kind]
        assert list(rec.timesteps) == [5, 10, 15, 20]
        assert rec.counts.shape == (4, 2, 64) and rec.counts.dtype == np.int64 and rec.num_groups.shape == (4, 2)
        assert not np.array_equal(rec.counts[0], rec.counts[3])           # the chains moved
        assert np.array_equal(rec.mean_distribution, compute.distribution_from_counts(
            rec.counts.sum(axis=0), rec.num_groups.sum(axis=0), dists[kind].bin_width))
    assert np.array_equal(recs["angle"].num_groups, [[121, 120]] * 4)
    # the trajectory with the recorders is the one without them, bit for bit
    assert np.array_equal(_bits(sim.state.pos), _bits(twin.state.pos))
    assert np.array_equal(_bits(sim.state.vel), _bits(twin.state.vel))
    recs["angle"].reset()
    assert recs["angle"].timesteps.shape == (0,) and recs["angle"].counts.shape == (0, 2, 64)
    assert not recs["angle"].mean_distribution.any()


def test_langevin_run_with_tabulated_angles_keeps_every_angle():
    """Chains under methods.Langevin with angle.Table forces (the harmonic potentials, tabulated on 256 intervals), 200
    steps: the forces stay finite and every recorded row holds every angle."""
    params = (dict(k=10.0, t0=2.0), dict(k=25.0, t0=2.8))
    table = azp.angle.Table()
    for name, p in zip(("T0", "T1"), params):
        table.params[name] = TR.sample("angle", 257, lambda t, p=p: 0.5 * p["k"] * (t - p["t0"]) ** 2, lambda t, p=p: -p["k"] * (t - p["t0"]))
    sim, dists, recs, f = _moving(recorder_period=50, method=azp.Langevin(azp.All(), kT=1.0), angle_force=table)
    sim.run(200)
    assert f is table and np.all(np.isfinite(f.forces)) and np.abs(f.forces).max() > 1.0
    assert np.all(np.isfinite(sim.state.pos.cpu().numpy()))
    rec = recs["angle"]
    assert list(rec.timesteps) == [50, 100, 150, 200]
    n_angles = len(R.chain_system(box="cubic")["angles"])
    assert n_angles == 241
    assert np.array_equal(rec.num_groups.sum(axis=1), [n_angles] * 4)
    assert np.array_equal(rec.counts.sum(axis=(1, 2)), [n_angles] * 4)
    assert abs(rec.mean_distribution[0].sum() * dists["angle"].bin_width - 1.0) < 1e-14
