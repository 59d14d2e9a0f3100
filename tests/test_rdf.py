"""compute.RadialDistributionFunction / compute.RDFRecorder without a GPU: the numpy reference on a lattice, the
normalisation, every refusal, the recorder's bookkeeping, the ABI struct and the edge-pair check of every random
fixture the GPU tests compare exactly (tests/rdf_fixtures.py)."""

import ctypes as C
import os
import subprocess
import tempfile
import types

import numpy as np
import pytest

import rdf_fixtures as fx
import rdf_ref

import azplugins_amd as azp
from azplugins_amd import _lib, compute

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------
def test_reference_simple_cubic_shells():
    a, n = 1.5, 6
    g = (np.arange(n) + 0.5) * a - 0.5 * n * a
    xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    N = n ** 3
    box = ((n * a,) * 3, fx.ORTHO, fx.PBC)
    num_bins, r_max = 90, 0.5 * n * a  # bins of 0.05
    row = rdf_ref.counts(xyz, np.zeros(N, dtype=int), box, None, None, r_max, num_bins)
    c = row[:num_bins]
    for r, neighbours in ((a, 6), (a * np.sqrt(2.0), 12), (a * np.sqrt(3.0), 8)):
        k = int(r * num_bins / r_max)
        assert c[k] == neighbours * N
    first = int(a * np.sqrt(3.0) * num_bins / r_max)
    assert c[: first + 1].sum() == 26 * N  # nothing else up to the third shell
    assert tuple(row[num_bins:]) == (N, N, N, 0)


@pytest.mark.parametrize("name", sorted(fx.random_fixtures()))
def test_random_fixtures_have_no_edge_pairs(name):
    """The GPU tests demand the reference's integers exactly, which is fair only if no pair of the fixture sits
    within rounding of a bin edge or of r_max. The cap is zero."""
    f = fx.random_fixtures()[name]
    for ga, gb in f["groups"]:
        assert rdf_ref.edge_pairs(f["xyz"], f["types"], f["box"], fx.mask(ga), fx.mask(gb), f["r_max"], f["num_bins"]) == 0


def test_edge_pairs_sees_an_edge():
    xyz = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 1.3, 0.0]])
    box = ((8.0,) * 3, fx.ORTHO, fx.PBC)
    assert rdf_ref.edge_pairs(xyz, [0, 0, 0], box, None, None, 4.0, 32) == 2   # r = 2 is a bin edge, both orders
    assert rdf_ref.edge_pairs(xyz[[0, 2]], [0, 0], box, None, None, 4.0, 32) == 0
    assert rdf_ref.edge_pairs(xyz[:2], [0, 0], box, None, None, 2.0, 7) == 2    # r = r_max


def test_reference_min_image_is_the_nearest_image_in_a_tilted_box():
    """The sequential minimum image of the device equals the nearest of the 27 images for every pair closer than
    r_max (half the smallest perpendicular width covers it)."""
    f = fx.triclinic()
    (Lx, Ly, Lz), (xy, xz, yz), _ = f["box"]
    cell = np.array([[Lx, 0.0, 0.0], [xy * Ly, Ly, 0.0], [xz * Lz, yz * Lz, Lz]])
    shifts = np.array([[i, j, k] for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)], dtype=float) @ cell
    d = f["xyz"][:, None, :] - f["xyz"][None, :, :]
    rsq = ((d[:, :, None, :] + shifts[None, None, :, :]) ** 2).sum(axis=-1).min(axis=-1)
    np.fill_diagonal(rsq, np.inf)
    r = np.sqrt(rsq[rsq < f["r_max"] ** 2])
    brute = np.bincount(np.minimum((r * (f["num_bins"] / f["r_max"])).astype(int), f["num_bins"] - 1), minlength=f["num_bins"])
    row = rdf_ref.counts(f["xyz"], f["types"], f["box"], None, None, f["r_max"], f["num_bins"])
    assert np.array_equal(brute, row[: f["num_bins"]])


def test_reference_counts_ghost_rows_as_partners_only():
    f = fx.tile(255)
    full = rdf_ref.counts(f["xyz"], f["types"], f["box"], None, None, f["r_max"], f["num_bins"])
    part = [rdf_ref.counts(np.roll(f["xyz"], -s, axis=0), np.roll(f["types"], -s), f["box"], None, None, f["r_max"], f["num_bins"],
                           n_own=n) for s, n in ((0, 100), (100, 155))]
    assert np.array_equal(full[:-4], part[0][:-4] + part[1][:-4])
    assert part[0][-4] == 100 and part[1][-3] == 155


# ---------------------------------------------------------------------------
# normalisation
# ---------------------------------------------------------------------------
def test_rdf_from_counts_ideal_gas_is_one():
    num_bins, r_max, n, volume = 40, 3.0, 1000, 20.0 ** 3
    edges = np.linspace(0.0, r_max, num_bins + 1)
    shell = 4.0 * np.pi / 3.0 * (edges[1:] ** 3 - edges[:-1] ** 3)
    n_pairs = n * n - n
    ideal = n_pairs * shell / volume  # (expected ordered pairs per bin of an uncorrelated system; not integers)
    g = compute.rdf_from_counts(ideal, n, n, n, volume, r_max)
    assert np.allclose(g, 1.0, rtol=1e-14, atol=0.0)
    # two disjoint groups: n_ab = 0
    g = compute.rdf_from_counts(300 * 700 * shell / volume, 300, 700, 0, volume, r_max)
    assert np.allclose(g, 1.0, rtol=1e-14, atol=0.0)


def test_rdf_from_counts_without_pairs_is_zero():
    assert np.array_equal(compute.rdf_from_counts([0, 0, 0], 0, 5, 0, 10.0, 1.0), np.zeros(3))
    assert np.array_equal(compute.rdf_from_counts([0, 0], 1, 1, 1, 10.0, 1.0), np.zeros(2))  # one particle, A = B


def test_rdf_from_counts_overlapping_groups():
    # A = {a, b}, B = {b, c}: N_A N_B - N_AB = 3 ordered pairs (a, b), (a, c), (b, c)
    counts = np.array([0, 3])
    g = compute.rdf_from_counts(counts, 2, 2, 1, 8.0, 2.0)
    shell = 4.0 * np.pi / 3.0 * (8.0 - 1.0)
    assert g[0] == 0.0 and g[1] == pytest.approx(3.0 * 8.0 / (3.0 * shell), rel=1e-15)
    assert g.dtype == np.float64


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
def _rdf(**kw):
    args = dict(filter_a=azp.All(), filter_b=azp.All(), r_max=3.0, num_bins=100)
    args.update(kw)
    return compute.RadialDistributionFunction(**args)


@pytest.mark.parametrize("kw", [dict(r_max=0.0), dict(r_max=-1.0), dict(r_max=float("nan")), dict(num_bins=0), dict(num_bins=-3),
                                dict(num_bins=_lib.RDF_MAX_BINS + 1), dict(num_bins=2.5), dict(filter_a=None),
                                dict(filter_b="A"), dict(filter_b=object())])
def test_constructor_refuses(kw):
    with pytest.raises(_lib.AzpError):
        _rdf(**kw)


def test_setters_refuse_and_accept():
    r = _rdf(num_bins=_lib.RDF_MAX_BINS, filter_a=azp.Type(["A", "B"]), filter_b=azp.Type("B"))
    assert r.num_bins == _lib.RDF_MAX_BINS >= 4096 and r.filter_a == azp.Type(["B", "A"]) and r.filter_b == azp.Type(["B"])
    for name, value in (("r_max", 0.0), ("num_bins", 0), ("num_bins", _lib.RDF_MAX_BINS + 1), ("path", 3)):
        with pytest.raises(_lib.AzpError):
            setattr(r, name, value)
    r.num_bins, r.r_max, r.path = 7, 3.5, _lib.RDF_PATH_CELLS
    assert np.array_equal(r.bin_edges, np.linspace(0.0, 3.5, 8)) and np.allclose(r.bin_centers, (np.arange(7) + 0.5) * 0.5)


def _fake_sim(box, domain=None, forces=()):
    return types.SimpleNamespace(state=types.SimpleNamespace(box=box), domain=domain,
                                 operations=types.SimpleNamespace(integrator=types.SimpleNamespace(forces=list(forces))))


def test_r_max_beyond_half_a_periodic_width_is_refused():
    r = _rdf(r_max=4.0)
    r._check_box(_fake_sim(azp.Box(8.0, 9.0, 10.0)))  # exactly half the smallest width: accepted
    r.r_max = np.nextafter(4.0, 5.0)
    with pytest.raises(_lib.AzpError, match="minimum image"):
        r._check_box(_fake_sim(azp.Box(8.0, 9.0, 10.0)))
    r._check_box(_fake_sim(azp.Box(8.0, 9.0, 10.0, periodic=(False, True, True))))  # the short axis is not periodic
    # a tilt narrows the perpendicular width: Lx / sqrt(1 + xy^2) = 8 / sqrt(1.25) = 7.155
    r.r_max = 3.6
    r._check_box(_fake_sim(azp.Box(8.0, 9.0, 10.0)))
    with pytest.raises(_lib.AzpError, match="minimum image"):
        r._check_box(_fake_sim(azp.Box(8.0, 9.0, 10.0, xy=0.5)))
    assert compute.perpendicular_widths(azp.Box(8.0, 9.0, 10.0, xy=0.5))[0] == pytest.approx(8.0 / np.sqrt(1.25))


def test_r_max_beyond_the_ghost_coverage_is_refused():
    dom = types.SimpleNamespace(decomp=types.SimpleNamespace(r_ghost=3.4))
    pot = types.SimpleNamespace(nlist=types.SimpleNamespace(buffer=0.4))
    box = azp.Box(20.0)
    _rdf(r_max=3.0)._check_box(_fake_sim(box, dom, [pot]))
    with pytest.raises(_lib.AzpError, match=r"3\.4.*0\.4"):
        _rdf(r_max=3.1)._check_box(_fake_sim(box, dom, [pot]))
    _rdf(r_max=3.4)._check_box(_fake_sim(box, dom, []))  # no neighbor list: the whole shell counts


def _c_args(L=(8.0, 8.0, 8.0), tilt=fx.ORTHO, periodic=fx.PBC, r_max=4.0, num_bins=32, path=0, n=100):
    a = _lib.RdfArgs()
    a.N = a.n_total = n
    a.box = _lib.make_box(L, tilt, periodic)
    a.ntypes = 1
    a.num_bins = num_bins
    a.r_max = r_max
    a.scale = num_bins / r_max if r_max > 0 else 1.0
    a.path = path
    return a


def test_c_abi_refuses_before_anything_is_launched():
    """azp_rdf_scratch_size runs the checks of azp_rdf_counts and touches no device."""
    lib = _lib.lib()
    need = C.c_uint64(12345)

    def rc(**kw):
        return lib.azp_rdf_scratch_size(C.byref(_c_args(**kw)), C.byref(need))

    assert rc() == 0 and need.value == 0  # two cells per axis: all-pairs, no scratch
    assert rc(L=(12.0, 12.0, 12.0)) == 0 and need.value > 100 * 36  # three cells: the binned copy lives in the scratch
    assert rc(L=(12.0, 12.0, 12.0), path=1) == 0 and need.value == 0
    bad = -1  # AZP_ERROR_INVALID_ARGUMENT
    assert rc(r_max=0.0) == bad and rc(r_max=-2.0) == bad
    assert rc(num_bins=0) == bad and rc(num_bins=_lib.RDF_MAX_BINS + 1) == bad and rc(num_bins=_lib.RDF_MAX_BINS) == 0
    assert rc(r_max=float(np.nextafter(4.0, 5.0))) == bad
    assert rc(r_max=float(np.nextafter(4.0, 5.0)), periodic=(0, 0, 0)) == 0
    assert rc(path=2) == bad                                     # two cells: a forced cells path is refused
    assert rc(L=(12.0, 12.0, 12.0), path=2) == 0
    assert rc(L=(12.0, 12.0, 12.0), tilt=(0.1, 0.0, 0.0), path=2) == bad  # tilt
    assert rc(L=(12.0, 12.0, 12.0), tilt=(0.1, 0.0, 0.0), path=0) == 0 and need.value == 0
    assert rc(L=(12.0, 12.0, 5.0), periodic=(1, 1, 0), path=2) == 0       # a short non-periodic axis has clamped cells
    assert rc(path=3) == bad
    a = _c_args()
    a.N = 101
    assert lib.azp_rdf_scratch_size(C.byref(a), C.byref(need)) == bad
    # azp_rdf_counts itself refuses the same way, before it reads a pointer
    assert lib.azp_rdf_counts(C.byref(_c_args(r_max=0.0)), None) == bad
    assert lib.azp_rdf_counts(C.byref(_c_args(path=2)), None) == bad
    assert lib.azp_rdf_counts(C.byref(_c_args()), None) == bad  # NULL d_out


def test_abi_struct_size_matches_header():
    src = '#include <stdio.h>\n#include "azp.h"\nint main(){printf("%zu %d\\n", sizeof(azp_rdf_args), AZP_RDF_MAX_BINS);return 0;}'
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "s.c"), "w") as f:
            f.write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        size, max_bins = (int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split())
    assert size == C.sizeof(_lib.RdfArgs)
    assert max_bins == _lib.RDF_MAX_BINS >= 4096


# ---------------------------------------------------------------------------
# attachment and the recorder
# ---------------------------------------------------------------------------
def test_unattached_reads_raise_data_access_error():
    r = _rdf()
    for name in ("counts", "rdf", "num_pairs", "group_sizes"):
        with pytest.raises(compute.DataAccessError):
            getattr(r, name)
    sim = azp.Simulation(device="cuda:0")
    sim.operations.computes.append(r)  # in the list, but the simulation has no state
    with pytest.raises(compute.DataAccessError):
        r.counts
    assert r.bin_edges.shape == (101,) and r.bin_centers.shape == (100,)  # (these need no state)


def test_recorder_timesteps_in_run():
    rec = compute.RDFRecorder(_rdf(), 10)
    assert rec.trigger == azp.Periodic(10)
    assert rec.timesteps_in_run(0, 30) == [10, 20, 30]
    assert rec.timesteps_in_run(10, 9) == [] and rec.timesteps_in_run(10, 10) == [20]
    assert compute.RDFRecorder(_rdf(), azp.Periodic(10, phase=3)).timesteps_in_run(0, 25) == [3, 13, 23]
    assert rec.timesteps.shape == (0,) and rec.counts.shape == (0, 100) and rec.rdf.shape == (0, 100)
    assert np.array_equal(rec.mean_rdf, np.zeros(100)) and rec.num_pairs == []
    rec.reset()
    with pytest.raises(_lib.AzpError):
        compute.RDFRecorder(compute.ThermodynamicQuantities(azp.All()), 10)
    with pytest.raises(_lib.AzpError):
        compute.ThermodynamicRecorder(_rdf(), 10)


def test_operations_add_and_remove_both_recorder_kinds():
    sim = azp.Simulation(device="cuda:0")
    thermo, rdf = compute.ThermodynamicQuantities(azp.All()), _rdf()
    recs = [compute.ThermodynamicRecorder(thermo, 5), compute.RDFRecorder(rdf, 5)]
    for op in (thermo, rdf) + tuple(recs):
        sim.operations.add(op)
        sim.operations.add(op)  # (adding twice keeps one)
    assert [c for c in sim.operations.computes] == [thermo, rdf]
    assert sim.operations.writers == recs
    assert recs[0]._compute is thermo and recs[1]._compute is rdf
    sim._check_writers()
    sim.operations.remove(rdf)
    with pytest.raises(_lib.AzpError, match="RDFRecorder: its RadialDistributionFunction is not in sim.operations.computes"):
        sim._check_writers()
    sim.operations.remove(recs[1])
    sim._check_writers()
    sim.operations.remove(thermo)
    with pytest.raises(_lib.AzpError, match="ThermodynamicRecorder: its ThermodynamicQuantities is not in"):
        sim._check_writers()
    sim.operations.remove(recs[0])
    assert sim.operations.writers == []
    with pytest.raises(ValueError):
        sim.operations.remove(recs[1])
