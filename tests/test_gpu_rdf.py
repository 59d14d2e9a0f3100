"""compute.RadialDistributionFunction and compute.RDFRecorder on the GPU: the integer pair counts equal the numpy
all-pairs reference (tests/rdf_ref.py) exactly on fixtures without edge pairs (tests/rdf_fixtures.py), the two paths
agree wherever both are valid, and a recorder leaves the run bit-identical."""

import ctypes as C

import numpy as np
import pytest

import rdf_fixtures as fx
import rdf_ref

import azplugins_amd as azp
from azplugins_amd import _lib, compute
from azplugins_amd import synthetic as syn

pytestmark = pytest.mark.gpu

ALL_PAIRS, CELLS = _lib.RDF_PATH_ALL_PAIRS, _lib.RDF_PATH_CELLS


def _filter(names):
    return azp.All() if names is None else azp.Type(list(names))


def _box(f):
    L, tilt, periodic = f["box"]
    return azp.Box(L[0], L[1], L[2], tilt[0], tilt[1], tilt[2], periodic=periodic)


def _sim(f):
    snap = azp.Snapshot.from_arrays(f["xyz"], _box(f), typeid=f["types"], types=f["type_names"])
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(snap)
    return sim


def _compute(sim, f, group, path=0, num_bins=None):
    rdf = compute.RadialDistributionFunction(_filter(group[0]), _filter(group[1]), f["r_max"], num_bins or f["num_bins"])
    rdf.path = path
    sim.operations.computes.append(rdf)
    return rdf


def _reference(f, group, num_bins=None):
    ga, gb = group
    assert rdf_ref.edge_pairs(f["xyz"], f["types"], f["box"], fx.mask(ga), fx.mask(gb), f["r_max"], num_bins or f["num_bins"]) == 0
    return rdf_ref.counts(f["xyz"], f["types"], f["box"], fx.mask(ga), fx.mask(gb), f["r_max"], num_bins or f["num_bins"])


def _row(rdf):
    return rdf._read("row")


def _check(f, paths):
    """Every group of the fixture on every path: the whole row (counts and group sizes) equals the reference."""
    sim = _sim(f)
    for group in f["groups"]:
        ref = _reference(f, group)
        for path in paths:
            rdf = _compute(sim, f, group, path)
            row = _row(rdf)
            assert np.array_equal(row, ref), (group, path, np.nonzero(row != ref)[0][:8], int(row[:-4].sum()), int(ref[:-4].sum()))
            assert rdf.group_sizes == tuple(ref[-4:-1]) and rdf.num_pairs == ref[-4] * ref[-3] - ref[-2]
            assert np.array_equal(rdf.rdf, compute.rdf_from_counts(ref[:-4], ref[-4], ref[-3], ref[-2], np.prod(f["box"][0]), f["r_max"]))


# ---------------------------------------------------------------------------
# edge rules on dyadic positions (exact in any order, FMA or not: no edge-pair condition needed)
# ---------------------------------------------------------------------------
def test_dyadic_lattice_edges_and_single_bin_waves():
    f = fx.dyadic_lattice()
    sim = _sim(f)
    for group in f["groups"]:
        ref = rdf_ref.counts(f["xyz"], f["types"], f["box"], fx.mask(group[0]), fx.mask(group[1]), f["r_max"], f["num_bins"])
        for path in (0, ALL_PAIRS):
            assert np.array_equal(_row(_compute(sim, f, group, path)), ref), (group, path)
    c = _compute(sim, f, fx.ALL_ALL, ALL_PAIRS).counts
    assert c.dtype == np.int64 and c.shape == (32,)
    assert c[8] == 6 * 512 and c[:8].sum() == 0       # r = 1 on the lower edge of bin 8, every hit of a wave in one bin
    assert c[16] == 6 * 512                            # r = 2 on the lower edge of bin 16
    assert c[11] == 12 * 512 and c[13] == 8 * 512      # sqrt(2), sqrt(3)
    # r = 4 = r_max (6 per particle, at exactly half the box) is excluded: what is counted are the lattice vectors
    # with 0 < n^2 < 16, of which there are 250
    assert c.sum() == 250 * 512


@pytest.mark.parametrize("pick,bin_", [((0, 1), 16), ((0, 2), 20), ((0, 3), None), ((0, 4), 31)])
def test_dyadic_points_land_in_their_bins(pick, bin_):
    f = fx.dyadic_points()
    f = dict(f, xyz=f["xyz"][list(pick)], types=f["types"][list(pick)])
    c = _compute(_sim(f), f, fx.ALL_ALL).counts
    expect = np.zeros(32, dtype=np.int64)
    if bin_ is not None:
        expect[bin_] = 2  # both orders
    assert np.array_equal(c, expect)


def test_dyadic_points_together():
    f = fx.dyadic_points()
    ref = rdf_ref.counts(f["xyz"], f["types"], f["box"], None, None, f["r_max"], f["num_bins"])
    assert np.array_equal(_row(_compute(_sim(f), f, fx.ALL_ALL)), ref)


# ---------------------------------------------------------------------------
# all-pairs: tile and mask edges
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", fx.TILE_SIZES)
def test_all_pairs_tile_and_mask_edges(n):
    _check(fx.tile(n), (ALL_PAIRS, 0))


# ---------------------------------------------------------------------------
# bins
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("num_bins", fx.BIN_COUNTS)
def test_bin_counts(num_bins):
    assert fx.BIN_COUNTS[-1] == _lib.RDF_MAX_BINS
    _check(fx.bins(num_bins), (ALL_PAIRS, CELLS))


def test_one_bin_past_the_largest_is_refused():
    f = fx.bins(64)
    sim = _sim(f)
    rdf = _compute(sim, f, fx.ALL_ALL)
    with pytest.raises(_lib.AzpError):
        rdf.num_bins = _lib.RDF_MAX_BINS + 1
    with pytest.raises(_lib.AzpError):
        compute.RadialDistributionFunction(azp.All(), azp.All(), 3.0, _lib.RDF_MAX_BINS + 1)
    # and by the library itself
    import torch

    st = sim.state
    out = torch.zeros(_lib.RDF_MAX_BINS + 5, dtype=torch.int64, device=st.device)
    a = _lib.RdfArgs()
    a.d_pos, a.N, a.n_total, a.box, a.ntypes = st.pos.data_ptr(), st.N, st.N, st.box.to_c(), 4
    a.num_bins, a.r_max, a.scale, a.path, a.d_out = _lib.RDF_MAX_BINS + 1, 3.0, (_lib.RDF_MAX_BINS + 1) / 3.0, ALL_PAIRS, out.data_ptr()
    assert _lib.lib().azp_rdf_counts(C.byref(a), _lib.raw_stream(st.device)) == -1
    a.num_bins, a.scale = _lib.RDF_MAX_BINS, _lib.RDF_MAX_BINS / 3.0
    assert _lib.lib().azp_rdf_counts(C.byref(a), _lib.raw_stream(st.device)) == 0
    torch.cuda.synchronize()
    assert int(out[: _lib.RDF_MAX_BINS].sum()) == int(_reference(f, fx.ALL_ALL, _lib.RDF_MAX_BINS)[:-4].sum())


# ---------------------------------------------------------------------------
# boxes
# ---------------------------------------------------------------------------
def test_triclinic_box_all_pairs():
    f = fx.triclinic()
    _check(f, (ALL_PAIRS, 0))
    rdf = _compute(_sim(f), f, fx.ALL_ALL, CELLS)
    with pytest.raises(_lib.AzpError):
        rdf.counts  # the cells path does not take a tilted box


def test_r_max_at_half_the_smallest_width():
    f = fx.dyadic_lattice()
    sim = _sim(f)
    rdf = _compute(sim, f, fx.ALL_ALL)
    assert rdf.r_max == 0.5 * f["box"][0][0]
    assert rdf.counts.sum() == 250 * 512
    rdf.r_max = np.nextafter(4.0, 5.0)
    with pytest.raises(_lib.AzpError, match="minimum image"):
        rdf.counts


# ---------------------------------------------------------------------------
# the cells path
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", fx.CELL_NAMES)
def test_cells_path_equals_all_pairs_and_reference(name):
    """3, 4 and 5 cells per axis, a non-cubic grid, a non-periodic axis, a cluster: both paths give the reference's
    row (hence each other's) exactly."""
    _check(fx.cells(name), (CELLS, ALL_PAIRS, 0))


def test_two_cells_on_an_axis():
    f = fx.two_cells()
    sim = _sim(f)
    ref = _reference(f, fx.ALL_ALL)
    with pytest.raises(_lib.AzpError):
        _row(_compute(sim, f, fx.ALL_ALL, CELLS))
    auto = _compute(sim, f, fx.ALL_ALL, 0)
    assert np.array_equal(_row(auto), ref) and np.array_equal(_row(_compute(sim, f, fx.ALL_ALL, ALL_PAIRS)), ref)
    # path 0 took all-pairs: it asked for no scratch
    a = _lib.RdfArgs()
    a.N = a.n_total = sim.state.N
    a.box, a.ntypes, a.num_bins, a.r_max, a.scale, a.path = sim.state.box.to_c(), 4, f["num_bins"], f["r_max"], f["num_bins"] / f["r_max"], 0
    need = C.c_uint64(1)
    assert _lib.lib().azp_rdf_scratch_size(C.byref(a), C.byref(need)) == 0 and need.value == 0


def _grid_rule(L, periodic, r_max, n_total):
    """walk_make_grid (csrc/pair_walk.hpp) restated: floor(L / r_max) cells per axis, at least 1 and at most 1024 (fewer
    than 3 on a periodic axis: no grid); while there are more cells than max(64, 2 n_total) (at most 2^21), every axis is
    scaled by min(cbrt(cap / cells), 0.95), rounded down, not below 3 (periodic) or 1."""
    dim = [np.floor(L[d] / r_max) for d in range(3)]
    if any(periodic[d] and dim[d] < 3 for d in range(3)):
        return None
    dim = [min(max(x, 1.0), 1024.0) for x in dim]
    cap = min(float(1 << 21), max(64.0, 2.0 * n_total))
    for _ in range(64):
        if np.prod(dim) <= cap:
            break
        f = min(np.cbrt(cap / np.prod(dim)), 0.95)
        dim = [max(3.0 if periodic[d] else 1.0, np.floor(dim[d] * f)) for d in range(3)]
    return tuple(int(x) for x in dim) if np.prod(dim) <= (1 << 21) else None


@pytest.mark.parametrize("dims,n", [((17, 17, 15), 2400), ((33, 33, 34), 19000)], ids=["scan1", "scan3x10"])
def test_cells_path_on_every_scan_path(dims, n):
    """The counting sort behind the cells path (cell_bin.hpp) on the scan paths the small fixtures do not reach:
    4,335 cells take more than one trip of the single workgroup, 37,026 cells the three-kernel scan with 10 blocks of
    4,096, the last one partial (the rule of binning_cases.paths_of). Orthorhombic periodic box of
    L_k = (dims_k + 0.5) r_max, uniform random fill, r_max = 1, 32 bins: _grid_rule gives exactly dims (n is large enough
    for the cap max(64, 2 n) to leave the grid alone). The whole row of the cells path equals the all-pairs row, which
    shares no binning code with it; about two ordered pairs per particle are counted."""
    import binning_cases as B

    r_max = 1.0
    L = tuple((d + 0.5) * r_max for d in dims)
    assert _grid_rule(L, fx.PBC, r_max, n) == dims
    assert B.paths_of(dims, n)[0] == ("scan1x2" if n == 2400 else "scan3x10") and int(np.prod(dims)) % B.SCAN_BLOCK != 0
    xyz, types = fx._uniform(n, L, 41)
    f = fx._fixture(xyz, types, L, r_max, 32, (fx.ALL_ALL, fx.AB_BC))
    sim = _sim(f)
    for group in f["groups"]:
        rows = {path: _row(_compute(sim, f, group, path)) for path in (CELLS, ALL_PAIRS)}
        assert rows[CELLS].shape == (f["num_bins"] + 4,)
        assert np.array_equal(rows[CELLS], rows[ALL_PAIRS]), (group, np.nonzero(rows[CELLS] != rows[ALL_PAIRS])[0][:8])
        assert int(rows[CELLS][:-4].sum()) > 0
        if group == fx.ALL_ALL:
            assert n < int(rows[CELLS][:-4].sum()) < 3 * n


# ---------------------------------------------------------------------------
# mid size
# ---------------------------------------------------------------------------
def test_mid_size_paths_agree_and_total_matches_the_neighbor_list():
    """32,768 particles, r_max = r_cut = 3: the cells row equals the all-pairs row, and the number of counted pairs
    equals the total of the row lengths of the product's neighbor list at r_list = r_max (azp_nlist_count, an
    independent kernel). The two could differ by pairs within rounding of the radius; the configuration (seed 2, the
    default) has none within 1e-11 r_max, which is checked here on the device with torch."""
    import torch

    import helpers

    cfg = syn.config_plj_sc(32)
    n = cfg["xyz"].shape[0]
    r_max = cfg["r_cut"]
    f = dict(xyz=cfg["xyz"], types=np.zeros(n, dtype=np.int64), type_names=("A",), box=(tuple(cfg["L"]), fx.ORTHO, fx.PBC),
             r_max=r_max, num_bins=300)
    sim = _sim(f)
    # pairs with | r - r_max | <= 1e-11 r_max: none
    x = sim.state.pos[:, :3]
    L = torch.tensor(cfg["L"], dtype=torch.float64, device=x.device)
    near = 0
    for c0 in range(0, n, 1024):
        d = x[c0:c0 + 1024, None, :] - x[None, :, :]
        d -= L * torch.round(d / L)
        r = d.pow(2).sum(dim=-1).sqrt()
        near += int(((r - r_max).abs() <= 1e-11 * r_max).sum())
    assert near == 0
    rows = {path: _row(_compute(sim, f, fx.ALL_ALL, path)) for path in (CELLS, ALL_PAIRS)}
    assert np.array_equal(rows[CELLS], rows[ALL_PAIRS])
    a, t = helpers.gpu_cells(syn.pos4(cfg["xyz"]), (cfg["L"], fx.ORTHO, fx.PBC), r_max)
    out = helpers.gpu_nlist_rows(a, t)
    assert out["rc_count"] == 0
    total = int(out["n_count"].sum())
    assert total > 80 * n and int(rows[CELLS][:300].sum()) == total
    assert tuple(rows[CELLS][300:]) == (n, n, n, 0)


# ---------------------------------------------------------------------------
# determinism and reuse
# ---------------------------------------------------------------------------
def test_two_reads_agree_and_buffers_follow_changes():
    import torch

    f, g = fx.cells("four"), fx.cells("noncubic")
    sim = _sim(f)
    rdf = _compute(sim, f, fx.AB_BC)
    first, second = _row(rdf), _row(rdf)
    assert np.array_equal(first, second) and np.array_equal(first, _reference(f, fx.AB_BC))
    rdf.num_bins = 77
    assert np.array_equal(_row(rdf), _reference(f, fx.AB_BC, 77))
    rdf.num_bins = f["num_bins"]
    sim.create_state_from_snapshot(azp.Snapshot.from_arrays(g["xyz"], _box(g), typeid=g["types"], types=g["type_names"]))
    assert np.array_equal(_row(rdf), _reference(g, fx.AB_BC))
    # a row of garbage is overwritten whole, on both paths
    for path in (CELLS, ALL_PAIRS):
        rdf.path = path
        out = torch.full((1, g["num_bins"] + 4), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=sim.state.device)
        rdf._launch(out.data_ptr())
        assert np.array_equal(out.cpu().numpy()[0], _reference(g, fx.AB_BC))


# ---------------------------------------------------------------------------
# the recorder
# ---------------------------------------------------------------------------
def _liquid(recorder_period=None, evaporator=False):
    cfg = syn.config_plj_sc(12)  # 1728 particles
    n = cfg["xyz"].shape[0]
    tag = np.arange(n, dtype=np.uint64)
    v = np.stack([syn.normal(77, tag, c) for c in range(3)], axis=1)
    names = ("A", "E") if evaporator else ("A",)
    snap = azp.Snapshot.from_arrays(cfg["xyz"], cfg["L"], types=names, velocity=v - v.mean(axis=0))
    sim = azp.Simulation(device="cuda:0", seed=5)
    sim.create_state_from_snapshot(snap)
    plj = azp.pair.PerturbedLennardJones(nlist=azp.nlist.Cell(buffer=cfg["r_buff"]), default_r_cut=cfg["r_cut"], mode="shift")
    for a_ in names:
        for b_ in names:
            plj.params[(a_, b_)] = cfg["params"]
    sim.operations.integrator = azp.Integrator(dt=0.004, forces=[plj], methods=[azp.ConstantVolume()])
    rdf = compute.RadialDistributionFunction(azp.Type(["A"]) if evaporator else azp.All(), azp.All(), cfg["r_cut"], 60)
    sim.operations.add(rdf)
    rec = None
    if recorder_period is not None:
        rec = compute.RDFRecorder(rdf, recorder_period)
        sim.operations.add(rec)
    if evaporator:
        from azplugins_amd.evaporate import ParticleEvaporator

        half = 0.5 * float(cfg["L"][2])
        sim.operations.add(ParticleEvaporator(trigger=10, solvent_type="A", evaporated_type="E", lo=-half, hi=half, Nmax=100))
    return sim, rdf, rec


def _bits(t):
    import torch

    return t.clone().view(torch.int64).cpu().numpy()


def test_recorder_rows_equal_the_compute_and_the_run_is_unchanged():
    sim, rdf, rec = _liquid(recorder_period=10)
    sim.run(30)
    assert list(rec.timesteps) == [10, 20, 30]
    counts, g = rec.counts, rec.rdf
    assert counts.shape == (3, 60) and counts.dtype == np.int64 and g.shape == (3, 60)
    plain = None
    for k, stop in enumerate((10, 20, 30)):
        # a second, identical run without a recorder that stops there
        plain, rdf2, _ = _liquid()
        plain.run(stop)
        assert np.array_equal(rdf2.counts, counts[k]), stop
        assert np.array_equal(rdf2.rdf, g[k])
    assert not np.array_equal(counts[0], counts[2])  # (the liquid moved)
    assert np.array_equal(_bits(sim.state.pos), _bits(plain.state.pos))
    assert np.array_equal(_bits(sim.state.vel), _bits(plain.state.vel))
    n = sim.state.N
    vol = float(np.prod(syn.config_plj_sc(12)["L"]))
    # the mean: the sum of the counts over the sum of the pair numbers, 3 (n^2 - n)
    assert np.array_equal(rec.mean_rdf, compute.rdf_from_counts(counts.sum(axis=0), 3 * (n * n - n), 1, 0, vol, 3.0))
    assert rec.num_pairs == [n * n - n] * 3
    rec.reset()
    assert rec.timesteps.shape == (0,) and rec.counts.shape == (0, 60)


def test_recorder_frames_follow_an_evaporator():
    """100 particles change from A to E at the timesteps 0, 10, 20 (ahead of the step): the frames at 10, 20, 30 see
    N_A = N - 100, N - 200, N - 300 and are normalised with their own pair numbers."""
    sim, rdf, rec = _liquid(recorder_period=10, evaporator=True)
    sim.run(30)
    n = sim.state.N
    table = rec._table("rows")
    assert [int(r[60]) for r in table] == [n - 100, n - 200, n - 300] and all(int(r[61]) == n for r in table)
    assert [int(r[62]) for r in table] == [n - 100, n - 200, n - 300]
    pairs = [(n - 100 * k) * n - (n - 100 * k) for k in (1, 2, 3)]
    assert rec.num_pairs == pairs
    vol = float(np.prod(syn.config_plj_sc(12)["L"]))
    for k in range(3):
        assert np.array_equal(rec.rdf[k], compute.rdf_from_counts(rec.counts[k], n - 100 * (k + 1), n, n - 100 * (k + 1), vol, 3.0))
    # (with the first frame's pair number the last frame would come out (n - 300) / (n - 100) = 0.88 times too small)
    stale = compute.rdf_from_counts(rec.counts[2], n - 100, n, n - 100, vol, 3.0)
    assert np.allclose(stale[-10:], rec.rdf[2][-10:] * (n - 300) / (n - 100), rtol=1e-12) and rec.rdf[2][-10:].min() > 0.0
    assert np.array_equal(rdf.group_sizes, (n - 300, n, n - 300))
