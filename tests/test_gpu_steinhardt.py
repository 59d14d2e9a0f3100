"""compute.Steinhardt, compute.SolidLiquid and their recorders on the GPU against the numpy reference
(tests/steinhardt_ref.py) on the fixtures of tests/steinhardt_fixtures.py, whose own conditions tests/test_steinhardt.py
checks on the CPU. The bounds, in units u = 2^-40:

    S_lm     N_b(i) u against the exact sum: 0.5 u of quantisation per bond and an evaluation error below 0.5 u
             (measured on the host build of the same header: 0.004 u)
    T_lm     2 (N_b(i) + 1) u: each of the N_b + 1 added q_lm(k) carries the error of S(k) / N_b(k) <= 1 u, 0.5 u of its own
             quantisation, and 2^-52-relative rounding of the division
    q_l      6 u absolute: the 2-norm is 1-Lipschitz, sqrt(4 pi / (2l + 1) * 2 sum_m) of per-component errors <= 1 u
             stays below sqrt(8 pi) u = 5.02 u
    qbar_l   12 u absolute, the same with components within 2 u
    every count, flag and histogram: exact."""

import functools

import numpy as np
import pytest

import steinhardt_fixtures as fx
import steinhardt_ref as ref

import azplugins_amd as azp
from azplugins_amd import _lib, compute
from azplugins_amd import synthetic as syn

pytestmark = pytest.mark.gpu

ALL_PAIRS, CELLS = _lib.STEINHARDT_PATH_ALL_PAIRS, _lib.STEINHARDT_PATH_CELLS
U = 2.0 ** -40


def _filter(names):
    return azp.All() if names is None else azp.Type(list(names))


def _sim(f):
    L, tilt, periodic = f["box"]
    box = azp.Box(L[0], L[1], L[2], tilt[0], tilt[1], tilt[2], periodic=periodic)
    snap = azp.Snapshot.from_arrays(f["xyz"], box, typeid=f["types"], types=f["type_names"])
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(snap)
    return sim


def _steinhardt(sim, f, group, l, path, average=False):
    c = compute.Steinhardt(_filter(group), l, f["r_max"], average=average, num_bins=fx.NUM_BINS)
    c.path = path
    sim.operations.add(c)
    return c


def _solid_liquid(sim, f, group, l, path, q_threshold, solid_threshold):
    c = compute.SolidLiquid(_filter(group), l, f["r_max"], q_threshold, solid_threshold)
    c.path = path
    sim.operations.add(c)
    return c


@functools.lru_cache(maxsize=None)
def _fixture(name):
    if name in fx.LATTICES:
        return fx.lattice(name)
    if name in fx.RANDOM:
        return fx.random(*fx.RANDOM[name])
    return getattr(fx, name)()


@functools.lru_cache(maxsize=None)
def _reference(name, group, l, q_threshold=None):
    """Computed once per (fixture, group, l) and shared; nobody writes to it."""
    f = _fixture(name)
    return ref.reference(f["xyz"], f["types"], f["box"], fx.mask(group), l, f["r_max"], q_threshold=q_threshold)


def _read_all(c):
    """One read per quantity of a Steinhardt: (num_neighbors, S words, order, T words or None, summary row)."""
    return (c.num_neighbors.astype(np.int64), c._read("qlm"), c.particle_order, c._read("qlm_average") if c.average else None,
            c._read("summary"))


def _check_against_reference(got, out, l, average, tag):
    """Prints every figure, then asserts the bounds of the module docstring."""
    nb, S, order, T, row = got
    assert np.array_equal(nb, out["num_neighbors"]), tag
    assert not np.isnan(order).any(), tag
    err_s = np.abs(S.astype(ref.LD) - out["S"]).astype(np.float64).max(axis=1)
    print("%s: max |S - exact| = %.3f u (worst row N_b = %d)" % (tag, err_s.max(), nb[err_s.argmax()]))
    assert np.all(err_s <= np.maximum(nb, 0)), tag
    want = out["qbar"] if average else out["q"]
    err_q = np.abs(order - want).max()
    print("%s: max |%s - reference| = %.3f u" % (tag, "qbar_l" if average else "q_l", err_q / U))
    assert err_q <= (12 if average else 6) * U, tag
    if average:
        err_t = np.abs(T.astype(ref.LD) - out["T"]).astype(np.float64).max(axis=1)
        print("%s: max |T - exact| = %.3f u" % (tag, err_t.max()))
        assert np.all(err_t <= 2 * (nb + 1)), tag
    want_row = ref.summary(out, l, fx.NUM_BINS, average=average)
    nt = len(l)
    assert np.array_equal(row[:4], want_row[:4]) and np.array_equal(row[4 + nt:], want_row[4 + nt:]), tag
    # (the sums of q_l are the device's own llrint(q_l 2^40): exact against its own particle_order, and within the
    # per-particle bound + 1 u of rounding of the reference's)
    g = out["in_group"]
    assert np.array_equal(row[4:4 + nt], np.rint(order[g].astype(ref.LD) * ref.FIXED).astype(np.int64).sum(axis=0)), tag
    assert np.all(np.abs(row[4:4 + nt] - want_row[4:4 + nt]) <= ((12 if average else 6) + 1) * g.sum()), tag
    assert np.all(order[~g] == 0.0) and not S[~g].any(), tag


# ---------------------------------------------------------------------------
# lattices: dyadic positions, exact displacements
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(fx.LATTICES))
def test_lattices(name):
    _, _, neighbours, expect = fx.LATTICES[name]
    f = _fixture(name)
    sim = _sim(f)
    out = _reference(name, None, (4, 6))
    words = {}
    for path in (ALL_PAIRS, CELLS):
        for average in (False, True):
            c = _steinhardt(sim, f, None, (4, 6), path, average)
            got = _read_all(c)
            assert np.all(got[0] == neighbours)
            _check_against_reference(got, out, (4, 6), average, "%s path %d average %d" % (name, path, average))
            assert np.abs(got[2] - np.array(expect)).max() < 1e-6
            words[(path, average)] = (got[1], got[3])
            if average:  # every particle has the same q_lm: qbar_l == q_l within the bound
                assert np.abs(got[2] - out["q"]).max() <= 12 * U
            assert np.abs(c.order - np.array(expect)).max() < 1e-6 and c.histogram.sum() == 2 * f["xyz"].shape[0]
    assert np.array_equal(words[(ALL_PAIRS, False)][0], words[(CELLS, False)][0])
    assert np.array_equal(words[(ALL_PAIRS, True)][0], words[(CELLS, True)][0])
    assert np.array_equal(words[(ALL_PAIRS, True)][1], words[(CELLS, True)][1])


def test_fcc_is_all_solid():
    f = _fixture("fcc")
    sim = _sim(f)
    for path in (ALL_PAIRS, CELLS):
        c = _solid_liquid(sim, f, None, 6, path, 0.7, 12)
        assert np.all(c.num_connections == 12) and c.solid.all() and c.num_solid == 256 and np.all(c.num_neighbors == 12)
        h = c.connection_histogram
        assert h[12] == 256 and h.sum() == 256
    strict = _solid_liquid(sim, f, None, 6, 0, 0.7, 13)
    assert not strict.solid.any() and strict.num_solid == 0


# ---------------------------------------------------------------------------
# random fixtures
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("l", [(4, 6), (1, 12)], ids=["l4_6", "l1_12"])
@pytest.mark.parametrize("group", [None, fx.AB], ids=["all", "AB"])
@pytest.mark.parametrize("name", sorted(fx.RANDOM))
def test_random_fixtures(name, group, l):
    f = _fixture(name)
    sim = _sim(f)
    tilted = name.startswith("tilted")
    out = _reference(name, group, l)
    got = {}
    for path in (ALL_PAIRS,) if tilted else (ALL_PAIRS, CELLS):
        for average in (False, True):
            c = _steinhardt(sim, f, group, l, path, average)
            got[(path, average)] = _read_all(c)
            _check_against_reference(got[(path, average)], out, l, average, "%s %r %r path %d average %d" % (name, group, l, path, average))
    if tilted:
        with pytest.raises(_lib.AzpError):
            _steinhardt(sim, f, group, l, CELLS).order  # the cells path does not take a tilted box
        auto = _steinhardt(sim, f, group, l, 0)
        assert np.array_equal(auto._read("qlm"), got[(ALL_PAIRS, False)][1])
        return
    for average in (False, True):
        a, b = got[(ALL_PAIRS, average)], got[(CELLS, average)]
        nb = a[0]
        assert np.all(np.abs(a[1] - b[1]).max(axis=1) <= nb)
        same = np.array_equal(a[1], b[1]) and (not average or np.array_equal(a[3], b[3]))
        print("%s %r %r average %d: the two paths give %s words" % (name, group, l, average, "identical" if same else "DIFFERENT"))
        assert np.array_equal(a[4][:4], b[4][:4])


# ---------------------------------------------------------------------------
# further cases
# ---------------------------------------------------------------------------
def test_sparse_rows_without_neighbours_are_zero():
    f = _fixture("sparse")
    sim = _sim(f)
    out = _reference("sparse", None, (4, 6))
    alone = out["num_neighbors"] == 0
    assert alone.any() and not alone.all()
    for path in (ALL_PAIRS, CELLS):
        for average in (False, True):
            got = _read_all(_steinhardt(sim, f, None, (4, 6), path, average))
            _check_against_reference(got, out, (4, 6), average, "sparse path %d average %d" % (path, average))
            assert np.all(got[2][alone] == 0.0) and not got[1][alone].any() and not np.isnan(got[2]).any()
        assert ref.threshold_gap(_reference("sparse", None, (6,), 0.5), 0.5) >= 1e-6
        c = _solid_liquid(sim, f, None, 6, path, 0.5, 1)
        nc = c.num_connections
        assert np.all(nc[alone] == 0) and not c.solid[alone].any()
        assert np.array_equal(nc, _reference("sparse", None, (6,), 0.5)["num_connections"])


def test_blob_more_rows_and_candidates_than_a_tile():
    f = _fixture("blob")
    sim = _sim(f)
    for l in ((4, 6), (1, 12)):
        out = _reference("blob", None, l)
        words = []
        for path in (ALL_PAIRS, CELLS):
            for average in (False, True):
                got = _read_all(_steinhardt(sim, f, None, l, path, average))
                assert np.all(got[0] == 299)
                _check_against_reference(got, out, l, average, "blob %r path %d average %d" % (l, path, average))
            words.append(got[1])
        assert np.array_equal(words[0], words[1])


def test_two_phases_connections_and_solid_flags_are_exact():
    f, p = _fixture("two_phase"), fx.TWO_PHASE
    sim = _sim(f)
    out = _reference("two_phase", None, (p["l"],), p["q_threshold"])
    assert ref.threshold_gap(out, p["q_threshold"]) >= 1e-6
    want_solid = out["num_connections"] >= p["solid_threshold"]
    n = f["xyz"].shape[0]
    for path in (ALL_PAIRS, CELLS):
        c = _solid_liquid(sim, f, None, p["l"], path, p["q_threshold"], p["solid_threshold"])
        assert np.array_equal(c.num_connections.astype(np.int64), out["num_connections"]), path
        assert np.array_equal(c.solid, want_solid)
        assert 0 < c.num_solid < n and c.num_solid == want_solid.sum()
        assert np.array_equal(c.num_neighbors.astype(np.int64), out["num_neighbors"])
        want_row = ref.summary(out, (p["l"],), 1, solid_threshold=p["solid_threshold"])
        row = c._read("summary")
        assert np.array_equal(row[:4], want_row[:4]) and np.array_equal(row[5:], want_row[5:])
        assert np.array_equal(c.connection_histogram, np.bincount(np.minimum(out["num_connections"], 32), minlength=33))


def test_reproducible_across_reads_and_the_particle_sorter():
    f = _fixture("cube515")
    sim = _sim(f)
    st = sim.state
    computes = {path: _steinhardt(sim, f, fx.AB, (4, 6), path, True) for path in (ALL_PAIRS, CELLS)}
    solid = {path: _solid_liquid(sim, f, fx.AB, 6, path, 0.3, 3) for path in (ALL_PAIRS, CELLS)}

    def by_tag(path):
        tag = st.tag[: st.N].cpu().numpy().astype(np.int64)
        order = np.argsort(tag)
        c = computes[path]
        return [x[order] for x in (c._read("qlm"), c._read("qlm_average"), c.num_neighbors, solid[path].num_connections)]

    before = {path: by_tag(path) for path in computes}
    again = {path: by_tag(path) for path in computes}
    for path in computes:
        assert all(np.array_equal(a, b) for a, b in zip(before[path], again[path]))  # two reads: bit-identical
    tag0 = st.tag[: st.N].cpu().numpy().copy()
    azp.ParticleSorter(particles_per_block=16).sort(sim)
    assert not np.array_equal(st.tag[: st.N].cpu().numpy(), tag0)  # (the rows moved)
    for path in computes:
        after = by_tag(path)
        assert all(np.array_equal(a, b) for a, b in zip(before[path], after)), path


# ---------------------------------------------------------------------------
# the recorders
# ---------------------------------------------------------------------------
def _liquid(recorders):
    cfg = syn.config_north_star(4)  # 256 particles
    n = cfg["xyz"].shape[0]
    assert n == 256
    tag = np.arange(n, dtype=np.uint64)
    v = np.stack([syn.normal(77, tag, c) for c in range(3)], axis=1)
    snap = azp.Snapshot.from_arrays(cfg["xyz"], cfg["L"], types=("A",), velocity=v - v.mean(axis=0))
    sim = azp.Simulation(device="cuda:0", seed=5)
    sim.create_state_from_snapshot(snap)
    plj = azp.pair.PerturbedLennardJones(nlist=azp.nlist.Cell(buffer=0.3), default_r_cut=2.5, mode="shift")
    plj.params[("A", "A")] = cfg["params"]
    sim.operations.integrator = azp.Integrator(dt=0.004, forces=[plj], methods=[azp.ConstantVolume()])
    st = compute.Steinhardt(azp.All(), (4, 6), 1.5, average=True, num_bins=50)
    sl = compute.SolidLiquid(azp.All(), 6, 1.5, 0.6, 6)
    sim.operations.add(st)
    sim.operations.add(sl)
    recs = None
    if recorders:
        recs = (compute.SteinhardtRecorder(st, 10), compute.SolidLiquidRecorder(sl, 10))
        for r in recs:
            sim.operations.add(r)
    return sim, st, sl, recs


def _bits(t):
    import torch

    return t.clone().view(torch.int64).cpu().numpy()


def test_recorders_leave_the_run_unchanged_and_record_the_computes_own_rows():
    sim, st, sl, (rec_st, rec_sl) = _liquid(True)
    sim.run(20)
    assert list(rec_st.timesteps) == [10, 20] and list(rec_sl.timesteps) == [10, 20]
    order, hist, num_solid, conn = rec_st.order, rec_st.histogram, rec_sl.num_solid, rec_sl.connection_histogram
    assert order.shape == (2, 2) and hist.shape == (2, 2, 50) and num_solid.shape == (2,) and conn.shape == (2, 33)
    assert np.all(rec_st.num_particles == 256) and np.all(hist.sum(axis=2) == 256) and np.all(conn.sum(axis=1) == 256)
    plain = None
    for k, stop in enumerate((10, 20)):
        plain, st2, sl2, _ = _liquid(False)
        plain.run(stop)
        assert np.array_equal(st2.order, order[k]) and np.array_equal(st2.histogram, hist[k]), stop
        assert sl2.num_solid == num_solid[k] and np.array_equal(sl2.connection_histogram, conn[k]), stop
    assert np.array_equal(_bits(sim.state.pos), _bits(plain.state.pos))
    assert np.array_equal(_bits(sim.state.vel), _bits(plain.state.vel))
    assert not np.array_equal(order[0], order[1])  # (the liquid moved)
    rec_st.reset()
    rec_sl.reset()
    assert rec_st.timesteps.shape == (0,) and rec_st.order.shape == (0, 2) and rec_sl.num_solid.shape == (0,)
