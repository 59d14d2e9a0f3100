"""compute.Cluster and its recorder on the GPU against the all-pairs reference (tests/cluster_ref.py) on the fixtures of
tests/cluster_fixtures.py, whose own condition tests/test_cluster.py checks on the CPU: no pair within 1e-9 of r_max^2.
Everything is exact (``np.array_equal``): keys, sizes, the whole summary row and ``cluster_idx``. There is no tolerance
anywhere."""

import functools

import numpy as np
import pytest

import cluster_fixtures as fx
import cluster_ref as ref
import steinhardt_fixtures as sf

import azplugins_amd as azp
from azplugins_amd import _lib, compute
from azplugins_amd import synthetic as syn

pytestmark = pytest.mark.gpu

ALL_PAIRS, CELLS = _lib.CLUSTER_PATH_ALL_PAIRS, _lib.CLUSTER_PATH_CELLS
NONE = _lib.CLUSTER_NONE


def _filter(names):
    return azp.All() if names is None else azp.Type(list(names))


def _sim(f):
    L, tilt, periodic = f["box"]
    box = azp.Box(L[0], L[1], L[2], tilt[0], tilt[1], tilt[2], periodic=periodic)
    snap = azp.Snapshot.from_arrays(f["xyz"], box, typeid=f["types"], types=f["type_names"], tag=f.get("tags"))
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(snap)
    return sim


def _cluster(sim, f, group, path, **kw):
    c = compute.Cluster(_filter(group), f["r_max"], size_bins=fx.SIZE_BINS, **kw)
    c.path = path
    sim.operations.add(c)
    return c


@functools.lru_cache(maxsize=None)
def _fixture(name):
    return fx.FIXTURES[name]()


@functools.lru_cache(maxsize=None)
def _reference(name, group):
    """Computed once per (fixture, group) and shared; nobody writes to it."""
    f = _fixture(name)
    return ref.reference(f["xyz"], f["types"], f["box"], sf.mask(group), f["r_max"], tags=fx.tags_of(f), size_bins=fx.SIZE_BINS)


def _check(c, out, tag):
    """Every output of one compute against a reference, exactly."""
    keys, sizes, row, idx = c.cluster_keys, c.cluster_sizes, c._read("summary"), c.cluster_idx
    assert keys.dtype == np.uint32 and sizes.dtype == np.uint32 and row.dtype == np.int64 and idx.dtype == np.int64, tag
    assert np.array_equal(row, out["row"]), "%s: row %r, expected %r" % (tag, row[:8], out["row"][:8])
    assert np.array_equal(keys, out["keys"]), tag
    assert np.array_equal(sizes, out["sizes"]), tag
    assert np.array_equal(idx, out["idx"]), tag
    s = compute.cluster_summary(out["row"], fx.SIZE_BINS)
    assert (c.num_particles, c.num_clusters, c.largest_cluster_size, c.largest_cluster_key, c.num_edges) == (
        s["num_particles"], s["num_clusters"], s["largest_cluster_size"], s["largest_cluster_key"], s["num_edges"]), tag
    assert np.array_equal(c.size_histogram, s["size_histogram"]), tag
    if s["num_particles"]:
        assert c.mean_cluster_size == s["num_particles"] / s["num_clusters"], tag
        assert c.weight_average_cluster_size == s["sum_size_squared"] / s["num_particles"], tag
    else:
        assert c.mean_cluster_size == 0.0 and c.weight_average_cluster_size == 0.0, tag
    return keys, sizes, row


# ---------------------------------------------------------------------------
# every fixture x every group x both paths
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("group", fx.GROUPS, ids=["all", "AB"])
@pytest.mark.parametrize("name", sorted(fx.FIXTURES))
def test_fixtures(name, group):
    f = _fixture(name)
    sim = _sim(f)
    out = _reference(name, group)
    got = {}
    for path in (ALL_PAIRS,) if fx.tilted(f) else (ALL_PAIRS, CELLS):
        got[path] = _check(_cluster(sim, f, group, path), out, "%s %r path %d" % (name, group, path))
    if fx.tilted(f):
        with pytest.raises(_lib.AzpError):
            _cluster(sim, f, group, CELLS).num_clusters  # the cells path does not take a tilted box
        auto = _cluster(sim, f, group, 0)
        assert np.array_equal(auto.cluster_keys, got[ALL_PAIRS][0])
    else:
        assert all(np.array_equal(a, b) for a, b in zip(got[ALL_PAIRS], got[CELLS]))


def test_ring_closes_through_the_boundary_in_every_tag_order():
    for tags in fx.RING_TAGS:
        f = _fixture("ring_" + tags)
        sim = _sim(f)
        for path in (ALL_PAIRS, CELLS):
            c = _cluster(sim, f, None, path)
            assert np.all(c.cluster_keys == 0) and np.all(c.cluster_sizes == 600), (tags, path)
            assert tuple(c._read("summary")[:6]) == (600, 1, 600, 0, 360000, 600), (tags, path)
    f = _fixture("ring_minus_one")
    c = _cluster(_sim(f), f, None, 0)
    assert tuple(c._read("summary")[:6]) == (599, 1, 599, int(fx.tags_of(f).min()), 599 ** 2, 598)
    f = _fixture("ring_minus_two")
    c = _cluster(_sim(f), f, None, 0)
    assert c.num_clusters == 2 and c.num_edges == 596 and sorted(np.unique(c.cluster_sizes)) == [249, 349]


def test_blob_bridge_and_size_ties():
    f = _fixture("blob")
    sim = _sim(f)
    for path in (ALL_PAIRS, CELLS):
        assert tuple(_cluster(sim, f, None, path)._read("summary")[:6]) == (300, 1, 300, 0, 90000, 44850)
    f = _fixture("bridge")
    sim = _sim(f)
    assert _cluster(sim, f, None, 0).num_clusters == 1
    two = _cluster(sim, f, fx.AB, 0)
    keys, sizes = two.cluster_keys, two.cluster_sizes
    assert two.num_clusters == 2 and keys[0] == NONE and sizes[0] == 0 and two.cluster_idx[0] == -1
    assert np.all(keys[1:6] == 1) and np.all(sizes[1:6] == 5) and np.all(keys[6:] == 6) and np.all(sizes[6:] == 4)
    f = _fixture("sc_singletons")
    sim = _sim(f)
    for path in (ALL_PAIRS, CELLS):
        row = _cluster(sim, f, None, path)._read("summary")
        assert tuple(row[:7]) == (64, 64, 1, 0, 64, 0, 64)  # among 64 clusters of one, the smallest tag


def test_empty_group_and_one_particle():
    f = _fixture("sc")
    sim = _sim(f)
    want = np.zeros(6 + fx.SIZE_BINS, dtype=np.int64)
    want[3] = -1
    for path in (ALL_PAIRS, CELLS):
        c = _cluster(sim, f, ("C",), path)
        assert np.array_equal(c._read("summary"), want), path
        assert np.all(c.cluster_keys == NONE) and not c.cluster_sizes.any() and np.all(c.cluster_idx == -1)
        assert c.largest_cluster_key == -1 and c.mean_cluster_size == 0.0 and c.weight_average_cluster_size == 0.0
    f = _fixture("single")
    sim = _sim(f)
    for path in (ALL_PAIRS, CELLS):
        c = _cluster(sim, f, None, path)
        assert tuple(c._read("summary")[:7]) == (1, 1, 1, 0, 1, 0, 1)
        assert list(c.cluster_keys) == [0] and list(c.cluster_sizes) == [1] and list(c.cluster_idx) == [0]
        assert _cluster(sim, f, ("A",), path).largest_cluster_key == -1  # the particle is of type B


# ---------------------------------------------------------------------------
# solid=
# ---------------------------------------------------------------------------
def test_clusters_of_the_solid_particles():
    f, p = fx.two_phase(), sf.TWO_PHASE
    sim = _sim(f)
    sl = compute.SolidLiquid(azp.All(), p["l"], f["r_max"], p["q_threshold"], p["solid_threshold"])
    sim.operations.add(sl)
    solid = sl.solid  # (pinned exactly by tests/test_gpu_steinhardt.py)
    assert 0 < solid.sum() < solid.shape[0]
    out = ref.reference(f["xyz"], f["types"], f["box"], None, f["r_max"], member=solid, size_bins=fx.SIZE_BINS)
    for path in (ALL_PAIRS, CELLS):
        c = _cluster(sim, f, None, path, solid=sl)
        _check(c, out, "two_phase solid path %d" % path)
        assert c.num_particles == solid.sum() == sl.num_solid
        print("two_phase path %d: %d solid particles in %d clusters, the largest of %d" % (
            path, c.num_particles, c.num_clusters, c.largest_cluster_size))
    # a cut-off of the cluster's own: fewer edges, the same group
    g = dict(f, r_max=fx.TWO_PHASE_R_MAX)
    out = ref.reference(g["xyz"], g["types"], g["box"], None, g["r_max"], member=solid, size_bins=fx.SIZE_BINS)
    assert out["num_clusters"] > 1
    for path in (ALL_PAIRS, CELLS):
        _check(_cluster(sim, g, None, path, solid=sl), out, "two_phase solid r_max %g path %d" % (g["r_max"], path))
    # a SolidLiquid of another simulation, or of none, is refused
    other = _sim(f)
    foreign = compute.SolidLiquid(azp.All(), p["l"], f["r_max"], p["q_threshold"], p["solid_threshold"])
    other.operations.add(foreign)
    with pytest.raises(_lib.AzpError, match="same simulation"):
        _cluster(sim, f, None, 0, solid=foreign).num_clusters
    loose = compute.SolidLiquid(azp.All(), p["l"], f["r_max"], p["q_threshold"], p["solid_threshold"])
    with pytest.raises(_lib.AzpError, match="same simulation"):
        _cluster(sim, f, None, 0, solid=loose).num_clusters


# ---------------------------------------------------------------------------
# reproducibility
# ---------------------------------------------------------------------------
def test_reproducible_across_reads_paths_and_the_particle_sorter():
    f = _fixture("cube515_hi")
    sim = _sim(f)
    st = sim.state
    computes = {path: _cluster(sim, f, fx.AB, path) for path in (ALL_PAIRS, CELLS)}

    def by_tag(path):
        tag = st.tag[: st.N].cpu().numpy().astype(np.int64)
        order = np.argsort(tag)
        c = computes[path]
        return [c.cluster_keys[order], c.cluster_sizes[order], c._read("summary")]

    before = {path: by_tag(path) for path in computes}
    again = {path: by_tag(path) for path in computes}
    for path in computes:
        assert all(np.array_equal(a, b) for a, b in zip(before[path], again[path]))  # two reads: identical
    assert all(np.array_equal(a, b) for a, b in zip(before[ALL_PAIRS], before[CELLS]))
    tag0 = st.tag[: st.N].cpu().numpy().copy()
    azp.ParticleSorter(particles_per_block=16).sort(sim)
    assert not np.array_equal(st.tag[: st.N].cpu().numpy(), tag0)  # (the rows moved)
    for path in computes:
        after = by_tag(path)
        assert all(np.array_equal(a, b) for a, b in zip(before[path], after)), path


# ---------------------------------------------------------------------------
# the recorder
# ---------------------------------------------------------------------------
def _liquid(recorder):
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
    c = compute.Cluster(azp.All(), 1.12, size_bins=16)  # (the lattice spacing is 1.21: thermal motion makes and breaks bonds)
    sim.operations.add(c)
    rec = None
    if recorder:
        rec = compute.ClusterRecorder(c, 10)
        sim.operations.add(rec)
    return sim, c, rec


def _bits(t):
    import torch

    return t.clone().view(torch.int64).cpu().numpy()


def test_recorder_leaves_the_run_unchanged_and_records_the_computes_own_rows():
    sim, c, rec = _liquid(True)
    sim.run(20)
    assert list(rec.timesteps) == [10, 20]
    table = rec._table()
    assert table.shape == (2, 22) and rec.size_histogram.shape == (2, 16)
    assert np.all(rec.num_particles == 256) and np.all((rec.size_histogram.sum(axis=1)) == rec.num_clusters)
    plain = None
    for k, stop in enumerate((10, 20)):
        plain, c2, _ = _liquid(False)
        plain.run(stop)
        row = c2._read("summary")
        assert np.array_equal(row, table[k]), stop
        assert (rec.num_clusters[k], rec.largest_cluster_size[k], rec.num_edges[k]) == (row[1], row[2], row[5])
        assert rec.weight_average_cluster_size[k] == c2.weight_average_cluster_size
    assert np.array_equal(_bits(sim.state.pos), _bits(plain.state.pos))
    assert np.array_equal(_bits(sim.state.vel), _bits(plain.state.vel))
    assert 1 < table[0, 1] < 256 and not np.array_equal(table[0], table[1])  # (clusters of several sizes; the liquid moved)
    rec.reset()
    assert rec.timesteps.shape == (0,) and rec.num_clusters.shape == (0,) and rec.size_histogram.shape == (0, 16)


# ---------------------------------------------------------------------------
# refusals before any launch
# ---------------------------------------------------------------------------
def test_refusals_when_read():
    f = _fixture("sc")
    sim = _sim(f)
    c = compute.Cluster(azp.All(), 4.5)  # the box is 8 wide
    sim.operations.add(c)
    with pytest.raises(_lib.AzpError, match="minimum image"):
        c.num_clusters
    c = compute.Cluster(azp.All(), 3.0)
    c.path = CELLS  # two cells per axis
    sim.operations.add(c)
    with pytest.raises(_lib.AzpError):
        c.cluster_keys
    c = _cluster(sim, f, None, 0)
    sim.domain = object()  # (a decomposed run: refused before the state is looked at)
    try:
        with pytest.raises(_lib.AzpError, match="decomposed"):
            c.num_clusters
    finally:
        sim.domain = None
    assert c.num_clusters == 1
