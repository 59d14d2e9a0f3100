"""compute.Cluster without a GPU: the fixtures' own conditions (no pair within 1e-9 of r_max^2, so that every integer the
device reports has to be the reference's), the figures of tests/cluster_fixtures.py re-derived, the reference
(tests/cluster_ref.py) against hand-built answers, ``cluster_indices``, the refusals of the constructors and of the C
entry (which come before any launch and touch no device), and the bookkeeping of the recorder."""

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import cluster_fixtures as fx
import cluster_ref as ref
import steinhardt_fixtures as sf
import steinhardt_ref

import azplugins_amd as azp
from azplugins_amd import _lib, compute

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = -1  # AZP_ERROR_INVALID_ARGUMENT
NONE = _lib.CLUSTER_NONE


def _reference(f, group=None, **kw):
    return ref.reference(f["xyz"], f["types"], f["box"], sf.mask(group), f["r_max"], tags=fx.tags_of(f), **kw)


# ---------------------------------------------------------------------------
# the fixtures
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(fx.FIXTURES))
def test_fixtures_meet_their_condition(name):
    f = fx.FIXTURES[name]()
    L, tilt, periodic = f["box"]
    widths = compute.perpendicular_widths(azp.Box(L[0], L[1], L[2], tilt[0], tilt[1], tilt[2], periodic=periodic))
    assert all(f["r_max"] <= 0.5 * w for w, p in zip(widths, periodic) if p)
    for group in fx.GROUPS:
        assert ref.edge_gap(f["xyz"], f["types"], f["box"], sf.mask(group), f["r_max"]) >= 1e-9
    assert np.unique(fx.tags_of(f)).shape[0] == f["xyz"].shape[0]


@pytest.mark.parametrize("name", sorted(fx.PERCOLATION))
def test_percolation_figures(name):
    _, r_max, clusters, edges, largest = fx.PERCOLATION[name]
    f = fx.FIXTURES[name]()
    assert f["r_max"] == r_max
    assert ref.edge_gap(f["xyz"], f["types"], f["box"], None, r_max) >= 3e-5
    out = _reference(f)
    assert (out["num_clusters"], out["num_edges"], int(out["sizes"].max())) == (clusters, edges, largest)
    assert tuple(out["row"][[1, 5, 2]]) == (clusters, edges, largest) and out["row"][0] == f["xyz"].shape[0]
    assert out["row"][6:].sum() == clusters and out["row"][4] == (out["sizes"].astype(np.int64)).sum()
    # the group of two types is a different graph with clusters of several sizes too
    sub = _reference(f, fx.AB)
    assert 1 < sub["num_clusters"] < sub["in_group"].sum() and np.all(sub["keys"][~sub["in_group"]] == NONE)


def test_two_phase_solid_particles_meet_the_condition():
    f, p = fx.two_phase(), sf.TWO_PHASE
    st = steinhardt_ref.reference(f["xyz"], f["types"], f["box"], None, (p["l"],), f["r_max"], q_threshold=p["q_threshold"])
    assert steinhardt_ref.threshold_gap(st, p["q_threshold"]) >= 1e-6
    solid = st["num_connections"] >= p["solid_threshold"]
    assert 0 < solid.sum() < solid.shape[0]
    assert ref.edge_gap(f["xyz"], f["types"], f["box"], None, f["r_max"], member=solid) >= 1e-9
    out = _reference(f, member=solid)
    assert out["row"][0] == solid.sum() == 138 and np.all(out["keys"][~solid] == NONE) and tuple(out["row"][1:3]) == (1, 138)
    assert ref.edge_gap(f["xyz"], f["types"], f["box"], None, fx.TWO_PHASE_R_MAX, member=solid) >= 1e-9
    f["r_max"] = fx.TWO_PHASE_R_MAX
    assert tuple(_reference(f, member=solid)["row"][:3]) == (138, 11, 123)


# ---------------------------------------------------------------------------
# the reference against hand-built answers
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("tags", fx.RING_TAGS)
def test_ring_is_one_cluster_through_the_boundary(tags):
    f = fx.ring(tags)
    out = _reference(f)
    assert np.all(out["keys"] == 0) and np.all(out["sizes"] == 600) and np.all(out["idx"] == 0)
    want = np.zeros(6 + fx.SIZE_BINS, dtype=np.int64)
    want[:6] = [600, 1, 600, 0, 360000, 600]
    want[-1] = 1
    assert np.array_equal(out["row"], want)


def test_ring_with_particles_removed():
    f = fx.FIXTURES["ring_minus_one"]()
    out = _reference(f)
    assert f["xyz"].shape[0] == 599 and np.all(out["sizes"] == 599) and out["num_edges"] == 598
    assert np.all(out["keys"] == fx.tags_of(f).min())
    f = fx.FIXTURES["ring_minus_two"]()
    out = _reference(f)
    # positions 101 .. 349 are one piece, 351 .. 599 and 0 .. 99 (through the boundary) the other
    assert f["xyz"].shape[0] == 598 and out["num_clusters"] == 2 and out["num_edges"] == 596
    assert sorted(np.unique(out["sizes"])) == [249, 349]
    k = np.array([i for i in range(600) if i not in (100, 350)])
    assert np.all(out["sizes"][(k > 100) & (k < 350)] == 249) and np.all(out["sizes"][(k < 100) | (k > 350)] == 349)
    assert tuple(out["row"][:6]) == (598, 2, 349, out["keys"][0], 249 ** 2 + 349 ** 2, 596)


def test_bridge():
    f = fx.bridge()
    everything = _reference(f)
    assert np.all(everything["keys"] == 0) and np.all(everything["sizes"] == 10)
    two = _reference(f, fx.AB)
    assert everything["num_edges"] == two["num_edges"] + 2  # the C particle has exactly one neighbour on each side
    assert two["keys"][0] == NONE and two["sizes"][0] == 0 and two["idx"][0] == -1
    assert np.all(two["keys"][1:6] == 1) and np.all(two["sizes"][1:6] == 5) and np.all(two["idx"][1:6] == 0)
    assert np.all(two["keys"][6:] == 6) and np.all(two["sizes"][6:] == 4) and np.all(two["idx"][6:] == 1)
    assert tuple(two["row"][:5]) == (9, 2, 5, 1, 41) and two["row"][6 + 4] == 1 and two["row"][6 + 3] == 1


def test_simple_cubic_lattice_blob_and_single():
    out = _reference(fx.FIXTURES["sc"]())
    assert tuple(out["row"][:6]) == (64, 1, 64, 0, 4096, 192) and out["row"][-1] == 1
    out = _reference(fx.sc_singletons())
    # 64 clusters of one: among equal sizes the largest cluster's key is the smallest tag
    assert tuple(out["row"][:7]) == (64, 64, 1, 0, 64, 0, 64) and np.array_equal(out["idx"], np.arange(64))
    assert np.array_equal(out["keys"], np.arange(64))
    out = _reference(fx.FIXTURES["blob"]())
    assert tuple(out["row"][:6]) == (300, 1, 300, 0, 90000, 44850)
    out = _reference(fx.FIXTURES["sparse"]())
    assert out["row"][6] > out["row"][1] // 2  # mostly singletons
    out = _reference(fx.single())
    assert tuple(out["row"][:7]) == (1, 1, 1, 0, 1, 0, 1)
    empty = _reference(fx.FIXTURES["sc"](), ("C",))
    want = np.zeros(6 + fx.SIZE_BINS, dtype=np.int64)
    want[3] = -1
    assert np.array_equal(empty["row"], want) and np.all(empty["keys"] == NONE) and np.all(empty["idx"] == -1)


# ---------------------------------------------------------------------------
# cluster_indices and the summary row
# ---------------------------------------------------------------------------
def test_cluster_indices_ordering_ties_and_outside():
    keys = np.array([7, 2, NONE, 7, 5, 2, 7, 9, NONE, 3], dtype=np.uint32)
    sizes = np.array([3, 2, 0, 3, 1, 2, 3, 1, 0, 1], dtype=np.uint32)
    # 7 (size 3) first, then 2 (size 2), then the singletons 3, 5, 9 by ascending key
    want = np.array([0, 1, -1, 0, 3, 1, 0, 4, -1, 2])
    got = compute.cluster_indices(keys, sizes)
    assert got.dtype == np.int64 and np.array_equal(got, want) and np.array_equal(ref.indices(keys, sizes), want)
    assert np.array_equal(compute.cluster_indices(np.array([5, 1], dtype=np.uint32), [2, 2]), [1, 0])  # a tie: by key
    assert compute.cluster_indices(np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32)).shape == (0,)
    assert np.array_equal(compute.cluster_indices([NONE, NONE], [0, 0]), [-1, -1])
    with pytest.raises(_lib.AzpError):
        compute.cluster_indices([1, 2], [1])
    for name in ("cube515_hi", "bridge", "sc_singletons"):
        out = _reference(fx.FIXTURES[name](), fx.AB)
        assert np.array_equal(compute.cluster_indices(out["keys"], out["sizes"]), out["idx"])


def test_summary_row_parsing():
    row = np.arange(6 + 5, dtype=np.int64) + 10
    s = compute.cluster_summary(row, 5)
    assert (s["num_particles"], s["num_clusters"], s["largest_cluster_size"], s["largest_cluster_key"], s["sum_size_squared"],
            s["num_edges"]) == (10, 11, 12, 13, 14, 15)
    assert np.array_equal(s["size_histogram"], [16, 17, 18, 19, 20])
    with pytest.raises(_lib.AzpError):
        compute.cluster_summary(row, 6)


# ---------------------------------------------------------------------------
# the Python layer
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(filter=None), dict(filter="all"), dict(r_max=0.0), dict(r_max=-1.0), dict(r_max=float("nan")),
                                dict(r_max=float("inf")), dict(r_max="x"), dict(size_bins=0), dict(size_bins=1025), dict(size_bins=2.5),
                                dict(size_bins=True), dict(solid="solid"),
                                dict(solid=compute.Steinhardt(azp.All(), 6, 1.5))])
def test_constructor_refuses(kw):
    args = dict(filter=azp.All(), r_max=1.5)
    args.update(kw)
    with pytest.raises(_lib.AzpError):
        compute.Cluster(**args)


def test_accepted_arguments_and_path():
    sl = compute.SolidLiquid(azp.All(), 6, 1.5, 0.7, 6)
    c = compute.Cluster(azp.Type(["A", "B"]), 1.25, solid=sl, size_bins=1024)
    assert c.r_max == 1.25 and c.solid is sl and c.size_bins == 1024 and c.path == 0 and c._row_width() == 1030
    assert compute.Cluster(azp.All(), 1).size_bins == 64
    for p in (0, 1, 2):
        c.path = p
        assert c.path == p
    for p in (3, -1, "cells", None, True):
        with pytest.raises(_lib.AzpError):
            c.path = p
    with pytest.raises(_lib.AzpError):
        compute.ClusterRecorder(sl, 10)


def _fake_sim(box, domain=None):
    import types

    return types.SimpleNamespace(state=types.SimpleNamespace(box=box), domain=domain)


def test_box_and_domain_refusals():
    c = compute.Cluster(azp.All(), 4.0)
    c._check_box(_fake_sim(azp.Box(8.0, 9.0, 10.0)))  # exactly half the smallest width
    c._check_box(_fake_sim(azp.Box(7.0, 9.0, 10.0, periodic=(False, True, True))))
    with pytest.raises(_lib.AzpError, match="minimum image"):
        c._check_box(_fake_sim(azp.Box(7.9, 9.0, 10.0)))
    with pytest.raises(_lib.AzpError, match="minimum image"):
        compute.Cluster(azp.All(), 3.6)._check_box(_fake_sim(azp.Box(8.0, 9.0, 10.0, xy=0.5)))
    with pytest.raises(_lib.AzpError, match="decomposed"):
        c._check_box(_fake_sim(azp.Box(20.0), domain=object()))


def test_unattached_reads_raise_data_access_error():
    c = compute.Cluster(azp.All(), 1.5)
    names = ("cluster_keys", "cluster_sizes", "cluster_idx", "num_particles", "num_clusters", "largest_cluster_size",
             "largest_cluster_key", "num_edges", "mean_cluster_size", "weight_average_cluster_size", "size_histogram")
    for name in names:
        with pytest.raises(compute.DataAccessError):
            getattr(c, name)
    sim = azp.Simulation(device="cuda:0")
    sim.operations.add(c)  # in the list, but the simulation has no state
    with pytest.raises(compute.DataAccessError):
        c.num_clusters


def test_recorder_bookkeeping():
    c = compute.Cluster(azp.All(), 1.5, size_bins=8)
    r = compute.ClusterRecorder(c, 10)
    assert r.cluster is c and r._compute is c and r._row_width() == 14 and r._dtype == "int64"
    assert r.timesteps_in_run(0, 25) == [10, 20]
    assert r.timesteps.shape == (0,) and r.num_clusters.shape == (0,) and r.largest_cluster_size.shape == (0,)
    assert r.num_edges.shape == (0,) and r.weight_average_cluster_size.shape == (0,) and r.size_histogram.shape == (0, 8)
    r.reset()
    assert r.timesteps.shape == (0,)


# ---------------------------------------------------------------------------
# the C entry
# ---------------------------------------------------------------------------
def _c_args(L=(8.0, 8.0, 8.0), tilt=sf.ORTHO, periodic=sf.PBC, r_max=2.0, path=0, n=100, size_bins=64, stages=0):
    a = _lib.ClusterArgs()
    a.N = n
    a.ntypes = 1
    a.box = _lib.make_box(L, tilt, periodic)
    a.r_max = r_max
    a.path = path
    a.size_bins = size_bins
    a.stages = stages
    return a


def test_c_abi_refuses_before_anything_is_launched():
    """azp_cluster_scratch_size runs the checks of azp_cluster_compute and touches no device."""
    lib = _lib.lib()
    need = C.c_uint64(0)

    def rc(**kw):
        return lib.azp_cluster_scratch_size(C.byref(_c_args(**kw)), C.byref(need))

    assert rc() == 0 and need.value >= 100 * (32 + 4 * 4)
    cells = need.value
    assert rc(path=1) == 0 and 100 * (32 + 4 * 4) <= need.value < cells  # no cell tables
    assert rc(n=0) == 0
    assert rc(r_max=0.0) == BAD and rc(r_max=-1.0) == BAD and rc(r_max=float("nan")) == BAD and rc(r_max=float("inf")) == BAD
    assert rc(size_bins=0) == BAD and rc(size_bins=1025) == BAD and rc(size_bins=1024) == 0 and rc(size_bins=1) == 0
    assert rc(n=_lib.CLUSTER_MAX_N + 1) == BAD and rc(n=_lib.CLUSTER_MAX_N, path=1) == 0
    assert need.value >= _lib.CLUSTER_MAX_N * 48  # (the plan's arithmetic is 64-bit)
    assert rc(n=_lib.CLUSTER_MAX_N) == 0
    assert rc(L=(8.0, 0.0, 8.0)) == BAD
    assert rc(r_max=float(np.nextafter(4.0, 5.0))) == BAD and rc(r_max=4.0) == 0
    assert rc(r_max=5.0, periodic=(0, 0, 0)) == 0
    assert rc(path=3) == BAD and rc(stages=3) == BAD and rc(stages=2) == 0
    assert rc(r_max=3.0, path=2) == BAD and rc(r_max=3.0, path=0) == 0  # two cells per axis
    assert rc(tilt=(0.1, 0.0, 0.0), path=2) == BAD and rc(tilt=(0.1, 0.0, 0.0), path=0) == 0
    assert rc(L=(8.0, 8.0, 3.0), periodic=(1, 1, 0), path=2) == 0  # a short non-periodic axis has clamped cells
    a = _c_args()
    a.d_type_mask = 1
    a.ntypes = 0
    assert lib.azp_cluster_scratch_size(C.byref(a), C.byref(need)) == BAD
    assert lib.azp_cluster_scratch_size(None, C.byref(need)) == BAD
    assert lib.azp_cluster_scratch_size(C.byref(_c_args()), None) == BAD
    # azp_cluster_compute itself refuses the same way, and a NULL output, before it reads a pointer
    assert lib.azp_cluster_compute(None, None) == BAD
    assert lib.azp_cluster_compute(C.byref(_c_args(r_max=0.0)), None) == BAD
    assert lib.azp_cluster_compute(C.byref(_c_args(path=2, r_max=3.0)), None) == BAD
    assert lib.azp_cluster_compute(C.byref(_c_args()), None) == BAD  # NULL d_summary
    a = _c_args()
    a.d_summary = 8
    assert lib.azp_cluster_compute(C.byref(a), None) == BAD  # NULL d_pos and outputs with N > 0


def test_abi_struct_matches_the_header():
    fields = ("box", "d_type_mask", "d_tag", "d_member", "member_min", "path", "r_max", "size_bins", "stages", "d_cluster_key",
              "d_cluster_size", "d_summary", "d_scratch", "scratch_bytes")
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "azp.h"\nint main(){printf("%zu %u %d %u\\n", sizeof(azp_cluster_args), '
           'AZP_CLUSTER_NONE, AZP_CLUSTER_MAX_BINS, AZP_CLUSTER_MAX_N);'
           + "".join('printf("%%zu\\n", offsetof(azp_cluster_args, %s));' % f for f in fields) + "return 0;}")
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "s.c"), "w") as f:
            f.write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    A = _lib.ClusterArgs
    assert got[:4] == [C.sizeof(A), _lib.CLUSTER_NONE, _lib.CLUSTER_MAX_BINS, _lib.CLUSTER_MAX_N]
    assert got[4:] == [getattr(A, f).offset for f in fields]
    assert (_lib.CLUSTER_PATH_AUTO, _lib.CLUSTER_PATH_ALL_PAIRS, _lib.CLUSTER_PATH_CELLS) == (0, 1, 2)
