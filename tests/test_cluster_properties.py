"""compute.ClusterProperties without a GPU: the conditions of the fixtures (tests/cluster_properties_fixtures.py) under
which the device has to give the references' numbers, the two references (tests/cluster_properties_ref.py) against each
other and against closed forms, ``cluster_properties_table``, the refusals of the constructors and of the C entry (which
come before any launch and touch no device), and the structs against the header."""

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import cluster_fixtures as cf
import cluster_properties_fixtures as fx
import cluster_properties_ref as pref
import cluster_ref
import steinhardt_fixtures as sf

import azplugins_amd as azp
from azplugins_amd import _lib, compute

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = -1  # AZP_ERROR_INVALID_ARGUMENT
NEW = sorted(set(fx.FIXTURES) - set(cf.FIXTURES))


# ---------------------------------------------------------------------------
# the fixtures
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", NEW)
def test_new_fixtures_meet_the_condition_of_the_cluster_fixtures(name):
    f = fx.fixture(name)
    L, tilt, periodic = f["box"]
    widths = compute.perpendicular_widths(azp.Box(L[0], L[1], L[2], tilt[0], tilt[1], tilt[2], periodic=periodic))
    assert all(f["r_max"] <= 0.5 * w for w, p in zip(widths, periodic) if p)
    for group in fx.GROUPS:
        assert cluster_ref.edge_gap(f["xyz"], f["types"], f["box"], sf.mask(group), f["r_max"]) >= 1e-9
    s = pref.fractional(f["xyz"], f["box"])
    assert np.all(s >= 0.0) and np.all(s < 1.0)  # inside the box


@pytest.mark.parametrize("name", sorted(fx.FIXTURES))
def test_fixture_conditions_and_the_two_references(name):
    f = fx.fixture(name)
    per = np.asarray(f["box"][2], dtype=bool)
    L = max(f["box"][0])
    for group in fx.GROUPS:
        out, edges, formula = fx.expected(name, group)
        assert set(edges) == set(formula) == set(int(k) for k in np.unique(out["keys"]) if k != cluster_ref.NONE)
        loose = 0
        for key, e in edges.items():
            g = formula[key]
            assert e["size"] == g["size"] == int(out["sizes"][out["keys"] == key][0])
            # no extent within 1e-6 of 1/2: the flag is the references' whatever the device rounds
            assert np.all(np.abs(e["extent"][per] - 0.5) >= 1e-6) and np.all(np.abs(g["extent"][per] - 0.5) >= 1e-6), (name, group, key)
            assert e["compact"] == g["compact"], (name, group, key)
            if not e["compact"]:
                loose += 1
                continue
            # the two references agree on a compact cluster
            assert pref.center_distance(e["center"], g["center"], f["box"]) <= 1e-13 * L, (name, group, key)
            assert np.abs(e["gyration"] - g["gyration"]).max() <= 1e-13 * L * L and abs(e["rg2"] - g["rg2"]) <= 1e-13 * L * L
            assert np.abs(e["extent"] - g["extent"]).max() <= 1e-13
        if fx.random_fixture(name):
            assert loose <= 4, (name, group, loose)
            if len(edges) >= 60:
                assert loose <= 0.07 * len(edges)  # at least 93 % go against by_edges
    if name in fx.NEVER_COMPACT:
        assert not any(e["compact"] for e in fx.expected(name, None)[1].values())


def test_one_cluster_fixtures_are_one_cluster_by_construction():
    for n in fx.ONE_CLUSTER_N:
        f = fx.one_cluster(n)
        assert f["xyz"].shape == (n, 3) and f["box"][2] == (0, 0, 0)
        assert np.linalg.norm(f["xyz"] - 1.0, axis=1).max() < 0.9  # every pair is closer than 1.8 < r_max = 2
        assert f["r_max"] == 2.0


def test_translated_fixtures_cross_the_boundary():
    for name in fx.TRANSLATED:
        base = fx.fixture(name)
        for k, d in enumerate(fx.DIRECTIONS):
            f = fx.fixture("%s_moved%d" % (name, k))
            assert np.array_equal(f["vector"] != 0.0, np.asarray(d) != 0)
            moved = base["xyz"] + f["vector"]
            for axis in np.flatnonzero(d):
                assert moved[:, axis].min() < 4.0 < moved[:, axis].max()  # some rows wrapped, some did not
            assert np.abs(f["xyz"]).max() <= 4.0


# ---------------------------------------------------------------------------
# closed forms
# ---------------------------------------------------------------------------
def test_closed_forms_hold_for_the_references():
    out, edges, formula = fx.expected("single", None)
    for r in (edges[0], formula[0]):
        assert np.allclose(r["center"], [0.5, -0.25, 1.0], rtol=0, atol=1e-15) and np.abs(r["gyration"]).max() <= 1e-30
        assert r["compact"] and r["size"] == 1
    out, edges, formula = fx.expected("ring_minus_two", None)
    key = [k for k, e in edges.items() if e["size"] == 249][0]
    want = 0.125 ** 2 * (249 ** 2 - 1) / 12.0
    for r in (edges[key], formula[key]):
        assert np.allclose(r["center"], [-9.3125, 0.25, -0.5], rtol=0, atol=1e-12)
        assert abs(r["gyration"][0, 0] - want) <= 1e-11 and abs(r["rg2"] - want) <= 1e-11
        g = r["gyration"].copy()
        g[0, 0] = 0.0
        assert np.abs(g).max() <= 1e-14 and r["compact"]
    other = [k for k, e in edges.items() if e["size"] == 349][0]
    assert not edges[other]["compact"] and not formula[other]["compact"]
    # the simple cubic lattice: circular sums of (nearly) 0 in float64, exactly 0 in the device's integers
    out, edges, formula = fx.expected("sc", None)
    assert np.all(formula[0]["resultant"] < 1e-12) and not pref.eligible(formula[0])
    # a dimer across the face: the centre is on the far side of the face from the first particle
    out, edges, formula = fx.expected("dimer", None)
    for r in (edges[0], formula[0]):
        assert pref.center_distance(r["center"], [4.125, 1.125, -2.0], fx.fixture("dimer")["box"]) <= 1e-14
        assert np.allclose(r["gyration"], np.outer([0.25, 0.125, 0.0], [0.25, 0.125, 0.0]), rtol=0, atol=1e-15)
        assert np.all(np.abs(r["center"]) <= 4.0)


def test_shift_rule():
    def shift(n):
        return min(52, 61 - int(np.ceil(np.log2(max(n, 2)))))

    assert [shift(n) for n in (0, 1, 2, 512, 513, 1030, 4096, 4097, 1 << 20, 1 << 30)] == [52, 52, 52, 52, 51, 50, 49, 48, 41, 31]
    assert all(n * 2 ** shift(n) <= 2 ** 61 for n in (2, 3, 512, 513, 4096, 4097, (1 << 30) - 1, 1 << 30))


# ---------------------------------------------------------------------------
# cluster_properties_table
# ---------------------------------------------------------------------------
def _row(key, size, seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([[key, size], rng.random(3), rng.random(6), [0.0], [seed % 2], rng.random(3)])


def test_cluster_properties_table_orders_as_freud_does():
    rows = np.array([_row(7, 3, 1), _row(2, 5, 2), _row(9, 3, 3), _row(4, 1, 4), _row(1, 3, 5), _row(99, 8, 6)])
    rows[:, 11] = rows[:, 5] + rows[:, 8] + rows[:, 10]
    summary = np.concatenate([[5, 15, 52, 0], rows[1]])  # (the sixth row is behind summary[0]: not part of the table)
    t = compute.cluster_properties_table(rows, summary)
    assert t["num_clusters"] == 5 and t["num_particles"] == 15 and t["shift"] == 52
    assert list(t["keys"]) == [2, 1, 7, 9, 4] and list(t["sizes"]) == [5, 3, 3, 3, 1]
    assert t["keys"].dtype == np.int64 and t["sizes"].dtype == np.int64 and t["compact"].dtype == np.bool_
    order = [1, 4, 0, 2, 3]
    assert np.array_equal(t["centers"], rows[order, 2:5]) and np.array_equal(t["extents"], rows[order, 13:16])
    assert np.array_equal(t["compact"], rows[order, 12] != 0)
    g = t["gyrations"]
    assert g.shape == (5, 3, 3) and np.array_equal(g, np.transpose(g, (0, 2, 1)))
    assert np.array_equal(g[:, 0, 0], rows[order, 5]) and np.array_equal(g[:, 0, 1], rows[order, 6])
    assert np.array_equal(g[:, 0, 2], rows[order, 7]) and np.array_equal(g[:, 1, 1], rows[order, 8])
    assert np.array_equal(g[:, 1, 2], rows[order, 9]) and np.array_equal(g[:, 2, 2], rows[order, 10])
    assert np.array_equal(t["radii_of_gyration"], np.sqrt(rows[order, 11]))
    big = t["largest"]
    assert big["key"] == 2 and big["size"] == 5 and np.array_equal(big["center"], rows[1, 2:5]) and big["compact"] == bool(rows[1, 12])
    assert np.array_equal(big["gyration"], g[0]) and big["radius_of_gyration"] == np.sqrt(rows[1, 11])
    # no rows
    empty = np.zeros(20)
    empty[2], empty[4] = 52, -1
    t = compute.cluster_properties_table(np.zeros((0, 16)), empty)
    assert t["num_clusters"] == 0 and t["keys"].shape == (0,) and t["centers"].shape == (0, 3) and t["gyrations"].shape == (0, 3, 3)
    assert t["largest"]["key"] == -1 and t["largest"]["size"] == 0
    for bad in ((rows[:, :15], summary), (rows, summary[:19]), (rows[:3], summary)):
        with pytest.raises(_lib.AzpError):
            compute.cluster_properties_table(*bad)


# ---------------------------------------------------------------------------
# the Python layer
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(cluster=None), dict(cluster="cluster"), dict(cluster=compute.SolidLiquid(azp.All(), 6, 1.5, 0.7, 6)),
                                dict(min_size=0), dict(min_size=-1), dict(min_size=2.0), dict(min_size=True), dict(min_size="2"),
                                dict(min_size=None), dict(min_size=1 << 32)])
def test_constructor_refuses(kw):
    args = dict(cluster=compute.Cluster(azp.All(), 1.5))
    args.update(kw)
    with pytest.raises(_lib.AzpError):
        compute.ClusterProperties(**args)


def test_accepted_arguments_unattached_reads_and_the_recorder():
    c = compute.Cluster(azp.All(), 1.5)
    p = compute.ClusterProperties(c)
    assert p.cluster is c and p.min_size == 1 and p._row_width() == 20
    assert compute.ClusterProperties(c, min_size=np.int64(7)).min_size == 7
    names = ("num_clusters", "keys", "sizes", "centers", "gyrations", "radii_of_gyration", "compact", "extents",
             "principal_moments", "relative_shape_anisotropy", "largest")
    for name in names:
        with pytest.raises(compute.DataAccessError):
            getattr(p, name)
    sim = azp.Simulation(device="cuda:0")
    sim.operations.add(p)  # in the list, but the simulation has no state
    with pytest.raises(compute.DataAccessError):
        p.num_clusters
    for bad in (c, None, "props"):
        with pytest.raises(_lib.AzpError):
            compute.ClusterPropertiesRecorder(bad, 10)
    r = compute.ClusterPropertiesRecorder(p, 10)
    assert r.props is p and r._compute is p and r._row_width() == 20 and r._dtype == "float64"
    assert r.timesteps_in_run(0, 25) == [10, 20]
    assert r.timesteps.shape == (0,) and r.num_clusters.shape == (0,) and r.largest_cluster_size.shape == (0,)
    assert r.largest_cluster_key.shape == (0,) and r.largest_center.shape == (0, 3) and r.largest_gyration.shape == (0, 3, 3)
    assert r.largest_radius_of_gyration.shape == (0,) and r.largest_compact.shape == (0,)
    r.reset()
    assert r.timesteps.shape == (0,)


# ---------------------------------------------------------------------------
# the C entry
# ---------------------------------------------------------------------------
def _c_args(L=(8.0, 8.0, 8.0), tilt=sf.ORTHO, periodic=sf.PBC, n=100, min_size=1):
    a = _lib.ClusterPropertiesArgs()
    a.N = n
    a.min_size = min_size
    a.box = _lib.make_box(L, tilt, periodic)
    return a


def test_c_abi_refuses_before_anything_is_launched():
    """azp_cluster_properties_scratch_size runs the checks of azp_cluster_properties and touches no device."""
    lib = _lib.lib()
    need = C.c_uint64(0)

    def rc(**kw):
        return lib.azp_cluster_properties_scratch_size(C.byref(_c_args(**kw)), C.byref(need))

    assert rc() == 0 and need.value >= 100 * (4 + 4 + 21 * 8)
    whole = need.value
    assert rc(min_size=10) == 0 and need.value < whole  # ten rows at the most
    assert rc(min_size=101) == 0 and rc(n=0) == 0
    assert rc(min_size=0) == BAD
    assert rc(n=_lib.CLUSTER_MAX_N + 1) == BAD and rc(n=_lib.CLUSTER_MAX_N) == 0
    assert need.value >= _lib.CLUSTER_MAX_N * (4 + 4 + 21 * 8)  # (the plan's arithmetic is 64-bit)
    assert rc(L=(8.0, 0.0, 8.0)) == BAD and rc(L=(8.0, 8.0, -1.0)) == BAD and rc(L=(float("nan"), 8.0, 8.0)) == BAD
    assert rc(tilt=(0.2, -0.1, 0.3)) == 0 and rc(periodic=(0, 0, 0)) == 0
    assert lib.azp_cluster_properties_scratch_size(None, C.byref(need)) == BAD
    assert lib.azp_cluster_properties_scratch_size(C.byref(_c_args()), None) == BAD
    # azp_cluster_properties itself refuses the same way, and a NULL output, before it reads a pointer
    assert lib.azp_cluster_properties(None, None) == BAD
    assert lib.azp_cluster_properties(C.byref(_c_args(min_size=0)), None) == BAD
    assert lib.azp_cluster_properties(C.byref(_c_args()), None) == BAD  # NULL d_summary
    a = _c_args()
    a.d_summary = 8
    assert lib.azp_cluster_properties(C.byref(a), None) == BAD  # NULL d_pos and labels with N > 0


def _offsets(struct, fields, consts):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "azp.h"\nint main(){printf("%%zu\\n", sizeof(%s));' % struct
           + "".join('printf("%%lld\\n", (long long)%s);' % c for c in consts)
           + "".join('printf("%%zu\\n", offsetof(%s, %s));' % (struct, f) for f in fields) + "return 0;}")
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "s.c"), "w") as f:
            f.write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        return [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]


def test_abi_structs_match_the_header():
    fields = ("d_pos", "N", "min_size", "box", "d_cluster_rep", "d_cluster_key", "d_cluster_size", "d_table", "d_summary",
              "d_scratch", "scratch_bytes")
    got = _offsets("azp_cluster_properties_args", fields, ("AZP_CLUSTER_PROPERTIES_ROW", "AZP_CLUSTER_PROPERTIES_SUMMARY"))
    A = _lib.ClusterPropertiesArgs
    assert got[:3] == [C.sizeof(A), _lib.CLUSTER_PROPERTIES_ROW, _lib.CLUSTER_PROPERTIES_SUMMARY] and got[1:3] == [16, 20]
    assert got[3:] == [getattr(A, f).offset for f in fields]
    # the field added to azp_cluster_args is its last one
    got = _offsets("azp_cluster_args", ("scratch_bytes", "d_cluster_rep"), ())
    B = _lib.ClusterArgs
    assert got == [C.sizeof(B), B.scratch_bytes.offset, B.d_cluster_rep.offset]
    assert B.d_cluster_rep.offset + 8 == C.sizeof(B) and B._fields_[-1][0] == "d_cluster_rep"
