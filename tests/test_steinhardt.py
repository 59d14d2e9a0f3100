"""compute.Steinhardt / compute.SolidLiquid without a GPU: the numpy reference (tests/steinhardt_ref.py) against scipy and
the known lattice values, the kernel's term arithmetic (csrc/steinhardt_device.hpp) compiled for the host against the
reference, every refusal of the Python classes and of the C ABI, the summary-row parsing, and each fixture's own
conditions (tests/steinhardt_fixtures.py)."""

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import steinhardt_fixtures as fx
import steinhardt_ref as ref

import azplugins_amd as azp
from azplugins_amd import _lib, compute

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = -1  # AZP_ERROR_INVALID_ARGUMENT


# ---------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------
def _directions(n, seed):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3)) * rng.uniform(0.3, 2.0, size=(n, 1))
    poles = np.array([[0.0, 0.0, 1.3], [0.0, 0.0, -0.7], [1.0, 0.0, 0.0], [0.0, -2.0, 0.0], [1e-9, 0.0, 1.0], [0.0, 1e-200, -1.0]])
    return np.concatenate([d, poles])


@pytest.mark.parametrize("l", range(1, 13))
def test_reference_equals_scipy(l):
    """Every (l, m >= 0), the poles (0, 0, +-z) included, to 1e-13."""
    from scipy.special import sph_harm_y

    d = _directions(200, l)
    # (the polar angle by atan2: acos(z / r) loses half the digits next to a pole)
    theta, phi = np.arctan2(np.hypot(d[:, 0], d[:, 1]), d[:, 2]), np.arctan2(d[:, 1], d[:, 0])
    worst = 0.0
    for m in range(l + 1):
        re, im = ref.ylm_complex(d, l, m)
        y = sph_harm_y(l, m, theta, phi)
        worst = max(worst, float(np.abs(re.astype(np.float64) - y.real).max()), float(np.abs(im.astype(np.float64) - y.imag).max()))
    assert worst < 1e-13, worst


@pytest.mark.parametrize("name", sorted(fx.LATTICES))
def test_reference_gives_the_lattice_values(name):
    _, r_max, neighbours, expect = fx.LATTICES[name]
    f = fx.lattice(name)
    out = ref.reference(f["xyz"], f["types"], f["box"], None, (4, 6), r_max)
    assert np.all(out["num_neighbors"] == neighbours)
    assert np.abs(out["q"] - np.array(expect)).max() < 1e-6
    assert np.abs(out["qbar"] - np.array(expect)).max() < 1e-6  # every particle has the same q_lm


def test_reference_counts_only_the_group():
    f = fx.random(257)
    m = fx.mask(fx.AB)
    out = ref.reference(f["xyz"], f["types"], f["box"], m, (4,), f["r_max"])
    outside = f["types"] == 2
    assert outside.any() and np.all(out["num_neighbors"][outside] == 0) and np.all(out["q"][outside] == 0.0)
    assert np.all(out["T"][outside] == 0) and np.all(out["qbar"][outside] == 0.0)
    sub = ref.reference(f["xyz"][~outside], f["types"][~outside], f["box"], None, (4,), f["r_max"])
    assert np.array_equal(sub["num_neighbors"], out["num_neighbors"][~outside])
    assert np.array_equal(sub["q"], out["q"][~outside])


# ---------------------------------------------------------------------------
# the fixtures' own conditions
# ---------------------------------------------------------------------------
def _all_fixtures():
    out = {name: (fx.lattice(name), (None,)) for name in fx.LATTICES}
    out.update({name: (fx.random(*args), (None, fx.AB)) for name, args in fx.RANDOM.items()})
    out.update(sparse=(fx.sparse(), (None,)), blob=(fx.blob(), (None,)), two_phase=(fx.two_phase(), (None,)))
    return out


def _histogram_gap(q, num_bins=fx.NUM_BINS):
    """Distance of q num_bins from the nearest INTERIOR bin edge: 0 and 1 are no edges (q >= 0, and the last bin is
    clamped)."""
    s = np.asarray(q * num_bins).ravel()
    k = np.rint(s)
    inner = (k > 0) & (k < num_bins)
    return float(np.abs(s - k)[inner].min()) if inner.any() else np.inf


@pytest.mark.parametrize("name", sorted(_all_fixtures()))
def test_fixtures_meet_their_conditions(name):
    f, groups = _all_fixtures()[name]
    dyadic = name in fx.LATTICES
    for group in groups:
        m = fx.mask(group)
        if not dyadic:  # (a lattice's separations are exact: an edge could not move)
            assert ref.edge_gap(f["xyz"], f["types"], f["box"], m, f["r_max"]) >= 1e-9
        for l in ((4, 6), (1, 12)):
            out = ref.reference(f["xyz"], f["types"], f["box"], m, l, f["r_max"])
            g = out["in_group"]
            for key in ("q", "qbar"):
                assert _histogram_gap(out[key][g]) > 1e-8, (group, l, key)
    if name == "sparse":
        assert (out["num_neighbors"] == 0).any() and (out["num_neighbors"] > 0).any()
    if name == "blob":
        assert np.all(out["num_neighbors"] == 299)
        cell = np.floor((f["xyz"] + 4.0) / 2.0)
        assert np.all(cell == cell[0])  # one cell of the 4^3 grid
    if name.startswith("cube"):
        assert 1 <= out["num_neighbors"][out["in_group"]].min() and out["num_neighbors"].max() <= 64


def test_two_phase_fixture_has_both_phases_and_no_bond_on_the_threshold():
    f, p = fx.two_phase(), fx.TWO_PHASE
    out = ref.reference(f["xyz"], f["types"], f["box"], None, (p["l"],), f["r_max"], q_threshold=p["q_threshold"])
    assert ref.threshold_gap(out, p["q_threshold"]) >= 1e-6
    solid = out["num_connections"] >= p["solid_threshold"]
    assert 0 < solid.sum() < solid.shape[0]
    assert solid[f["xyz"][:, 0] < -1.0].mean() > 0.9 and solid[f["xyz"][:, 0] > 1.0].mean() < 0.5


def test_fcc_bonds_are_all_solid():
    f = fx.lattice("fcc")
    out = ref.reference(f["xyz"], f["types"], f["box"], None, (6,), f["r_max"], q_threshold=0.7)
    assert ref.threshold_gap(out, 0.7) >= 1e-6 and np.all(out["num_connections"] == 12)


# ---------------------------------------------------------------------------
# the kernel's arithmetic on the host
# ---------------------------------------------------------------------------
_HOST_PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "steinhardt_device.hpp"
// in : n_terms, l[4] (uint32), norm[4][13] (double), n (uint64), n x 3 doubles
// out: n x words int64, then n x n_terms doubles: q_l of the single bond (N_b = 1)
struct Store { long long* row; void operator()(uint32_t w, long long v) const { row[w] += v; } };
int main(int argc, char** argv)
    {
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint32_t head[5];
    double norm[4][13];
    unsigned long long n;
    if (fread(head, 4, 5, in) != 5 || fread(norm, 8, 52, in) != 52 || fread(&n, 8, 1, in) != 1) return 3;
    azp::SteinhardtTerms s;
    if (!azp::steinhardt_make_terms(head[0], head + 1, norm, s)) return 4;
    std::vector<double> d(3 * n);
    if (fread(d.data(), 8, 3 * n, in) != 3 * n) return 5;
    std::vector<long long> w(n * s.words, 0);
    std::vector<double> q(n * s.n_terms);
    for (unsigned long long i = 0; i < n; ++i)
        {
        const double x = d[3 * i], y = d[3 * i + 1], z = d[3 * i + 2];
        azp::steinhardt_term(s, x, y, z, x * x + y * y + z * z, Store{w.data() + i * s.words});
        for (uint32_t t = 0; t < s.n_terms; ++t)
            q[i * s.n_terms + t] = azp::steinhardt_ql(w.data() + i * s.words + s.offset[t], s.l[t], 1.0);
        }
    fwrite(w.data(), 8, w.size(), out);
    fwrite(q.data(), 8, q.size(), out);
    fclose(out);
    return 0;
    }
"""


@pytest.fixture(scope="module")
def host_program():
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "st.cpp"), os.path.join(d, "st")
        with open(src, "w") as f:
            f.write(_HOST_PROGRAM)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=on", "-I", os.path.join(ROOT, "azplugins_amd", "csrc"),
                               src, "-o", exe])

        def run(l, disp):
            words = compute.steinhardt_words(l)[0]
            head = np.zeros(5, dtype=np.uint32)
            head[0] = len(l)
            head[1:1 + len(l)] = l
            norm = np.zeros((4, 13))
            for t, x in enumerate(l):
                norm[t, : x + 1] = compute.steinhardt_norms(x)
            with open(os.path.join(d, "in"), "wb") as f:
                f.write(head.tobytes() + norm.tobytes() + np.uint64(disp.shape[0]).tobytes() + np.ascontiguousarray(disp).tobytes())
            subprocess.check_call([exe, os.path.join(d, "in"), os.path.join(d, "out")])
            raw = np.fromfile(os.path.join(d, "out"), dtype=np.int64)
            n = disp.shape[0]
            return raw[: n * words].reshape(n, words), raw[n * words:].view(np.float64).reshape(n, len(l))

        yield run


@pytest.mark.parametrize("l", [(4, 6), (1, 12), (12, 11, 10, 9), (2, 3, 5, 8), (7,)])
def test_host_build_of_the_term_is_within_one_unit_of_the_reference(host_program, l):
    """2,000 random displacements and the poles: every quantised word within 1 unit of 2^-40 of the exact value (0.5
    of it is the quantisation); the worst evaluation error is printed (DESIGN 4.28 records it). A single bond has
    q_l = 1 (the addition theorem), which checks the finish arithmetic."""
    d = _directions(2000, 99)
    words, q = host_program(l, d)
    exact = ref.ylm(d, l) * ref.FIXED
    err = np.abs(words.astype(ref.LD) - exact).astype(np.float64)
    evaluation = max(err.max() - 0.5, 0.0)
    print("l = %r: worst |word - exact| = %.4f units of 2^-40, i.e. evaluation error <= %.4f" % (l, err.max(), evaluation))
    assert err.max() <= 1.0
    assert err.max() < 0.6  # the evaluation error itself is far below the 0.5 the GPU bounds allow it
    assert np.abs(q - 1.0).max() < 6.0 / 2.0 ** 40
    zero = host_program(l, np.zeros((1, 3)))[0]
    assert not zero.any()  # a bond of length 0 adds no term


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(l=0), dict(l=13), dict(l=(4, 4)), dict(l=()), dict(l=(1, 2, 3, 4, 5)), dict(l=4.0), dict(l=(4, 6.5)),
                                dict(l="6"), dict(l=True), dict(l=None), dict(r_max=0.0), dict(r_max=-1.0), dict(r_max=float("nan")),
                                dict(r_max=float("inf")), dict(num_bins=0), dict(num_bins=1025), dict(num_bins=2.5),
                                dict(filter=None), dict(filter="A"), dict(filter=object())])
def test_steinhardt_constructor_refuses(kw):
    args = dict(filter=azp.All(), l=(4, 6), r_max=1.5)
    args.update(kw)
    with pytest.raises(_lib.AzpError):
        compute.Steinhardt(**args)


@pytest.mark.parametrize("kw", [dict(l=(4, 6)), dict(l=(6,)), dict(l=0), dict(l=13), dict(r_max=0.0), dict(q_threshold=1.5),
                                dict(q_threshold=-1.5), dict(q_threshold=float("nan")), dict(q_threshold="x"), dict(solid_threshold=0),
                                dict(solid_threshold=-1), dict(solid_threshold=6.5), dict(solid_threshold=True), dict(filter=None)])
def test_solid_liquid_constructor_refuses(kw):
    args = dict(filter=azp.All(), l=6, r_max=1.5, q_threshold=0.7, solid_threshold=6)
    args.update(kw)
    with pytest.raises(_lib.AzpError):
        compute.SolidLiquid(**args)


def test_accepted_arguments_and_path():
    s = compute.Steinhardt(azp.Type(["A", "B"]), 6, 1.5, average=True, num_bins=1024)
    assert s.l == (6,) and s.average and s.num_bins == 1024 and s.r_max == 1.5 and s.path == 0
    assert np.array_equal(s.bin_edges, np.linspace(0.0, 1.0, 1025))
    assert compute.Steinhardt(azp.All(), (12, 1, 7, 3), 2.0).l == (12, 1, 7, 3)
    for bad in (3, -1, "cells"):
        with pytest.raises(_lib.AzpError):
            s.path = bad
    s.path = _lib.STEINHARDT_PATH_CELLS
    q = compute.SolidLiquid(azp.All(), np.int64(6), 1.5, -1.0, 1)
    assert q.l == (6,) and q.q_threshold == -1.0 and q.solid_threshold == 1


def _fake_sim(box, domain=None):
    import types

    return types.SimpleNamespace(state=types.SimpleNamespace(box=box), domain=domain)


def test_box_and_domain_refusals():
    s = compute.Steinhardt(azp.All(), (4, 6), 4.0)
    s._check_box(_fake_sim(azp.Box(8.0, 9.0, 10.0)))  # exactly half the smallest width
    s._check_box(_fake_sim(azp.Box(7.0, 9.0, 10.0, periodic=(False, True, True))))
    with pytest.raises(_lib.AzpError, match="minimum image"):
        s._check_box(_fake_sim(azp.Box(7.9, 9.0, 10.0)))
    with pytest.raises(_lib.AzpError, match="minimum image"):
        compute.Steinhardt(azp.All(), 6, 3.6)._check_box(_fake_sim(azp.Box(8.0, 9.0, 10.0, xy=0.5)))
    for c in (s, compute.SolidLiquid(azp.All(), 6, 1.5, 0.7, 6)):
        with pytest.raises(_lib.AzpError, match="decomposed"):
            c._check_box(_fake_sim(azp.Box(20.0), domain=object()))


def test_unattached_reads_raise_data_access_error():
    s = compute.Steinhardt(azp.All(), (4, 6), 1.5)
    for name in ("num_neighbors", "particle_order", "order", "histogram"):
        with pytest.raises(compute.DataAccessError):
            getattr(s, name)
    with pytest.raises(compute.DataAccessError):
        s._read("qlm")
    q = compute.SolidLiquid(azp.All(), 6, 1.5, 0.7, 6)
    for name in ("num_connections", "solid", "num_solid", "connection_histogram"):
        with pytest.raises(compute.DataAccessError):
            getattr(q, name)
    sim = azp.Simulation(device="cuda:0")
    sim.operations.add(s)  # in the list, but the simulation has no state
    with pytest.raises(compute.DataAccessError):
        s.order


def _c_args(L=(8.0, 8.0, 8.0), tilt=fx.ORTHO, periodic=fx.PBC, r_max=2.0, l=(4, 6), flags=0, path=0, n=100, num_bins=100,
            q_threshold=0.7):
    a = _lib.SteinhardtArgs()
    a.N = n
    a.ntypes = 1
    a.box = _lib.make_box(L, tilt, periodic)
    a.r_max = r_max
    a.q_threshold = q_threshold
    a.solid_threshold = 6
    a.n_terms = len(l)
    for t, x in enumerate(l[:4]):
        a.l[t] = x
        if 0 <= x <= 12:
            for m, v in enumerate(compute.steinhardt_norms(x)):
                a.norm[t][m] = v
    a.flags = flags
    a.path = path
    a.num_bins = num_bins
    return a


def test_c_abi_refuses_before_anything_is_launched():
    """azp_steinhardt_scratch_size runs the checks of azp_steinhardt_compute and touches no device."""
    lib = _lib.lib()
    need = C.c_uint64(0)

    def rc(**kw):
        return lib.azp_steinhardt_scratch_size(C.byref(_c_args(**kw)), C.byref(need))

    assert rc() == 0 and need.value >= 100 * (32 + 24 * 8 + 4)
    cells = need.value
    assert rc(path=1) == 0 and need.value < cells  # no cell tables
    plain = need.value
    assert rc(path=1, flags=_lib.STEINHARDT_AVERAGE) == 0 and need.value > plain
    assert rc(path=1, l=(6,), flags=_lib.STEINHARDT_CONNECTIONS) == 0
    assert rc(r_max=0.0) == BAD and rc(r_max=-1.0) == BAD and rc(r_max=float("nan")) == BAD
    assert rc(l=()) == BAD and rc(l=(4, 4)) == BAD and rc(l=(0,)) == BAD and rc(l=(13,)) == BAD
    a = _c_args(l=(1, 2, 3, 4))
    a.n_terms = 5
    assert lib.azp_steinhardt_scratch_size(C.byref(a), C.byref(need)) == BAD
    a = _c_args()
    a.norm[1][3] = 0.0
    assert lib.azp_steinhardt_scratch_size(C.byref(a), C.byref(need)) == BAD  # a missing N_lm
    assert rc(flags=4) == BAD
    assert rc(flags=_lib.STEINHARDT_CONNECTIONS) == BAD  # two terms
    assert rc(l=(6,), flags=_lib.STEINHARDT_CONNECTIONS, q_threshold=float("nan")) == BAD
    assert rc(num_bins=0) == BAD and rc(num_bins=1025) == BAD and rc(num_bins=1024) == 0
    assert rc(n=_lib.STEINHARDT_MAX_N + 1) == BAD and rc(n=_lib.STEINHARDT_MAX_N) == 0
    assert rc(L=(8.0, 0.0, 8.0)) == BAD
    assert rc(r_max=float(np.nextafter(4.0, 5.0))) == BAD and rc(r_max=4.0) == 0
    assert rc(r_max=5.0, periodic=(0, 0, 0)) == 0
    assert rc(path=3) == BAD
    assert rc(r_max=3.0, path=2) == BAD and rc(r_max=3.0, path=0) == 0  # two cells per axis
    assert rc(tilt=(0.1, 0.0, 0.0), path=2) == BAD and rc(tilt=(0.1, 0.0, 0.0), path=0) == 0
    assert rc(L=(8.0, 8.0, 3.0), periodic=(1, 1, 0), path=2) == 0  # a short non-periodic axis has clamped cells
    a = _c_args()
    a.d_type_mask = 1
    a.ntypes = 0
    assert lib.azp_steinhardt_scratch_size(C.byref(a), C.byref(need)) == BAD
    assert lib.azp_steinhardt_scratch_size(None, C.byref(need)) == BAD
    assert lib.azp_steinhardt_scratch_size(C.byref(_c_args()), None) == BAD
    # azp_steinhardt_compute itself refuses the same way, and a NULL output, before it reads a pointer
    assert lib.azp_steinhardt_compute(None, None) == BAD
    assert lib.azp_steinhardt_compute(C.byref(_c_args(r_max=0.0)), None) == BAD
    assert lib.azp_steinhardt_compute(C.byref(_c_args(path=2, r_max=3.0)), None) == BAD
    assert lib.azp_steinhardt_compute(C.byref(_c_args()), None) == BAD  # NULL d_summary
    a = _c_args()
    a.d_summary = 8
    assert lib.azp_steinhardt_compute(C.byref(a), None) == BAD  # NULL d_pos and outputs with N > 0


def test_abi_struct_matches_the_header():
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "azp.h"\nint main(){printf("%zu %zu %zu %zu %d %d %d %u %d\\n", '
           'sizeof(azp_steinhardt_args), offsetof(azp_steinhardt_args, norm), offsetof(azp_steinhardt_args, flags), '
           'offsetof(azp_steinhardt_args, d_summary), AZP_STEINHARDT_MAX_TERMS, AZP_STEINHARDT_MAX_L, AZP_STEINHARDT_MAX_BINS, '
           'AZP_STEINHARDT_MAX_N, AZP_STEINHARDT_CONNECTION_BINS);return 0;}')
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "s.c"), "w") as f:
            f.write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    A = _lib.SteinhardtArgs
    assert got == [C.sizeof(A), A.norm.offset, A.flags.offset, A.d_summary.offset, _lib.STEINHARDT_MAX_TERMS, _lib.STEINHARDT_MAX_L,
                   _lib.STEINHARDT_MAX_BINS, _lib.STEINHARDT_MAX_N, _lib.STEINHARDT_CONNECTION_BINS]


# ---------------------------------------------------------------------------
# the summary row and the recorders' bookkeeping
# ---------------------------------------------------------------------------
def test_summary_row_parsing():
    nt, nb = 2, 5
    width = compute.steinhardt_summary_width(nt, nb)
    assert width == 4 + 2 * 6 + 33
    row = np.zeros(width, dtype=np.int64)
    row[:4] = (10, 8, 44, 3)
    row[4], row[5] = 5 << 40, (1 << 40) // 4 * 10  # means 0.5 and 0.25
    row[6:11] = (1, 2, 3, 4, 0)
    row[11:16] = (0, 0, 10, 0, 0)
    row[16 + 12] = 7
    row[-1] = 3
    s = compute.steinhardt_summary(row, nt, nb)
    assert (s["num_particles"], s["num_with_neighbors"], s["sum_neighbors"], s["num_solid"]) == (10, 8, 44, 3)
    assert np.array_equal(s["order"], [0.5, 0.25]) and s["order_sums"] == [5 << 40, 10 * ((1 << 40) // 4)]
    assert np.array_equal(s["histogram"], [[1, 2, 3, 4, 0], [0, 0, 10, 0, 0]])
    assert s["connection_histogram"].shape == (33,) and s["connection_histogram"][12] == 7 and s["connection_histogram"][32] == 3
    empty = compute.steinhardt_summary(np.zeros(width, dtype=np.int64), nt, nb)
    assert np.array_equal(empty["order"], [0.0, 0.0])  # an empty group: no division by zero
    for bad in (row[:-1], np.zeros((2, width), dtype=np.int64)):
        with pytest.raises(_lib.AzpError):
            compute.steinhardt_summary(bad, nt, nb)
    # the reference's own summary goes through the same layout
    f = fx.lattice("sc")
    out = ref.reference(f["xyz"], f["types"], f["box"], None, (4, 6), f["r_max"])
    s = compute.steinhardt_summary(ref.summary(out, (4, 6), 100), 2, 100)
    assert s["num_particles"] == 64 and s["sum_neighbors"] == 6 * 64 and np.abs(s["order"] - (0.763763, 0.353553)).max() < 1e-6
    assert s["histogram"][0, 76] == 64 and s["histogram"][1, 35] == 64


def test_words_layout_and_norms():
    assert compute.steinhardt_words((4, 6)) == (24, [0, 10])
    assert compute.steinhardt_words((12, 11, 10, 9)) == (92, [0, 26, 50, 72])
    n = compute.steinhardt_norms(2)
    assert n == pytest.approx([np.sqrt(5 / (4 * np.pi)), np.sqrt(5 / (24 * np.pi)), np.sqrt(5 / (96 * np.pi))], rel=1e-15)


def test_recorders_bookkeeping():
    s = compute.Steinhardt(azp.All(), (4, 6), 1.5, num_bins=10)
    q = compute.SolidLiquid(azp.All(), 6, 1.5, 0.7, 6)
    rs, rq = compute.SteinhardtRecorder(s, 10), compute.SolidLiquidRecorder(q, azp.Periodic(5, phase=2))
    assert rs.trigger == azp.Periodic(10) and rs.timesteps_in_run(0, 30) == [10, 20, 30] and rq.timesteps_in_run(0, 12) == [2, 7, 12]
    assert rs._compute is s and rq._compute is q and rs._row_width() == 4 + 2 * 11 + 33 and rq._row_width() == 4 + 2 + 33
    assert rs.timesteps.shape == (0,) and rs.order.shape == (0, 2) and rs.histogram.shape == (0, 2, 10)
    assert rq.num_solid.shape == (0,) and rq.connection_histogram.shape == (0, 33) and rq.num_particles.shape == (0,)
    rs.reset()
    rq.reset()
    for cls, arg in ((compute.SteinhardtRecorder, q), (compute.SolidLiquidRecorder, s), (compute.SteinhardtRecorder, None)):
        with pytest.raises(_lib.AzpError):
            cls(arg, 10)
    sim = azp.Simulation(device="cuda:0")
    for op in (s, q, rs, rq):
        sim.operations.add(op)
    assert sim.operations.writers == [rs, rq] and [c for c in sim.operations.computes] == [s, q]
    sim._check_writers()
    sim.operations.remove(q)
    with pytest.raises(_lib.AzpError, match="SolidLiquidRecorder: its SolidLiquid is not in sim.operations.computes"):
        sim._check_writers()
