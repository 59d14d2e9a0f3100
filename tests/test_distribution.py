"""compute.BondedDistribution, host side (no GPU): what the constructor refuses, the reference module
(tests/distribution_ref.py) against a plain Python loop, the guard of the exact GPU comparisons on the systems those
use, and the error returns of azp_bonded_histogram."""

import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import azplugins_amd as azp
import distribution_ref as R
from azplugins_amd import _lib, compute

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("bond", "angle", "dihedral", "pair")


def test_constructor_refuses():
    for kw in (dict(kind="improper", num_bins=8), dict(kind=2, num_bins=8), dict(kind="bonds", num_bins=8, r_min=0.0, r_max=1.0),
               dict(kind="angle", num_bins=0), dict(kind="angle", num_bins=_lib.RDF_MAX_BINS + 1), dict(kind="angle", num_bins=-4),
               dict(kind="angle", num_bins=2.5), dict(kind="dihedral", num_bins=True),
               dict(kind="bond", num_bins=8), dict(kind="bond", num_bins=8, r_min=0.5), dict(kind="pair", num_bins=8, r_max=2.0),
               dict(kind="bond", num_bins=8, r_min=1.0, r_max=1.0), dict(kind="bond", num_bins=8, r_min=2.0, r_max=1.0),
               dict(kind="pair", num_bins=8, r_min=-0.5, r_max=1.0), dict(kind="bond", num_bins=8, r_min=0.0, r_max=math.inf),
               dict(kind="bond", num_bins=8, r_min=math.nan, r_max=1.0),
               dict(kind="angle", num_bins=8, r_min=0.0), dict(kind="angle", num_bins=8, r_max=3.0),
               dict(kind="dihedral", num_bins=8, r_min=0.0, r_max=3.0)):
        with pytest.raises(azp.AzpError):
            compute.BondedDistribution(**kw)
    d = compute.BondedDistribution("bond", _lib.RDF_MAX_BINS, r_min=0.0, r_max=2.0)
    assert d.kind == "bond" and d.num_bins == 8192 and (d.r_min, d.r_max) == (0.0, 2.0)
    with pytest.raises(azp.AzpError):
        d.num_bins = 0
    with pytest.raises(azp.AzpError):
        d.path = 3
    assert compute.BondedDistribution("angle", 1).r_max is None


def test_bins_need_no_state_and_reads_need_one():
    a = compute.BondedDistribution("angle", 64)
    assert a.bin_edges.shape == (65,) and a.bin_edges[0] == 0.0 and a.bin_edges[-1] == math.pi
    assert abs(a.bin_width - math.pi / 64) < 1e-17 and a.bin_centers.shape == (64,)
    d = compute.BondedDistribution("dihedral", 10)
    assert d.bin_edges[0] == -math.pi and d.bin_edges[-1] == math.pi and abs(d.bin_centers[0] + 0.9 * math.pi) < 1e-15
    b = compute.BondedDistribution("bond", 4, r_min=1.0, r_max=2.0)
    assert np.array_equal(b.bin_edges, [1.0, 1.25, 1.5, 1.75, 2.0])
    for name in ("counts", "outside", "num_groups", "distribution", "types"):
        with pytest.raises(compute.DataAccessError):
            getattr(a, name)
    sim = azp.Simulation(device="cuda:0")
    sim.operations.add(a)                       # in the list, but the simulation has no state
    with pytest.raises(compute.DataAccessError):
        a.counts


def test_recorder_before_a_run():
    a = compute.BondedDistribution("angle", 16)
    rec = compute.BondedDistributionRecorder(a, 5)
    assert rec.trigger == azp.Periodic(5) and rec.timesteps_in_run(0, 20) == [5, 10, 15, 20]
    assert rec.timesteps.shape == (0,) and rec.counts.shape[0] == 0 and rec.counts.shape[2] == 16
    rec.reset()
    with pytest.raises(azp.AzpError):
        compute.BondedDistributionRecorder(compute.ThermodynamicQuantities(azp.All()), 5)
    sim = azp.Simulation(device="cuda:0")
    sim.operations.add(rec)
    assert sim.operations.writers == [rec] and rec._compute is a
    with pytest.raises(azp.AzpError, match="BondedDistributionRecorder: its BondedDistribution is not in"):
        sim._check_writers()
    sim.operations.add(a)
    sim._check_writers()


def test_distribution_from_counts():
    counts = np.array([[1, 3, 0, 0], [0, 0, 0, 0], [2, 2, 2, 2]])
    got = compute.distribution_from_counts(counts, [5, 0, 8], 0.25)
    assert np.array_equal(got[0], [0.8, 2.4, 0.0, 0.0]) and not got[1].any() and np.array_equal(got[2], [1.0] * 4)
    assert abs(got[2].sum() * 0.25 - 1.0) < 1e-15 and abs(got[0].sum() * 0.25 - 0.8) < 1e-15   # one of the five lies outside


# ---------------------------------------------------------------------------
# the reference against a plain loop
# ---------------------------------------------------------------------------
def _loop(kind, s, num_bins, r_min=None, r_max=None):
    """Counts by a plain Python loop with its own geometry (cubic box: the minimum image is a rounding per axis)."""
    L = s["L"]
    assert s["tilt"] == (0.0, 0.0, 0.0)

    def sep(i, j):
        return [(s["xyz"][i][c] - s["xyz"][j][c]) - L[c] * round((s["xyz"][i][c] - s["xyz"][j][c]) / L[c]) for c in range(3)]

    def cross(u, v):
        return [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]

    def dot(u, v):
        return u[0] * v[0] + u[1] * v[1] + u[2] * v[2]

    lo, hi = {"angle": (0.0, math.pi), "dihedral": (-math.pi, math.pi)}.get(kind, (r_min, r_max))
    counts = [[0] * num_bins for _ in range(2)]
    outside, total = [0, 0], [0, 0]
    for g, t in zip(s[kind + "s"].tolist(), s[kind + "_typeid"].tolist()):
        if len(g) == 2:
            x = math.sqrt(dot(sep(g[0], g[1]), sep(g[0], g[1])))
        elif len(g) == 3:
            u, v = sep(g[0], g[1]), sep(g[2], g[1])
            x = math.atan2(math.sqrt(dot(cross(u, v), cross(u, v))), dot(u, v))
        else:
            b1, b2, b3 = sep(g[1], g[0]), sep(g[2], g[1]), sep(g[3], g[2])
            x = math.atan2(math.sqrt(dot(b2, b2)) * dot(b1, cross(b2, b3)), dot(cross(b1, b2), cross(b2, b3)))
        total[t] += 1
        if len(g) == 2 and not lo <= x < hi:
            outside[t] += 1
            continue
        k = int((x - lo) * (num_bins / (hi - lo)))
        counts[t][min(k, num_bins - 1)] += 1
    return counts, outside, total


@pytest.mark.parametrize("kind", KINDS)
def test_reference_agrees_with_a_plain_loop(kind):
    s = R.chain_system(n_chains=4, chain_len=8, box="cubic", seed=11)
    assert s["xyz"].shape == (35, 3) and len(s["bonds"]) == 30 and len(s["angles"]) == 25 and len(s["dihedrals"]) == 20
    ref = R.histogram(kind, s["xyz"], s[kind + "s"], s[kind + "_typeid"], 2, 16, s["L"], s["tilt"], **R.ranges(kind))
    counts, outside, total = _loop(kind, s, 16, **R.ranges(kind))
    assert R.guard(ref["index"][ref["inside"]]) > 1e-9
    assert ref["counts"].tolist() == counts and ref["outside"].tolist() == outside and ref["num_groups"].tolist() == total
    assert ref["counts"].sum() + ref["outside"].sum() == len(s[kind + "s"]) and ref["counts"].sum() > 0
    if kind == "bond":
        assert ref["outside"].sum() > 0        # the bond range is narrower than the bond lengths drawn


def test_reference_edges():
    """Lower edges inclusive, r_max exclusive, theta == pi and phi == pi in the last bin, phi == -pi in the first."""
    xyz = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.25, 0.0], [0.0, 0.0, 1.5], [-2.0, 0.0, 0.0]])
    L = (20.0, 20.0, 20.0)
    h = R.histogram("bond", xyz, [(0, 1), (0, 2), (0, 3), (0, 4)], [0, 0, 0, 0], 1, 4, L, r_min=1.0, r_max=2.0)
    assert h["counts"].tolist() == [[1, 1, 1, 0]] and h["outside"].tolist() == [1] and h["num_groups"].tolist() == [4]
    h = R.histogram("angle", xyz, [(1, 0, 4)], [0], 1, 8, L)
    assert h["x"][0] == math.pi and h["counts"].tolist() == [[0] * 7 + [1]]
    trans = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 1.0]])
    h = R.histogram("dihedral", trans, [(0, 1, 2, 3)], [0], 1, 8, L)
    assert h["x"][0] == math.pi and h["counts"].tolist() == [[0] * 7 + [1]]


@pytest.mark.parametrize("box", ["triclinic", "cubic"])
@pytest.mark.parametrize("kind", KINDS)
def test_guard_of_the_gpu_systems(kind, box):
    """The systems of tests/test_gpu_distribution.py: every group's index lies at least 1e-9 from an integer, seven
    orders above the rounding of a device coordinate. No group is left out of the comparison there."""
    s = R.chain_system(box=box)
    assert s["xyz"].shape[0] == 323
    for num_bins in (64, 8192):
        ref = R.chain_reference(kind, num_bins, box=box)
        assert R.guard(ref["index"]) > 1e-9   # (bonds and pairs: also from the ends of the range, index 0 and num_bins)
    ref = R.chain_reference(kind, 64, box=box)
    assert ref["num_groups"].tolist() == [(len(s[kind + "s"]) + 1) // 2, len(s[kind + "s"]) // 2]
    assert (ref["counts"].sum(axis=1) > 0).all() and (ref["counts"] > 0).sum() > 20
    if kind == "bond":
        assert ref["outside"].min() > 0


# ---------------------------------------------------------------------------
# the C entry, without a device
# ---------------------------------------------------------------------------
def _c_args(**kw):
    a = _lib.BondedHistogramArgs()
    a.arity, a.n_types, a.num_bins, a.r_min, a.r_max = 2, 2, 64, 0.5, 1.5
    a.box = _lib.make_box((10.0, 10.0, 10.0))
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_c_entry_refuses_bad_arguments_and_accepts_no_particles():
    fn = _lib.lib().azp_bonded_histogram
    bad = -1  # AZP_ERROR_INVALID_ARGUMENT
    assert fn(None, None) == bad
    assert fn(C.byref(_c_args()), None) == 0                    # N == 0: success before any array is looked at
    for arity in (3, 4):
        assert fn(C.byref(_c_args(arity=arity, r_min=0.0, r_max=0.0)), None) == 0   # (the range is not looked at)
    for kw in (dict(arity=1), dict(arity=5), dict(num_bins=0), dict(num_bins=_lib.RDF_MAX_BINS + 1), dict(n_types=0), dict(path=3),
               dict(r_min=1.5), dict(r_min=-0.1), dict(r_max=math.inf), dict(r_min=math.nan),
               dict(path=1, num_bins=_lib.RDF_MAX_BINS)):      # 2 x 8194 words do not fit: a forced LDS path is refused
        assert fn(C.byref(_c_args(**kw)), None) == bad, kw
    assert fn(C.byref(_c_args(path=1, num_bins=_lib.RDF_MAX_BINS, n_types=1)), None) == 0
    assert fn(C.byref(_c_args(path=2)), None) == 0
    assert fn(C.byref(_c_args(N=8, n_max=8)), None) == bad       # particles, and every array NULL


def test_abi_struct_size_and_threshold_match_the_header():
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "azp.h"\nint main(){printf("%zu %zu %zu %d\\n", '
           'sizeof(azp_bonded_histogram_args), offsetof(azp_bonded_histogram_args, pitch), '
           'offsetof(azp_bonded_histogram_args, d_out), AZP_BONDED_HISTOGRAM_LDS_WORDS);return 0;}')
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "s.c"), "w") as f:
            f.write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        size, pitch, out, words = (int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split())
    A = _lib.BondedHistogramArgs
    assert (size, pitch, out) == (C.sizeof(A), A.pitch.offset, A.d_out.offset)
    assert words == _lib.BONDED_HISTOGRAM_LDS_WORDS == 64 * 1024 // 4
