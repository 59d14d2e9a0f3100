"""compute.MeanSquaredDisplacement / compute.SelfIntermediateScattering without a device: the reference of
tests/displacement_ref.py against closed forms, the lag averaging (``average_over_origins``,
``intermediate_scattering_from_amplitudes``) on hand-made tables, and the argument refusals that need no GPU."""

import ctypes as C

import numpy as np
import pytest

import displacement_ref as ref

import azplugins_amd as azp
from azplugins_amd import _lib, compute

CUBE = ((8.0, 8.0, 8.0), (0.0, 0.0, 0.0))
TILTED = ((9.0, 10.0, 11.0), (0.3, -0.2, 0.4))


def _box(box):
    (Lx, Ly, Lz), (xy, xz, yz) = box
    return azp.Box(Lx, Ly, Lz, xy, xz, yz)


def _wrapped(n, box, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((n, 3)) - 0.5) @ ref.box_ref.box_matrix(*box).T


def _wrap(pos, box):
    out, image = ref.box_ref.wrap(pos, np.zeros(pos.shape, dtype=np.int64), box[0], box[1])
    return out, image


# ---------------------------------------------------------------------------
# the reference against closed forms
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("box", [CUBE, TILTED])
def test_uniform_displacement_closed_forms(box):
    """Every particle moves by the same d: msd = |d|^2, the tensor is d d^T, the drift-removed msd is 0, the
    non-Gaussian parameter of a delta distribution is 3/5 - 1, and F_s(q) = cos(q . d) with Im = -sin(q . d)."""
    pos0 = _wrapped(300, box, 1)
    d = np.array([0.75, -1.5, 2.25])
    pos, image = _wrap(pos0 + d, box)
    assert np.abs(image).sum() > 10  # (some crossed a face)
    got = ref.displacements(pos, image, pos0, np.zeros_like(image), box)
    assert np.abs(np.asarray(got, dtype=np.float64) - d).max() < 1e-14
    p = compute.displacement_moments(ref.moments(got))
    assert p["num_particles"] == 300 and abs(p["msd"] - d @ d) < 1e-12 and np.abs(p["msd_tensor"] - np.outer(d, d)).max() < 1e-12
    assert np.abs(p["mean_displacement"] - d).max() < 1e-13 and abs(p["msd_drift_removed"]) < 1e-11
    assert abs(p["non_gaussian"] + 0.4) < 1e-12 and abs(p["fourth_moment"] - (d @ d) ** 2) < 1e-10
    assert np.allclose(p["msd_components"], d * d, rtol=0, atol=1e-12)
    m, _ = compute.structure_factor_vectors(_box(box), 2.5, 5)
    q = compute.reciprocal_vectors(_box(box), m)
    re, im = ref.self_amplitudes(pos, pos0, box, m)
    assert len(m) > 50 and np.abs(re / 300 - np.cos(q @ d)).max() < 1e-12 and np.abs(im / 300 + np.sin(q @ d)).max() < 1e-12
    f_s, f_i = compute.self_scattering_from_row(np.concatenate([re, im, [300.0, 0.0]]), len(m))
    # (x * (1 / N) against x / N: the rounded reciprocal and one product, 3 u)
    assert np.allclose(f_s, re / 300, rtol=3 * ref.U, atol=0) and np.allclose(f_i, im / 300, rtol=3 * ref.U, atol=0)


def test_whole_lattice_vectors_leave_the_scattering_at_one():
    """A displacement by a lattice vector is a change of the image only: F_s = 1 exactly on every vector, while the
    mean squared displacement sees it."""
    pos0 = _wrapped(100, TILTED, 2)
    rng = np.random.default_rng(3)
    image = rng.integers(-3, 4, (100, 3))
    d = ref.displacements(pos0, image, pos0, np.zeros_like(image), TILTED)
    h = ref.box_ref.box_matrix(*TILTED)
    assert np.abs(np.asarray(d, dtype=np.float64) - image @ h.T).max() < 1e-13
    m, _ = compute.structure_factor_vectors(_box(TILTED), 2.0, 4)
    re, im = ref.self_amplitudes(pos0, pos0, TILTED, m)
    assert np.array_equal(re, np.full(len(m), 100.0)) and np.array_equal(im, np.zeros(len(m)))
    assert compute.displacement_moments(ref.moments(d))["msd"] > 100.0


def test_no_cancellation_after_many_crossings():
    """An image of 10^6 at both times: subtracted as integers, nothing is lost."""
    pos0 = np.array([[1.0, 2.0, 3.0]])
    pos = pos0 + 2.0 ** -30
    image = np.full((1, 3), 10 ** 6)
    for d in (ref.displacements(pos, image, pos0, image, CUBE), ref.displacements_f64(pos, image, pos0, image, CUBE)):
        assert np.array_equal(np.asarray(d, dtype=np.float64), np.full((1, 3), 2.0 ** -30))


def test_reference_orders_bounds_and_histogram():
    rng = np.random.default_rng(45)
    pos0, image0 = _wrapped(500, TILTED, 4), rng.integers(-3, 4, (500, 3))
    pos, image = _wrapped(500, TILTED, 5), rng.integers(-3, 4, (500, 3))
    member = np.arange(500) % 3 == 0
    d = ref.displacements(pos, image, pos0, image0, TILTED)
    d64 = ref.displacements_f64(pos, image, pos0, image0, TILTED)
    A = ref.magnitudes(pos, image, pos0, image0, TILTED)
    assert np.all(np.abs(np.asarray(d, dtype=np.float64)) <= A * (1 + 1e-15))
    assert np.all(np.abs(d64 - np.asarray(d, dtype=np.float64)) <= ref.displacement_bound(A))
    for mem in (None, member):
        exact, tree, b = ref.moments(d, mem), ref.tree_moments(d64, mem), ref.moments_bound(A, mem)
        assert exact[0] == tree[0] == (500 if mem is None else member.sum()) and exact[11] == tree[11] == b[11] == 0.0
        assert np.all(np.abs(exact - tree) <= b) and np.all(b[1:11] < 1e-9 * np.abs(ref.terms(np.asarray(d, dtype=np.float64), mem)).sum(axis=1)[1:])
    assert ref.depth(1) == 1 + 6 + 3 + 1 + 6 and ref.depth(16385) == 1 + 6 + 3 + 2 + 6 and ref.depth(524289) == 2 + 6 + 3 + 17 + 6
    counts, outside = ref.histogram(d, 50, 50.0, member)
    assert counts.sum() + outside == member.sum() and outside > 0 and counts.max() > 3
    with pytest.raises(AssertionError):
        ref.histogram(np.array([[3.0, 4.0, 0.0]]), 10, 10.0)  # |d| = 5 sits on an edge
    assert ref.histogram(np.array([[3.0, 4.0, 0.0], [0.0, 0.0, 0.0]]), 10, 10.0, exact=True)[0][5] == 1
    vh = compute.van_hove_from_counts(counts, member.sum(), 50.0)
    shell = 4.0 * np.pi / 3.0 * np.diff(np.linspace(0.0, 50.0, 51) ** 3)
    assert abs((vh * shell).sum() - (1.0 - outside / member.sum())) < 1e-12
    assert np.array_equal(compute.van_hove_from_counts(np.zeros(5, dtype=np.int64), 0, 1.0), np.zeros(5))
    assert ref.fs_c_arg(CUBE) == np.pi * 6.0 and ref.fs_c_arg(TILTED) <= 32.0


def test_moments_of_an_empty_group_are_zeros():
    p = compute.displacement_moments(np.zeros(12))
    assert p["num_particles"] == 0 and p["msd"] == 0.0 and np.array_equal(p["msd_tensor"], np.zeros((3, 3))) and np.isnan(p["non_gaussian"])
    assert np.array_equal(compute.self_scattering_from_row(np.zeros(8), 3)[0], np.zeros(3))


# ---------------------------------------------------------------------------
# lag averaging
# ---------------------------------------------------------------------------
def test_average_over_origins_ring_overwrite_unfilled_slots_and_unequal_groups():
    """Rows at 10, 20, ..., 60 with a ring of two slots and a new origin at every second firing: the origins are 10 (slot 0),
    30 (slot 1), 50 (slot 0 again, overwriting 10). The sums of equal lag are added BEFORE normalising: with N_g of 1 and 3
    behind the two pairs of lag 10 the mean is (s1 + s2) / 4, not the mean of the two ratios."""
    steps = [10, 20, 30, 40, 50, 60]
    origin_steps = [[10, -1], [10, -1], [10, 30], [10, 30], [50, 30], [50, 30]]
    rows = np.zeros((6, 2, 2))  # (N_g, S)
    rows[:, :, 0] = [[1, 0], [1, 0], [1, 3], [1, 3], [2, 3], [2, 3]]
    rows[:, :, 1] = [[0.0, 99.0], [5.0, 99.0], [7.0, 0.0], [11.0, 9.0], [0.0, 13.0], [4.0, 17.0]]
    lags, samples, sums = compute.average_over_origins(steps, origin_steps, rows)
    assert list(lags) == [0, 10, 20, 30] and list(samples) == [3, 3, 2, 2]
    assert np.array_equal(sums[:, 0], [1 + 3 + 2, 1 + 3 + 2, 1 + 3, 1 + 3])
    assert np.array_equal(sums[:, 1], [0.0, 5.0 + 9.0 + 4.0, 7.0 + 13.0, 11.0 + 17.0])  # (the 99s of unfilled slots never count)
    assert sums[1, 1] / sums[1, 0] == 3.0 and np.mean([5.0 / 1, 9.0 / 3, 4.0 / 2]) != 3.0
    ints = compute.average_over_origins(steps, origin_steps, rows.astype(np.int64))[2]
    assert ints.dtype == np.int64 and np.array_equal(ints, sums.astype(np.int64))
    none = compute.average_over_origins([], np.zeros((0, 2)), np.zeros((0, 2, 2)))
    assert none[0].shape == (0,) and none[2].shape == (0, 2)


def test_intermediate_scattering_from_amplitudes():
    """Two vectors, three frames at 0, 5, 10: F(m, 0) is the mean static S, F(m, 5) averages the two pairs of lag 5."""
    rng = np.random.default_rng(6)
    amp = rng.normal(size=(3, 2, 2)) + 1j * rng.normal(size=(3, 2, 2))
    sizes = np.array([[4.0, 9.0], [4.0, 9.0], [5.0, 9.0]])
    lags, F = compute.intermediate_scattering_from_amplitudes(amp, [0, 5, 10], sizes)
    assert list(lags) == [0, 5, 10] and F.shape == (3, 2)

    def pair(r, s):
        return (amp[r, 0] * np.conj(amp[s, 1])).real, np.sqrt(sizes[r, 0] * sizes[s, 1])

    for lag, pairs in ((0, [(0, 0), (1, 1), (2, 2)]), (5, [(1, 0), (2, 1)]), (10, [(2, 0)])):
        num = sum(pair(r, s)[0] for r, s in pairs)
        den = sum(pair(r, s)[1] for r, s in pairs)
        assert np.allclose(F[list(lags).index(lag)], num / den, rtol=1e-15, atol=0)
    static = np.mean([compute.structure_factor_from_amplitudes(np.concatenate([a[0].real, a[0].imag, a[1].real, a[1].imag, [4.0, 9.0, 0.0, 0.0]]), 2)
                      for a in amp[:2]], axis=0)
    assert np.allclose(compute.intermediate_scattering_from_amplitudes(amp[:2], [0, 5], (4.0, 9.0))[1][0], static, rtol=1e-14)
    unnormalised = compute.intermediate_scattering_from_amplitudes(amp, [0, 5, 10])[1]
    assert np.allclose(unnormalised[2], pair(2, 0)[0])
    with pytest.raises(_lib.AzpError):
        compute.intermediate_scattering_from_amplitudes(amp, [0, 5])
    assert hasattr(compute.StructureFactorRecorder, "intermediate_scattering")


# ---------------------------------------------------------------------------
# refusals that need no device
# ---------------------------------------------------------------------------
def test_construction_refusals():
    E = _lib.AzpError
    for bad in (dict(filter="A"), dict(num_bins=-1), dict(num_bins=8193), dict(num_bins=1.5), dict(num_bins=10), dict(num_bins=10, r_max=0.0),
                dict(num_bins=10, r_max=float("inf"))):
        with pytest.raises(E):
            compute.MeanSquaredDisplacement(**bad)
    msd = compute.MeanSquaredDisplacement()
    assert isinstance(msd.filter, azp.All) and msd.num_bins == 0 and msd.r_max is None and msd.origin_timestep is None
    vh = compute.MeanSquaredDisplacement(azp.Type(["A"]), num_bins=4, r_max=2.0)
    assert np.array_equal(vh.bin_edges, [0.0, 0.5, 1.0, 1.5, 2.0]) and np.array_equal(vh.bin_centers, [0.25, 0.75, 1.25, 1.75])
    for args in ((None, 1.0, 4), (azp.All(), 0.0, 4), (azp.All(), 1.0, 0), (azp.All(), 1.0, 4, 0), (azp.All(), 1.0, 4, None, -1)):
        with pytest.raises(E, match="SelfIntermediateScattering"):
            compute.SelfIntermediateScattering(*args)
    fs = compute.SelfIntermediateScattering(azp.All(), 2.0, 8, max_vectors_per_bin=5, seed=3)
    assert (fs.q_max, fs.num_bins, fs.max_vectors_per_bin, fs.seed) == (2.0, 8, 5, 3) and len(fs.bin_edges) == 9
    for rec, c in ((compute.MeanSquaredDisplacementRecorder, msd), (compute.SelfIntermediateScatteringRecorder, fs)):
        for kw in (dict(origins=0), dict(origins=65), dict(origins=1.5), dict(origin_every=0), dict(origin_every=2.5)):
            with pytest.raises(E):
                rec(c, 10, **kw)
        with pytest.raises(E):
            rec(object(), 10)
        r = rec(c, 10, origins=4, origin_every=2)
        assert r.origins == 4 and r.origin_every == 2 and r.timesteps.shape == (0,) and r.lags.shape == (0,)
        assert r.origin_timesteps.shape == (0, 4) and r.samples_per_lag.shape == (0,)
    with pytest.raises(compute.DataAccessError):
        msd.msd
    with pytest.raises(compute.DataAccessError):
        fs.scattering
    with pytest.raises(compute.DataAccessError):
        msd.set_origin()


def _args(**kw):
    a = _lib.DisplacementArgs()
    a.N, a.ntypes, a.box, a.n_origins, a.active_mask = 1000, 1, _lib.make_box(8.0), 1, 1
    a.num_bins, a.r_max, a.n_vectors = 10, 4.0, 7
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_library_refusals_before_any_launch():
    """AZP_ERROR_INVALID_ARGUMENT (-1) from the argument checks: nothing is launched, no device is touched."""
    lib = _lib.lib()
    need = C.c_uint64(0)
    assert lib.azp_displacement_moments_scratch_size(C.byref(_args()), C.byref(need)) == 0 and need.value == 12 * 4 * 8
    assert lib.azp_displacement_moments_scratch_size(C.byref(_args(n_origins=3, N=16385)), C.byref(need)) == 0 and need.value == 3 * 12 * 65 * 8
    assert lib.azp_self_scattering_scratch_size(C.byref(_args()), C.byref(need)) == 0 and need.value == (2 * 7 + 2) * 4 * 8
    for size in (lib.azp_displacement_moments_scratch_size, lib.azp_self_scattering_scratch_size):
        assert size(None, C.byref(need)) == -1 and size(C.byref(_args()), None) == -1
        for kw in (dict(n_origins=0), dict(n_origins=65), dict(box=_lib.make_box((8.0, 8.0, 0.0))), dict(d_type_mask=8, ntypes=0)):
            assert size(C.byref(_args(**kw)), C.byref(need)) == -1, kw
    for kw in (dict(num_bins=_lib.RDF_MAX_BINS + 1), dict(r_max=0.0), dict(r_max=-1.0), dict(r_max=float("nan"))):
        assert lib.azp_displacement_moments_scratch_size(C.byref(_args(**kw)), C.byref(need)) == -1, kw
        assert lib.azp_displacement_moments(C.byref(_args(**kw)), None) == -1, kw
    assert lib.azp_displacement_moments_scratch_size(C.byref(_args(num_bins=0, r_max=0.0)), C.byref(need)) == 0
    for kw in (dict(n_vectors=0), dict(n_vectors=_lib.SF_MAX_VECTORS + 1), dict(box=_lib.make_box(8.0, periodic=(1, 1, 0)))):
        assert lib.azp_self_scattering_scratch_size(C.byref(_args(**kw)), C.byref(need)) == -1, kw
        assert lib.azp_self_scattering(C.byref(_args(**kw)), None) == -1, kw
    # null arrays and too small a scratch (the pointers are never followed: the checks come first)
    full = dict(d_pos=64, d_image=64, d_tag=64, d_rtag=64, d_origin_pos=64, d_origin_image=64, d_out=64, d_vectors=64, d_scratch=64)
    for missing in ("d_pos", "d_image", "d_tag", "d_rtag", "d_origin_pos", "d_origin_image", "d_out", "d_scratch"):
        kw = dict(full, scratch_bytes=1 << 20)
        kw[missing] = None
        assert lib.azp_displacement_moments(C.byref(_args(**kw)), None) == -1, missing
    for missing in ("d_pos", "d_tag", "d_rtag", "d_origin_pos", "d_out", "d_vectors", "d_scratch"):
        kw = dict(full, scratch_bytes=1 << 20)
        kw[missing] = None
        assert lib.azp_self_scattering(C.byref(_args(**kw)), None) == -1, missing
    assert lib.azp_displacement_moments(C.byref(_args(scratch_bytes=12 * 4 * 8 - 1, **full)), None) == -1
    assert lib.azp_self_scattering(C.byref(_args(scratch_bytes=(2 * 7 + 2) * 4 * 8 - 1, **full)), None) == -1
    o = _lib.DisplacementOriginArgs()
    assert lib.azp_displacement_origin(None, None) == -1
    o.N, o.n_slots, o.slot, o.build_rtag = 10, 2, 2, 1
    assert lib.azp_displacement_origin(C.byref(o), None) == -1  # slot >= n_slots
    o.slot, o.build_rtag = 0, 0
    assert lib.azp_displacement_origin(C.byref(o), None) == -1  # nothing to do
    o.build_rtag, o.d_tag = 1, 64
    assert lib.azp_displacement_origin(C.byref(o), None) == -1  # no table to write
    o.d_rtag, o.d_origin_pos = 64, 64
    assert lib.azp_displacement_origin(C.byref(o), None) == -1  # an origin without images
