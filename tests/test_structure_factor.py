"""compute.StructureFactor / compute.StructureFactorRecorder without a GPU: the wavevector set against a plain triple
loop (tests/structure_factor_ref.py), the thinning, the normalisation and the spherical average on hand-made rows,
every refusal, and the C ABI's refusals that return before anything is launched."""

import ctypes as C
import os
import subprocess
import tempfile
import types

import numpy as np
import pytest

import structure_factor_ref as ref

import azplugins_amd as azp
from azplugins_amd import _lib, compute

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CUBE = ((8.0, 8.0, 8.0), (0.0, 0.0, 0.0))
ORTHO = ((7.0, 9.5, 12.0), (0.0, 0.0, 0.0))
TILTED = ((9.0, 10.0, 11.0), (0.3, -0.2, 0.4))
BOXES = {"cube": (CUBE, 2.0 * np.pi * 4.5 / 8.0), "ortho": (ORTHO, 3.1), "tilted": (TILTED, 2.9)}


def _box(box):
    (Lx, Ly, Lz), (xy, xz, yz) = box
    return azp.Box(Lx, Ly, Lz, xy, xz, yz)


# ---------------------------------------------------------------------------
# the vector set
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(BOXES))
def test_enumeration_equals_the_triple_loop(name):
    box, q_max = BOXES[name]
    num_bins = 13
    m, bins = compute.structure_factor_vectors(_box(box), q_max, num_bins)
    m_ref, bins_ref, q_ref = ref.vectors(box, q_max, num_bins)
    assert m.dtype == np.int64 and m.shape == m_ref.shape and len(m) > 100
    assert np.array_equal(m, m_ref) and np.array_equal(bins, bins_ref)
    # the half space: one of each +-pair, never 0
    h, k, l = m.T
    assert np.all((l > 0) | ((l == 0) & (k > 0)) | ((l == 0) & (k == 0) & (h > 0)))
    assert len({tuple(v) for v in m} | {tuple(-v) for v in m}) == 2 * len(m)
    # (l, k, h) lexicographic
    key = [(int(v[2]), int(v[1]), int(v[0])) for v in m]
    assert key == sorted(key)
    # strictly inside q_max, and nothing inside was left out: brute force over a larger block with numpy.linalg
    (Lx, Ly, Lz), (xy, xz, yz) = box
    H = np.array([[Lx, xy * Ly, xz * Lz], [0.0, Ly, yz * Lz], [0.0, 0.0, Lz]])
    B = 2.0 * np.pi * np.linalg.inv(H).T
    q = compute.reciprocal_vectors(_box(box), m)
    assert np.allclose(q, m @ B.T, rtol=1e-13, atol=1e-13)
    assert np.all(np.linalg.norm(q, axis=1) < q_max) and np.allclose(np.linalg.norm(q, axis=1), q_ref, rtol=1e-15)
    r = np.arange(-12, 13)
    block = np.array([(a, b, c) for c in r for b in r for a in r])
    inside = np.linalg.norm(block @ B.T, axis=1) < q_max * (1.0 - 1e-12)
    assert inside.sum() - 1 <= 2 * len(m) <= (np.linalg.norm(block @ B.T, axis=1) < q_max * (1.0 + 1e-12)).sum() - 1


def test_cube_count_and_strict_q_max():
    # |m|^2 < 4.5^2 = 20.25: the lattice points with 0 < |m|^2 <= 20, half of them
    r = np.arange(-5, 6)
    n2 = (r[:, None, None] ** 2 + r[None, :, None] ** 2 + r[None, None, :] ** 2)
    m, _ = compute.structure_factor_vectors(_box(CUBE), 2.0 * np.pi * 4.5 / 8.0, 8)
    assert 2 * len(m) == ((n2 > 0) & (n2 <= 20)).sum()
    # q_max exactly on a shell (|m| = 2: q = pi / 2, (2 pi (2 / 8))^2 is computed exactly as such): strict, so excluded
    q2 = ref.q_of(CUBE, 2, 0, 0)[0]
    m, _ = compute.structure_factor_vectors(_box(CUBE), q2, 4)
    assert (m ** 2).sum(axis=1).max() == 3 and 2 * len(m) == ((n2 > 0) & (n2 <= 3)).sum()
    m, _ = compute.structure_factor_vectors(_box(CUBE), float(np.nextafter(q2, 10.0)), 4)
    assert (m ** 2).sum(axis=1).max() == 4
    # below the smallest |q| = 2 pi / 8: empty
    m, b = compute.structure_factor_vectors(_box(CUBE), 0.78, 4)
    assert m.shape == (0, 3) and b.shape == (0,)


@pytest.mark.parametrize("name", ["cube", "tilted"])
def test_thinning_keeps_the_smallest_keys_per_bin(name):
    box, q_max = BOXES[name]
    num_bins, M = 9, 7
    full, full_bins = compute.structure_factor_vectors(_box(box), q_max, num_bins)
    m, bins = compute.structure_factor_vectors(_box(box), q_max, num_bins, max_vectors_per_bin=M, seed=3)
    m_ref, bins_ref, _ = ref.vectors(box, q_max, num_bins, max_vectors_per_bin=M, seed=3)
    assert np.array_equal(m, m_ref) and np.array_equal(bins, bins_ref)
    available = np.bincount(full_bins, minlength=num_bins)
    assert np.array_equal(np.bincount(bins, minlength=num_bins), np.minimum(available, M))
    assert available.max() > M > available[available > 0].min()  # (both cases of min(M, available) occur)
    # a subset of the full list in its order, reproducible, and another seed picks other vectors
    pos = {tuple(v): i for i, v in enumerate(full)}
    idx = [pos[tuple(v)] for v in m]
    assert idx == sorted(idx)
    again, _ = compute.structure_factor_vectors(_box(box), q_max, num_bins, max_vectors_per_bin=M, seed=3)
    other, _ = compute.structure_factor_vectors(_box(box), q_max, num_bins, max_vectors_per_bin=M, seed=4)
    assert np.array_equal(again, m) and not np.array_equal(other, m)


def test_too_many_vectors_are_refused_with_their_number():
    box = azp.Box(100.0)
    with pytest.raises(_lib.AzpError, match="2\\^24"):
        compute.structure_factor_vectors(box, 2.0 * np.pi * 130.0 / 100.0, 10)   # 261^3 > 2^24 triples
    q_max = 2.0 * np.pi * 32.5 / 100.0
    with pytest.raises(_lib.AzpError) as e:
        compute.structure_factor_vectors(box, q_max, 10)
    r = np.arange(-33, 34)
    n2 = (r[:, None, None] ** 2 + r[None, :, None] ** 2 + r[None, None, :] ** 2)
    n = int(((n2 > 0) & (n2 < 32.5 ** 2)).sum()) // 2
    assert n > _lib.SF_MAX_VECTORS and str(n) in str(e.value) and "65536" in str(e.value)
    m, bins = compute.structure_factor_vectors(box, q_max, 10, max_vectors_per_bin=6000)
    assert len(m) <= 60000 and np.bincount(bins).max() == 6000


# ---------------------------------------------------------------------------
# normalisation and the spherical average
# ---------------------------------------------------------------------------
def _row(rho_a, rho_b, sizes):
    rho_a, rho_b = np.asarray(rho_a, dtype=complex), np.asarray(rho_b, dtype=complex)
    return np.concatenate([rho_a.real, rho_a.imag, rho_b.real, rho_b.imag, np.array(sizes + (0,), dtype=float)])


def test_structure_factor_from_amplitudes_hand_made_rows():
    rho = np.array([3.0 + 4.0j, -2.0j, 0.0])
    s = compute.structure_factor_from_amplitudes(_row(rho, rho, (5, 5, 5)), 3)
    assert np.array_equal(s, np.array([25.0, 4.0, 0.0]) / 5.0) and s.dtype == np.float64
    # disjoint groups: Re[rho_A conj(rho_B)] / sqrt(N_A N_B), which may be negative
    a, b = np.array([1.0 + 2.0j, 3.0]), np.array([2.0 - 1.0j, -1.0 + 5.0j])
    s = compute.structure_factor_from_amplitudes(_row(a, b, (4, 9, 0)), 2)
    assert np.array_equal(s, np.array([0.0, -3.0]) / 6.0)
    # an empty group: zeros
    assert np.array_equal(compute.structure_factor_from_amplitudes(_row(a, [0.0, 0.0], (4, 0, 0)), 2), np.zeros(2))
    assert np.array_equal(compute.structure_factor_from_amplitudes(_row([0.0, 0.0], b, (0, 9, 0)), 2), np.zeros(2))


def test_spherical_average_and_empty_bins():
    mean, count = compute.spherical_average([1.0, 3.0, 10.0, -4.0], [0, 0, 3, 2], 5)
    assert np.array_equal(count, [2, 0, 1, 1, 0]) and count.dtype == np.int64
    assert np.array_equal(mean[[0, 2, 3]], [2.0, -4.0, 10.0]) and np.isnan(mean[1]) and np.isnan(mean[4])


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
def _sf(**kw):
    args = dict(filter_a=azp.All(), filter_b=azp.All(), q_max=3.0, num_bins=20)
    args.update(kw)
    return compute.StructureFactor(**args)


@pytest.mark.parametrize("kw", [dict(q_max=0.0), dict(q_max=-1.0), dict(q_max=float("nan")), dict(q_max=float("inf")),
                                dict(num_bins=0), dict(num_bins=-3), dict(num_bins=2.5), dict(num_bins=_lib.RDF_MAX_BINS + 1),
                                dict(filter_a=None), dict(filter_b="A"), dict(max_vectors_per_bin=0),
                                dict(max_vectors_per_bin=1.5), dict(seed=-1), dict(seed=1 << 64), dict(seed=0.5)])
def test_constructor_refuses(kw):
    with pytest.raises(_lib.AzpError):
        _sf(**kw)


def test_setters_refuse_and_accept():
    s = _sf(filter_a=azp.Type(["A", "B"]), filter_b=azp.Type("B"), max_vectors_per_bin=5, seed=(1 << 64) - 1)
    assert s.filter_a == azp.Type(["B", "A"]) and s.filter_b == azp.Type(["B"]) and s.max_vectors_per_bin == 5
    assert s.path == _lib.SF_PATH_AUTO == 0 and (_lib.SF_PATH_DIRECT, _lib.SF_PATH_POWERS) == (1, 2)
    for name, value in (("q_max", 0.0), ("num_bins", 0), ("path", 3), ("max_vectors_per_bin", -1), ("seed", -5)):
        with pytest.raises(_lib.AzpError):
            setattr(s, name, value)
    s.num_bins, s.q_max, s.path, s.max_vectors_per_bin = 7, 3.5, _lib.SF_PATH_POWERS, None
    assert np.array_equal(s.bin_edges, np.linspace(0.0, 3.5, 8)) and np.allclose(s.bin_centers, (np.arange(7) + 0.5) * 0.5)
    assert s.max_vectors_per_bin is None


PROPERTIES = ("vectors", "q_vectors", "q", "amplitudes", "group_sizes", "vector_structure_factor", "vectors_per_bin",
              "structure_factor")


def test_unattached_reads_raise_data_access_error():
    s = _sf()
    for name in PROPERTIES:
        with pytest.raises(compute.DataAccessError):
            getattr(s, name)
    sim = azp.Simulation(device="cuda:0")
    sim.operations.computes.append(s)  # in the list, but the simulation has no state
    with pytest.raises(compute.DataAccessError):
        s.structure_factor
    assert s.bin_edges.shape == (21,) and s.bin_centers.shape == (20,)  # (these need no state)


def _attached(box, **kw):
    """A compute attached to a stand-in simulation whose state has a box and nothing else: enough for the vector set."""
    s = _sf(**kw)
    state = types.SimpleNamespace(box=box, box_generation=0, device="cpu")
    s._sim = types.SimpleNamespace(state=state, domain=None, operations=types.SimpleNamespace(computes=[s]))
    return s


def test_box_refusals_when_read():
    with pytest.raises(_lib.AzpError, match="periodic"):
        _attached(azp.Box(8.0, 8.0, 8.0, periodic=(True, True, False))).vectors
    with pytest.raises(_lib.AzpError, match="3-D"):
        _attached(azp.Box(8.0, 8.0, 0.0)).vectors
    with pytest.raises(_lib.AzpError, match="smallest"):
        _attached(azp.Box(8.0), q_max=0.78).vectors


def test_vector_properties_and_the_cache():
    box = _box(TILTED)
    s = _attached(box, q_max=2.9, num_bins=13)
    m_ref, bins_ref, q_ref = ref.vectors(TILTED, 2.9, 13)
    assert np.array_equal(s.vectors, m_ref) and s.vectors.dtype == np.int64
    assert np.array_equal(s.q, q_ref) and s.q_vectors.shape == (len(m_ref), 3)
    assert np.array_equal(s.vectors_per_bin, np.bincount(bins_ref, minlength=13)) and s.vectors_per_bin.sum() == len(m_ref)
    first = s._set
    assert s.vectors is not None and s._set is first  # (cached)
    for name, value in (("q_max", 2.5), ("num_bins", 11), ("max_vectors_per_bin", 3), ("seed", 9)):
        before = s._set
        setattr(s, name, value)
        s.vectors
        assert s._set is not before, name
    assert np.array_equal(s.vectors, ref.vectors(TILTED, 2.5, 11, 3, 9)[0])
    # a new box (State.set_box bumps box_generation)
    before = s._set
    s._sim.state.box, s._sim.state.box_generation = azp.Box(9.0, 10.0, 12.0, 0.3, -0.2, 0.4), 1
    assert len(s.vectors) and s._set is not before


# ---------------------------------------------------------------------------
# the recorder's bookkeeping
# ---------------------------------------------------------------------------
def test_recorder_construction_and_empty_tables():
    s = _sf(num_bins=20)
    rec = compute.StructureFactorRecorder(s, 10)
    assert rec.trigger == azp.Periodic(10) and rec._compute is s
    assert rec.timesteps_in_run(0, 30) == [10, 20, 30]
    assert rec.timesteps.shape == (0,) and rec.amplitudes.shape == (0, 2, 0) and rec.structure_factor.shape == (0, 20)
    assert rec.mean_structure_factor.shape == (20,) and np.all(np.isnan(rec.mean_structure_factor))
    rec.reset()
    with pytest.raises(_lib.AzpError):
        compute.StructureFactorRecorder(compute.ThermodynamicQuantities(azp.All()), 10)
    sim = azp.Simulation(device="cuda:0")
    sim.operations.add(s)
    sim.operations.add(rec)
    assert sim.operations.writers == [rec] and [c for c in sim.operations.computes] == [s]
    sim._check_writers()
    sim.operations.remove(s)
    with pytest.raises(_lib.AzpError, match="StructureFactorRecorder: its StructureFactor is not in sim.operations.computes"):
        sim._check_writers()


# ---------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------
def _c_args(L=(8.0, 8.0, 8.0), tilt=(0.0, 0.0, 0.0), periodic=(1, 1, 1), n_vectors=100, path=0, n=1000, m_max=(4, 4, 4), same=1):
    a = _lib.StructureFactorArgs()
    a.N = n
    a.ntypes = 1
    a.box = _lib.make_box(L, tilt, periodic)
    a.same_groups = same
    a.n_vectors = n_vectors
    for d in range(3):
        a.m_max[d] = m_max[d]
    a.path = path
    return a


def test_c_abi_refuses_before_anything_is_launched():
    """azp_structure_factor_scratch_size runs the checks of azp_structure_factor_amplitudes and touches no device."""
    lib = _lib.lib()
    need = C.c_uint64(12345)

    def rc(**kw):
        return lib.azp_structure_factor_scratch_size(C.byref(_c_args(**kw)), C.byref(need))

    # 1000 particles are 4 stages of 256: 4 chunks of one stage; 2 slots x 100 vectors + 3 counts
    assert rc() == 0 and need.value == (2 * 100 + 3) * 4 * 8
    assert ref.shape(1000, 100) == (1, 4)
    assert rc(same=0) == 0 and need.value == (4 * 100 + 3) * 4 * 8
    stages, n_chunks = ref.shape(1 << 20, 65536)
    assert (stages, n_chunks) == (256, 16) and ref.depth(1 << 20, 65536) == 519 and ref.depth(1 << 20, 2048) == 278
    assert rc(n=1 << 20, n_vectors=65536) == 0 and need.value == (2 * 65536 + 3) * 16 * 8
    bad = -1  # AZP_ERROR_INVALID_ARGUMENT
    assert rc(n_vectors=0) == bad and rc(n_vectors=_lib.SF_MAX_VECTORS + 1) == bad and rc(n_vectors=_lib.SF_MAX_VECTORS) == 0
    assert rc(periodic=(1, 1, 0)) == bad and rc(periodic=(0, 1, 1)) == bad
    assert rc(L=(8.0, 0.0, 8.0)) == bad and rc(L=(8.0, 8.0, -1.0)) == bad and rc(L=(float("inf"), 8.0, 8.0)) == bad
    assert rc(path=3) == bad and rc(path=1) == 0 and rc(path=2) == 0
    # the powers path: 32 rows of (Hx + Hy + Hz + 3 | 1) entries of 16 bytes within 48 KiB, i.e. at most 95 entries
    assert _lib.SF_POWERS_LDS_BYTES == 49152
    assert rc(path=2, m_max=(30, 31, 31)) == 0 and rc(path=2, m_max=(31, 31, 31)) == bad
    assert rc(path=0, m_max=(31, 31, 31)) == 0 and rc(path=1, m_max=(200, 200, 200)) == 0
    assert lib.azp_structure_factor_scratch_size(None, C.byref(need)) == bad
    assert lib.azp_structure_factor_scratch_size(C.byref(_c_args()), None) == bad
    # azp_structure_factor_amplitudes itself refuses the same way, before it reads a pointer
    assert lib.azp_structure_factor_amplitudes(C.byref(_c_args(n_vectors=0)), None) == bad
    assert lib.azp_structure_factor_amplitudes(C.byref(_c_args(periodic=(1, 0, 1))), None) == bad
    assert lib.azp_structure_factor_amplitudes(C.byref(_c_args(path=2, m_max=(2, 3, 90))), None) == bad
    assert lib.azp_structure_factor_amplitudes(C.byref(_c_args()), None) == bad  # NULL d_out, d_vectors, d_pos


def test_abi_struct_size_matches_header():
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "azp.h"\nint main(){printf("%zu %zu %zu %d %d\\n", '
           'sizeof(azp_structure_factor_args), offsetof(azp_structure_factor_args, m_max), '
           'offsetof(azp_structure_factor_args, d_out), AZP_SF_MAX_VECTORS, AZP_SF_POWERS_LDS_BYTES);return 0;}')
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "s.c"), "w") as f:
            f.write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        size, off_m, off_out, cap, lds = (int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split())
    A = _lib.StructureFactorArgs
    assert size == C.sizeof(A) and off_m == A.m_max.offset and off_out == A.d_out.offset
    assert cap == _lib.SF_MAX_VECTORS and lds == _lib.SF_POWERS_LDS_BYTES


# ---------------------------------------------------------------------------
# the reference itself
# ---------------------------------------------------------------------------
def test_reference_amplitudes_on_a_lattice_and_the_bound():
    g = np.array([-4.0, -2.0, 0.0, 2.0])
    xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    m, _, _ = ref.vectors(CUBE, 2.0 * np.pi * 4.5 / 8.0, 4)
    re, im = ref.amplitudes(xyz, CUBE, m)
    bragg = np.all(m % 4 == 0, axis=1)
    assert bragg.sum() == 3 and np.array_equal(re[bragg], [64.0] * 3) and np.abs(re[~bragg]).max() < 1e-16 and np.abs(im).max() < 1e-16
    # members only
    re_half, _ = ref.amplitudes(xyz, CUBE, m, member=np.arange(64) < 32)
    assert np.array_equal(re_half[bragg], [32.0] * 3)
    # the bound: the constants within the cap of 16, the orthorhombic c_arg = 2.5 pi
    assert ref.c_arg(CUBE) == pytest.approx(2.5 * np.pi) and ref.c_arg(CUBE) < ref.c_arg(TILTED) <= 16.0 and ref.C_TRIG <= 16.0
    b = ref.bound([[1, -2, 3]], 1000, 263, TILTED)
    assert b.shape == (1,) and b[0] == 1000 * 2.0 ** -52 * (ref.c_arg(TILTED) * 6 + 4.0 + 263)
    assert b[0] <= 1000 * 2.0 ** -52 * (16 * 6 + 16 + 263)
