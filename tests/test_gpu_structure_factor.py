"""compute.StructureFactor and compute.StructureFactorRecorder on the GPU: both kernels against the extended-precision
reference within its derived bound (tests/structure_factor_ref.py), exactly on a dyadic lattice, and a recorder that
leaves the run bit-identical.

Sizes: the kernel stages 256 particles at a time and, up to 131,072 particles, a chunk is ONE stage, so 257 is a chunk
plus one particle and 515 two chunks plus three. The chunks of two stages, the stage loop that ends early and a fold
over more than 64 partials are reached at 131,073 particles only; that case runs with 65 vectors."""

import ctypes as C

import numpy as np
import pytest

import structure_factor_ref as ref

import azplugins_amd as azp
from azplugins_amd import _lib, compute
from azplugins_amd import synthetic as syn

pytestmark = pytest.mark.gpu

DIRECT, POWERS = _lib.SF_PATH_DIRECT, _lib.SF_PATH_POWERS
TYPE_NAMES = ("A", "B", "C", "D")  # (no particle is of type D)
CUBE = ((8.0, 8.0, 8.0), (0.0, 0.0, 0.0))
TILTED = ((9.0, 10.0, 11.0), (0.3, -0.2, 0.4))
Q_CUBE = 2.0 * np.pi * 4.5 / 8.0  # 194 vectors
GROUPS = {"all_all": (None, None), "a_a": (("A",), ("A",)), "a_b": (("A",), ("B",)), "a_ab": (("A",), ("A", "B")),
          "empty": (("D",), None)}


def _filter(names):
    return azp.All() if names is None else azp.Type(list(names))


def _member(names, types):
    return None if names is None else np.isin(types, [TYPE_NAMES.index(t) for t in names])


def _box(box):
    (Lx, Ly, Lz), (xy, xz, yz) = box
    return azp.Box(Lx, Ly, Lz, xy, xz, yz)


def _random(n, box, seed):
    """n uniform random wrapped positions (fractional coordinates in [-0.5, 0.5)) and types 0, 1, 2."""
    (Lx, Ly, Lz), (xy, xz, yz) = box
    rng = np.random.default_rng(seed)
    f = rng.random((n, 3)) - 0.5
    z = f[:, 2] * Lz
    y = f[:, 1] * Ly + yz * z
    x = f[:, 0] * Lx + xy * f[:, 1] * Ly + xz * z
    return np.ascontiguousarray(np.stack([x, y, z], axis=1)), rng.integers(0, 3, n)


def _sim(xyz, box, types=None):
    snap = azp.Snapshot.from_arrays(xyz, _box(box), typeid=np.zeros(len(xyz), dtype=np.int64) if types is None else types, types=TYPE_NAMES)
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(snap)
    return sim


def _compute(sim, group, q_max, num_bins=10, path=0, **kw):
    sf = compute.StructureFactor(_filter(group[0]), _filter(group[1]), q_max, num_bins, **kw)
    sf.path = path
    sim.operations.computes.append(sf)
    return sf


def _check(xyz, types, box, q_max, groups, **kw):
    """Every group pair on both forced paths: Re and Im of both amplitudes of every vector within the bound of the
    reference, the two paths within twice the bound of each other, the group sizes exact. Returns the number of vectors."""
    sim = _sim(xyz, box, types)
    n_vectors = 0
    for name in groups:
        ga, gb = GROUPS[name]
        rows = {}
        for path in (DIRECT, POWERS):
            sf = _compute(sim, (ga, gb), q_max, path=path, **kw)
            rows[path] = sf._read("row")
            m = sf.vectors
        n = n_vectors = len(m)
        D = ref.depth(len(xyz), n)
        sizes = []
        for slot, g in enumerate((ga, gb)):
            member = _member(g, types)
            n_g = len(xyz) if member is None else int(member.sum())
            sizes.append(n_g)
            re, im = ref.amplitudes(xyz, box, m, member)
            b = ref.bound(m, n_g, D, box)
            assert b.max() <= n_g * 2.0 ** -52 * (16 * np.abs(m).sum(axis=1).max() + 16 + D)
            for path, row in rows.items():
                got_re, got_im = row[2 * slot * n:(2 * slot + 1) * n], row[(2 * slot + 1) * n:(2 * slot + 2) * n]
                err = np.maximum(np.abs(got_re - re), np.abs(got_im - im))
                print("%s N=%d n=%d path=%d slot=%d: worst error %.3g, %.3g of the bound" % (name, len(xyz), n, path, slot, err.max(),
                                                                                         (err / np.maximum(b, 1e-300)).max()))
                assert np.all(err <= b), (name, path, slot, int(np.argmax(err - b)), err.max(), b.min())
            assert np.all(np.abs(rows[DIRECT][2 * slot * n:(2 * slot + 2) * n] - rows[POWERS][2 * slot * n:(2 * slot + 2) * n])
                          <= 2.0 * np.tile(b, 2)), name
        both = _member(ga, types), _member(gb, types)
        n_ab = int(np.logical_and(*[np.ones(len(xyz), dtype=bool) if x is None else x for x in both]).sum())
        for row in rows.values():
            assert tuple(row[4 * n:]) == (sizes[0], sizes[1], n_ab, 0.0), name
    return n_vectors


# ---------------------------------------------------------------------------
# exact
# ---------------------------------------------------------------------------
def test_exact_lattice_on_both_paths():
    """4 x 4 x 4 simple cubic lattice of spacing 2 in a cube of 8: every fractional coordinate is a multiple of 1/4,
    every base phasor exactly +-1 or +-i, every product and sum exact: S(m) is 64 where h, k, l are all multiples of 4
    and 0 elsewhere, to the bit, on both paths."""
    g = np.array([-4.0, -2.0, 0.0, 2.0])
    xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    sim = _sim(xyz, CUBE)
    for path in (DIRECT, POWERS, 0):
        sf = _compute(sim, (None, None), 2.0 * np.pi * 8.5 / 8.0, num_bins=17, path=path)
        m = sf.vectors
        assert 1200 < len(m) < 1400 and np.abs(m).max() == 8
        s = sf.vector_structure_factor
        bragg = np.all(m % 4 == 0, axis=1)
        assert bragg.sum() == 16 and np.array_equal(s[bragg], np.full(16, 64.0)) and np.array_equal(s[~bragg], np.zeros((~bragg).sum()))
        row = sf._read("row")
        assert tuple(row[-4:]) == (64.0, 64.0, 64.0, 0.0) and sf.group_sizes == (64, 64, 64)
        assert np.array_equal(row[:2 * len(m)], row[2 * len(m):4 * len(m)])  # (one group: the B half is the copy)
        amp = sf.amplitudes
        assert amp.shape == (2, len(m)) and amp.dtype == np.complex128 and np.array_equal(amp[0][bragg], np.full(16, 64.0 + 0.0j))
        # the spherical average: bin k holds the shell |m| in [k / 2, (k + 1) / 2) of this cube
        mean, count = compute.spherical_average(s, np.minimum((sf.q * 17 / sf.q_max).astype(int), 16), 17)
        assert np.array_equal(sf.vectors_per_bin, count) and count[0] == count[1] == 0 and count.sum() == len(m)
        sfac = sf.structure_factor
        assert np.isnan(sfac[0]) and np.isnan(sfac[1]) and np.array_equal(sfac[2:], mean[2:])
        bins = np.minimum((sf.q * 17 / sf.q_max).astype(int), 16)
        k4 = bins[np.flatnonzero(np.all(m == (4, 0, 0), axis=1))[0]]  # (|m| = 4: the three axis vectors share a bin)
        assert (bragg & (bins == k4)).sum() == 3 and sfac[k4] == 64.0 * 3 / count[k4] and sfac[k4 + 1] == 0.0


# ---------------------------------------------------------------------------
# random systems against the reference
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 257, 515])
def test_chunk_and_stage_edges(n):
    xyz, types = _random(n, CUBE, 100 + n)
    groups = GROUPS if n in (257, 515) else ("all_all", "a_b")
    assert _check(xyz, types, CUBE, Q_CUBE, groups) == 194
    assert ref.shape(n, 194) == (1, -(-n // 256))


def test_chunks_of_two_stages_and_a_fold_over_many_partials():
    n = 512 * 256 + 1
    assert ref.shape(n, 65) == (2, 257) and ref.depth(n, 65) == 256 + 2 + 5 + 6
    xyz, types = _random(n, TILTED, 7)
    assert _check(xyz, types, TILTED, 2.0, ("a_ab",)) == 65


@pytest.mark.parametrize("q_max,n_vectors", [(0.6, 1), (2.0, 65)])
def test_vector_counts_off_the_wave_in_a_tilted_box(q_max, n_vectors):
    xyz, types = _random(600, TILTED, 31)
    assert _check(xyz, types, TILTED, q_max, GROUPS) == n_vectors


def test_thinned_vector_list():
    xyz, types = _random(400, TILTED, 32)
    assert _check(xyz, types, TILTED, 2.9, ("all_all", "a_ab"), num_bins=13, max_vectors_per_bin=5, seed=1) == 51


def test_sum_rule_over_a_partition():
    xyz, types = _random(1000, TILTED, 33)
    types = types % 2  # A and B partition the system
    sim = _sim(xyz, TILTED, types)
    for path in (DIRECT, POWERS):
        parts = _compute(sim, (("A",), ("B",)), 2.9, path=path).amplitudes
        whole = _compute(sim, (None, None), 2.9, path=path)
        rho = whole.amplitudes[0]
        b = ref.bound(whole.vectors, len(xyz), ref.depth(len(xyz), len(rho)), TILTED)
        d = rho - parts[0] - parts[1]
        assert np.all(np.abs(d.real) <= b) and np.all(np.abs(d.imag) <= b) and np.abs(rho).max() > 10.0


def test_ghost_rows_are_not_counted():
    xyz, types = _random(700, CUBE, 34)
    n_local = 443
    snap = azp.Snapshot.from_arrays(xyz, _box(CUBE), typeid=types, types=TYPE_NAMES)
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.state = azp.State(snap, "cuda:0", n_local=n_local)
    assert sim.state.N == n_local and sim.state.n_max == 700
    for path in (DIRECT, POWERS):
        sf = _compute(sim, (("A",), None), Q_CUBE, path=path)
        row = sf._read("row")
        m = sf.vectors
        n = len(m)
        own = types[:n_local]
        re, im = ref.amplitudes(xyz[:n_local], CUBE, m)
        b = ref.bound(m, n_local, ref.depth(n_local, n), CUBE)
        assert np.all(np.abs(row[2 * n:3 * n] - re) <= b) and np.all(np.abs(row[3 * n:4 * n] - im) <= b)
        assert tuple(row[4 * n:]) == (int((own == 0).sum()), n_local, int((own == 0).sum()), 0.0)
        re_all, _ = ref.amplitudes(xyz, CUBE, m)
        assert np.abs(re_all - re).max() > 1.0  # (the ghosts would have shown)


# ---------------------------------------------------------------------------
# determinism, overwriting, refusals
# ---------------------------------------------------------------------------
def test_two_reads_agree_and_garbage_is_overwritten():
    import torch

    xyz, types = _random(515, TILTED, 35)
    sim = _sim(xyz, TILTED, types)
    for path in (DIRECT, POWERS):
        sf = _compute(sim, (("A",), ("B", "C")), 2.9, path=path)
        first, second = sf._read("row"), sf._read("row")
        assert np.array_equal(first.view(np.int64), second.view(np.int64))
        out = torch.full((1, len(first)), float("nan"), dtype=torch.float64, device=sim.state.device)
        sf._launch(out.data_ptr())
        assert np.array_equal(out.cpu().numpy()[0].view(np.int64), first.view(np.int64))
    # N == 0 zeroes the row (through the library: no scratch, no positions)
    st = sim.state
    triples = torch.tensor([[1, 0, 0], [0, 1, 1]], dtype=torch.int32, device=st.device)
    out = torch.full((12,), float("nan"), dtype=torch.float64, device=st.device)
    a = _lib.StructureFactorArgs()
    a.N, a.ntypes, a.box, a.n_vectors, a.d_vectors, a.d_out, a.path = 0, 4, st.box.to_c(), 2, triples.data_ptr(), out.data_ptr(), DIRECT
    assert _lib.lib().azp_structure_factor_amplitudes(C.byref(a), _lib.raw_stream(st.device)) == 0
    assert np.array_equal(out.cpu().numpy(), np.zeros(12))
    assert np.array_equal(compute.structure_factor_from_amplitudes(out.cpu().numpy(), 2), np.zeros(2))


def test_refusals_write_nothing():
    import torch

    long_box = ((8.0, 8.0, 79.0), (0.0, 0.0, 0.0))
    xyz, types = _random(300, long_box, 36)
    sim = _sim(xyz, long_box, types)
    # the powers path beyond its LDS budget: |h|, |k| <= 8 and |l| <= 83 are 102 table entries, 95 fit
    sf = _compute(sim, (None, None), 2.0 * np.pi * 8.5 / 8.0, path=POWERS)
    assert tuple(np.abs(sf.vectors).max(axis=0)) == (8, 8, 83) and len(sf.vectors) < 15000
    out = torch.full((1, sf._row_width()), 7.0, dtype=torch.float64, device="cuda:0")
    with pytest.raises(_lib.AzpError):
        sf._launch(out.data_ptr())
    with pytest.raises(_lib.AzpError):
        sf.structure_factor
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    sf.path = 0  # (automatic: the direct path takes it)
    direct = _compute(sim, (None, None), 2.0 * np.pi * 8.5 / 8.0, path=DIRECT)
    assert np.array_equal(sf._read("row").view(np.int64), direct._read("row").view(np.int64))
    # a box that is not periodic on every axis: by the compute and by the library
    slab = azp.Simulation(device="cuda:0", seed=1)
    slab.create_state_from_snapshot(azp.Snapshot.from_arrays(xyz, azp.Box(8.0, 8.0, 79.0, periodic=(True, True, False)), types=TYPE_NAMES))
    with pytest.raises(_lib.AzpError, match="periodic"):
        _compute(slab, (None, None), Q_CUBE).structure_factor
    st = slab.state
    triples = torch.tensor([[1, 0, 0]], dtype=torch.int32, device=st.device)
    out = torch.full((8,), 7.0, dtype=torch.float64, device=st.device)
    scratch = torch.zeros(1 << 16, dtype=torch.uint8, device=st.device)
    a = _lib.StructureFactorArgs()
    a.d_pos, a.N, a.ntypes, a.box, a.same_groups, a.n_vectors = st.pos.data_ptr(), st.N, 4, st.box.to_c(), 1, 1
    a.d_vectors, a.d_out, a.d_scratch, a.scratch_bytes = triples.data_ptr(), out.data_ptr(), scratch.data_ptr(), scratch.numel()
    a.m_max[0], a.path = 1, DIRECT
    assert _lib.lib().azp_structure_factor_amplitudes(C.byref(a), _lib.raw_stream(st.device)) == -1
    a.scratch_bytes, a.box = 8, sim.state.box.to_c()
    assert _lib.lib().azp_structure_factor_amplitudes(C.byref(a), _lib.raw_stream(st.device)) == -1  # too little scratch
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---------------------------------------------------------------------------
# the recorder
# ---------------------------------------------------------------------------
def _liquid(recorder_period=None):
    cfg = syn.config_plj_sc(12)  # 1728 particles
    n = cfg["xyz"].shape[0]
    tag = np.arange(n, dtype=np.uint64)
    v = np.stack([syn.normal(77, tag, c) for c in range(3)], axis=1)
    snap = azp.Snapshot.from_arrays(cfg["xyz"], cfg["L"], types=("A",), velocity=v - v.mean(axis=0))
    sim = azp.Simulation(device="cuda:0", seed=5)
    sim.create_state_from_snapshot(snap)
    plj = azp.pair.PerturbedLennardJones(nlist=azp.nlist.Cell(buffer=cfg["r_buff"]), default_r_cut=cfg["r_cut"], mode="shift")
    plj.params[("A", "A")] = cfg["params"]
    sim.operations.integrator = azp.Integrator(dt=0.004, forces=[plj], methods=[azp.ConstantVolume()])
    sf = compute.StructureFactor(azp.All(), azp.All(), 2.0 * np.pi * 4.5 / float(cfg["L"][0]), 9)
    sim.operations.add(sf)
    rec = None
    if recorder_period is not None:
        rec = compute.StructureFactorRecorder(sf, recorder_period)
        sim.operations.add(rec)
    return sim, sf, rec


def _bits(t):
    import torch

    return t.clone().view(torch.int64).cpu().numpy()


def test_recorder_rows_equal_the_compute_and_the_run_is_unchanged():
    sim, sf, rec = _liquid(recorder_period=10)
    sim.run(20)
    assert list(rec.timesteps) == [10, 20]
    amp, s = rec.amplitudes, rec.structure_factor
    n = len(sf.vectors)
    assert amp.shape == (2, 2, n) and amp.dtype == np.complex128 and s.shape == (2, 9)
    plain = None
    per_vector = []
    for k, stop in enumerate((10, 20)):
        plain, sf2, _ = _liquid()  # a second, identical run without a recorder that stops there
        plain.run(stop)
        assert np.array_equal(sf2.amplitudes.view(np.float64).view(np.int64), amp[k].view(np.float64).view(np.int64)), stop
        assert np.array_equal(sf2.structure_factor, s[k], equal_nan=True)
        per_vector.append(sf2.vector_structure_factor)
    assert not np.array_equal(amp[0], amp[1])  # (the liquid moved)
    assert np.array_equal(_bits(sim.state.pos), _bits(plain.state.pos)) and np.array_equal(_bits(sim.state.vel), _bits(plain.state.vel))
    mean = compute.spherical_average(np.mean(per_vector, axis=0), np.minimum((sf.q * 9 / sf.q_max).astype(int), 8), 9)[0]
    assert np.array_equal(rec.mean_structure_factor, mean, equal_nan=True)
    # a resized box has other wavevectors: refused until reset()
    from azplugins_amd.update import BoxResize

    L = float(syn.config_plj_sc(12)["L"][0])
    BoxResize.update(sim.state, azp.Box(1.01 * L))
    with pytest.raises(_lib.AzpError, match="reset"):
        rec._record(sim, 21)
    assert list(rec.timesteps) == [10, 20]
    rec.reset()
    rec._record(sim, 21)
    assert list(rec.timesteps) == [21] and np.array_equal(rec.amplitudes[0], sf.amplitudes)
