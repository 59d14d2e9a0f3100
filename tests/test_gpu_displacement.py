"""compute.MeanSquaredDisplacement, compute.SelfIntermediateScattering and their recorders on the GPU
(csrc/displacement.hip) against tests/displacement_ref.py: to the bit where every operation is exact, to the bit against
the restated order of summation, within the derived bounds on random systems, and bit-identical between two reads,
under a sort, between one launch over K origins and K launches, and between a run with and without the recorders.

Everything in the reference is indexed by tag; the rows of the state carry a random permutation of the tags, so a kernel
that walked the rows would not reproduce any of the sums below."""

import numpy as np
import pytest

import box_cases
import displacement_ref as ref
import structure_factor_ref as sref

import azplugins_amd as azp
from azplugins_amd import _lib, compute

pytestmark = pytest.mark.gpu

TYPE_NAMES = ("A", "B", "C", "D")  # (no particle is of type D)
CUBE = ((8.0, 8.0, 8.0), (0.0, 0.0, 0.0))
TILTED = ((9.0, 10.0, 11.0), (0.3, -0.2, 0.4))
BOXES = {"cube": CUBE, "tilted": TILTED}
GROUPS = {"all": None, "a": ("A",), "empty": ("D",)}
NS = 12


def _filter(names):
    return azp.All() if names is None else azp.Type(list(names))


def _member(names, types):
    return None if names is None else np.isin(types, [TYPE_NAMES.index(t) for t in names])


def _box(box):
    (Lx, Ly, Lz), (xy, xz, yz) = box
    return azp.Box(Lx, Ly, Lz, xy, xz, yz)


class _System:
    """A state whose row i carries tag ``tags[i]``; positions and images are given BY TAG."""

    def __init__(self, box, pos, image, types, tags):
        import torch

        self.n = n = len(pos)
        snap = azp.Snapshot.from_arrays(np.ascontiguousarray(pos[tags]), _box(box), typeid=np.asarray(types)[tags], types=TYPE_NAMES)
        self.sim = sim = azp.Simulation(device="cuda:0", seed=1)
        sim.create_state_from_snapshot(snap)
        st = sim.state
        st.tag[:n] = torch.from_numpy(np.asarray(tags, dtype=np.int32)).to(st.device)
        st.order_generation += 1
        self.put(pos, image)

    def put(self, pos, image):
        """Overwrite the positions and images of the state's rows, whatever order they are in now."""
        import torch

        st = self.sim.state
        tags = st.tag[: self.n].cpu().numpy().astype(np.int64)
        st.pos[: self.n, :3] = torch.from_numpy(np.ascontiguousarray(pos[tags])).to(st.device)
        st.image[: self.n] = torch.from_numpy(np.ascontiguousarray(image[tags], dtype=np.int32)).to(st.device)

    def add(self, c):
        self.sim.operations.computes.append(c)
        return c


def _two_times(n, box, seed):
    """Random wrapped positions and images (|n| <= 3) at two times, types 0, 1, 2 and a permutation of the tags."""
    rng = np.random.default_rng(seed)
    h = ref.box_ref.box_matrix(*box)
    pos0, pos = ((rng.random((n, 3)) - 0.5) @ h.T for _ in range(2))
    image0, image = (rng.integers(-3, 4, (n, 3)) for _ in range(2))
    return pos0, image0, pos, image, rng.integers(0, 3, n), rng.permutation(n)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


# ---------------------------------------------------------------------------
# exact
# ---------------------------------------------------------------------------
def test_exact_on_a_dyadic_lattice():
    """4 x 4 x 4 lattice of spacing 2 in a cube of 8, moved by multiples of 1/4 up to 3 along every axis and wrapped by
    hand; two particles carry three more images (their true displacement is 24 longer), one an image of 10^6 at both
    times. Every d is a multiple of 1/4 below 32, every product a multiple of 2^-8 below 2^20 and every sum of 64 terms
    exact: moments, displacements and histogram (bin width 1, scale 1; the three long displacements fall outside) equal
    the extended-precision reference to the bit. Moved by multiples of 2, m . df is a multiple of 1/4 and sincospi gives 0 and +-1: F_s is an exact integer sum."""
    rng = np.random.default_rng(11)
    g = np.array([-4.0, -2.0, 0.0, 2.0])
    pos0 = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    n = len(pos0)
    types, tags = np.arange(n) % 3, rng.permutation(n)
    image0 = np.zeros((n, 3), dtype=np.int64)
    image0[5] = 10 ** 6

    def moved(steps, unit):
        new = pos0 + steps * unit
        up, down = new >= 4.0, new < -4.0
        new = new - 8.0 * up + 8.0 * down
        return new, image0 + up.astype(np.int64) - down.astype(np.int64)

    steps = rng.integers(-12, 13, (n, 3))
    pos, image = moved(steps, 0.25)
    assert ((image - image0) == 1).sum() > 5 and ((image - image0) == -1).sum() > 0 and np.abs(image[5]).min() >= 10 ** 6 - 1
    extra = np.zeros((n, 3), dtype=np.int64)
    extra[7, 0], extra[9, 1], extra[11, 2] = 3, -3, 3
    image = image + extra
    want = steps * 0.25 + 8.0 * extra
    s = _System(CUBE, pos0, image0, types, tags)
    computes = {name: s.add(compute.MeanSquaredDisplacement(_filter(gr), num_bins=16, r_max=16.0)) for name, gr in GROUPS.items()}
    for c in computes.values():
        c.set_origin()
        assert c.origin_timestep == 0
    s.put(pos, image)
    d = ref.displacements(pos, image, pos0, image0, CUBE)
    assert np.array_equal(np.asarray(d, dtype=np.float64), want) and np.array_equal(ref.displacements_f64(pos, image, pos0, image0, CUBE), want)
    assert np.abs(want).max() > 24.0
    for name, gr in GROUPS.items():
        c, member = computes[name], _member(gr, types)
        row = c._read("row")
        exact = ref.moments(d, member)
        assert np.array_equal(_bits(row[:NS]), _bits(exact)), (name, row[:NS].view(np.float64), exact)
        assert np.array_equal(_bits(row[:NS]), _bits(ref.tree_moments(want, member)))
        counts, outside = ref.histogram(d, 16, 16.0, member, exact=True)
        assert row[NS] == 0 and row[NS + 1] == outside and np.array_equal(row[NS + 2:], counts), name
        assert np.array_equal(_bits(c.displacements), _bits(want))  # (every particle, in the group or not)
        p = compute.displacement_moments(exact)
        n_g = n if member is None else int(member.sum())
        assert c.num_particles == n_g and c.msd == p["msd"] and np.array_equal(c.msd_tensor, p["msd_tensor"])
        assert np.array_equal(c.van_hove_counts, counts) and c.outside == outside
        assert np.array_equal(c.non_gaussian, p["non_gaussian"], equal_nan=True) and c.fourth_moment == p["fourth_moment"]
        if n_g:
            direct = (want[slice(None) if member is None else member] ** 2).sum() / n_g
            assert abs(c.msd - direct) <= 3 * ref.U * direct  # (the rounded 1 / N_g and one product)
    assert computes["empty"].msd == 0.0 and np.array_equal(computes["empty"].mean_displacement, np.zeros(3))
    assert computes["all"].outside == 3 and computes["all"].van_hove.shape == (16,)
    # F_s: moves by multiples of the lattice spacing
    steps2 = rng.integers(-1, 2, (n, 3))
    pos2, image2 = moved(steps2, 2.0)
    s.put(pos0, image0)
    fs = {name: s.add(compute.SelfIntermediateScattering(_filter(gr), 2.0 * np.pi * 2.5 / 8.0, 5)) for name, gr in GROUPS.items()}
    for c in fs.values():
        c.set_origin()
    s.put(pos2, image2)
    for name, gr in GROUPS.items():
        c, member = fs[name], _member(gr, types)
        m = c.vectors
        quarter = (steps2 @ m.T) % 4  # m . df in quarters, per (particle, vector)
        if member is not None:
            quarter = quarter[member]
        re = np.array([1.0, 0.0, -1.0, 0.0])[quarter].sum(axis=0)
        im = np.array([0.0, -1.0, 0.0, 1.0])[quarter].sum(axis=0)
        row = c._read("row")
        assert len(m) > 25 and np.array_equal(row[:len(m)], re) and np.array_equal(row[len(m):2 * len(m)], im), name
        assert row[-2] == len(quarter) and row[-1] == 0.0 and c.num_particles == len(quarter)
        if name == "all":
            assert np.abs(re).max() < n and np.abs(im).max() > 0 and np.array_equal(c.vector_scattering, re * (1.0 / n))


# ---------------------------------------------------------------------------
# the order of summation
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 257, 16385, 524289])
def test_sums_in_tag_order_equal_the_restated_tree_sum(n):
    """dx = 2^-k with random k in [0, 30]: dx, dx^2 >= 2^-60 and dx^4 >= 2^-120 are exact, their sums are not, so the row
    shows the order of the additions: it equals reduction_ref.tree_sum over the terms IN TAG ORDER to the bit. (Sums of
    powers of two often round alike in two orders, so dy is a uniform random double: d_y = y - 0 is exact, its products
    are single IEEE multiplications that numpy repeats bit for bit, and their sums differ between tag order and row
    order, which the test asserts of its own data.) 16,385: 65 partials, the second trip of the fold; 524,289: two tags
    per lane."""
    rng = np.random.default_rng(1000 + n)
    k = rng.integers(0, 31, n)
    pos0 = np.zeros((n, 3))
    pos = np.stack([2.0 ** -k, rng.uniform(-1.0, 1.0, n), np.zeros(n)], axis=1)
    image = np.zeros((n, 3), dtype=np.int64)
    types, tags = np.arange(n) % 3, rng.permutation(n)
    assert ref.reduction_ref.shape(n) == {1: (1, 1), 255: (1, 1), 257: (1, 2), 16385: (1, 65), 524289: (2, 1025)}[n]
    s = _System(CUBE, pos0, image, types, tags)
    for gr in (None, ("A",)):
        c = s.add(compute.MeanSquaredDisplacement(_filter(gr)))
        c.set_origin()
    s.put(pos, image)
    d64 = ref.displacements_f64(pos, image, pos0, image, CUBE)
    assert np.array_equal(d64, pos)
    for c, gr in zip(s.sim.operations.computes, (None, ("A",))):
        member = _member(gr, types)
        row = c._read("row")
        want = ref.tree_moments(d64, member)
        assert row.shape == (NS + 2,) and np.array_equal(_bits(row[:NS]), _bits(want)), (n, gr, row[:NS].view(np.float64), want)
        if n > 255 and member is None:
            in_row_order = ref.tree_moments(d64[tags])
            assert not np.array_equal(_bits(in_row_order), _bits(want))  # (the test tells the two orders apart)


# ---------------------------------------------------------------------------
# random systems within the derived bounds
# ---------------------------------------------------------------------------
SEEDS = {("cube", 257): 21, ("cube", 515): 22, ("tilted", 257): 23, ("tilted", 515): 24, ("tilted", 131073): 25}
R_MAX, NUM_BINS = 50.0, 50


def _check_bounded(box_name, n, groups, q_max):
    box = BOXES[box_name]
    pos0, image0, pos, image, types, tags = _two_times(n, box, SEEDS[(box_name, n)])
    s = _System(box, pos0, image0, types, tags)
    msd = {g: s.add(compute.MeanSquaredDisplacement(_filter(GROUPS[g]), num_bins=NUM_BINS, r_max=R_MAX)) for g in groups}
    fs = {g: s.add(compute.SelfIntermediateScattering(_filter(GROUPS[g]), q_max, 6)) for g in groups}
    for c in list(msd.values()) + list(fs.values()):
        c.set_origin()
    s.put(pos, image)
    d = ref.displacements(pos, image, pos0, image0, box)
    A = ref.magnitudes(pos, image, pos0, image0, box)
    n_vectors = 0
    for g in groups:
        member = _member(GROUPS[g], types)
        n_g = n if member is None else int(member.sum())
        row = msd[g]._read("row")
        got, want, b = row[:NS].view(np.float64), ref.moments(d, member), ref.moments_bound(A, member)
        err = np.abs(got - want)
        print("%s N=%d %s: moments, worst %.3g of the bound; depth %d" % (box_name, n, g, (err[1:11] / np.maximum(b[1:11], 1e-300)).max(), ref.depth(n)))
        assert got[0] == n_g and got[11] == 0.0 and np.all(err <= b), (g, err, b)
        counts, outside = ref.histogram(d, NUM_BINS, R_MAX, member)  # (asserts that no sample is near an edge)
        assert row[NS] == 0 and row[NS + 1] == outside and np.array_equal(row[NS + 2:], counts), g
        if n_g:
            assert outside > 0 and counts.sum() > 0
        derr = np.abs(msd[g].displacements - np.asarray(d, dtype=np.float64))
        assert np.all(derr <= ref.displacement_bound(A) + 2.0 ** -64 * A), (g, (derr / ref.displacement_bound(A)).max())
        m = fs[g].vectors
        n_vectors = len(m)
        D = sref.depth(n, n_vectors)
        re, im = ref.self_amplitudes(pos, pos0, box, m, member)
        fb = ref.fs_bound(m, n_g, D, box)
        assert fb.max() <= n_g * 2.0 ** -52 * (32 * np.abs(m).sum(axis=1).max() + 16 + D)
        frow = fs[g]._read("row")
        ferr = np.maximum(np.abs(frow[:n_vectors] - re), np.abs(frow[n_vectors:2 * n_vectors] - im))
        print("%s N=%d %s: F_s on %d vectors, worst error %.3g, %.3g of the bound" % (box_name, n, g, n_vectors, ferr.max(),
                                                                                     (ferr / np.maximum(fb, 1e-300)).max()))
        assert np.all(ferr <= fb) and frow[-2] == n_g and frow[-1] == 0.0, (g, ferr.max(), fb.min())
        if n_g:
            assert np.abs(frow[:n_vectors]).max() < 0.5 * n_g  # (random displacements: nothing coherent is left)
    return n_vectors


@pytest.mark.parametrize("n", [257, 515])
@pytest.mark.parametrize("box_name", ["cube", "tilted"])
def test_random_systems_within_the_derived_bounds(box_name, n):
    n_vectors = _check_bounded(box_name, n, ("all", "a", "empty"), 2.0 * np.pi * 4.5 / 8.0 if box_name == "cube" else 2.9)
    assert n_vectors == 194 if box_name == "cube" else n_vectors > 100
    assert sref.shape(n, n_vectors) == (1, -(-n // 256))


def test_chunks_of_two_stages_and_many_partials():
    """131,073 particles: chunks of two stages, the stage loop that ends early and a fold over 257 partials (the shapes
    tests/test_gpu_structure_factor.py argues for), with 65 vectors; the moments run 513 workgroups there."""
    n = 512 * 256 + 1
    assert sref.shape(n, 65) == (2, 257) and ref.reduction_ref.shape(n) == (1, 513)
    assert _check_bounded("tilted", n, ("a",), 2.0) == 65


# ---------------------------------------------------------------------------
# bit-identical: two reads, a sort, K origins in one launch
# ---------------------------------------------------------------------------
def _rows(computes):
    return [c._read("row").copy() for c in computes]


def test_two_reads_and_a_sort_change_no_bit():
    pos0, image0, pos, image, types, tags = _two_times(2000, TILTED, 31)
    s = _System(TILTED, pos0, image0, types, tags)
    computes = [s.add(compute.MeanSquaredDisplacement(azp.Type(["A", "B"]), num_bins=40, r_max=60.0)),
                s.add(compute.SelfIntermediateScattering(azp.Type(["A", "B"]), 2.0, 6))]
    for c in computes:
        c.set_origin()
    s.put(pos, image)
    first, second = _rows(computes), _rows(computes)
    disp = computes[0].displacements
    for a, b in zip(first, second):
        assert np.array_equal(_bits(a), _bits(b))
    st = s.sim.state
    tag0 = st.tag[: st.N].cpu().numpy().copy()
    generation = st.order_generation
    azp.ParticleSorter(particles_per_block=16).sort(s.sim)
    assert not np.array_equal(st.tag[: st.N].cpu().numpy(), tag0) and st.order_generation == generation + 1  # (the rows moved)
    for a, b in zip(first, _rows(computes)):
        assert np.array_equal(_bits(a), _bits(b))
    assert np.array_equal(_bits(disp), _bits(computes[0].displacements))
    assert first[0][:1].view(np.float64)[0] == np.isin(types, (0, 1)).sum() and np.abs(first[1][:65]).max() > 0.0
    # a new origin after the sort is the same origin: it is stored by tag
    s.put(pos0, image0)
    for c in computes:
        c.set_origin()
    s.put(pos, image)
    for a, b in zip(first, _rows(computes)):
        assert np.array_equal(_bits(a), _bits(b))


def test_one_launch_over_a_ring_equals_one_launch_per_origin():
    """A store of four slots with three filled: the rows of one launch equal three single-origin launches to the bit,
    the slot that was never filled gives zeros (whatever the store holds there)."""
    import torch

    n = 515
    times = [_two_times(n, TILTED, 40 + k) for k in range(2)]
    pos_t = [times[0][0], times[0][2], times[1][0], times[1][2]]
    img_t = [times[0][1], times[0][3], times[1][1], times[1][3]]
    types, tags = times[0][4], times[0][5]
    s = _System(TILTED, pos_t[0], img_t[0], types, tags)
    st = s.sim.state
    for c in (s.add(compute.MeanSquaredDisplacement(azp.Type(["B", "C"]), num_bins=30, r_max=60.0)),
              s.add(compute.SelfIntermediateScattering(azp.Type(["B", "C"]), 2.0, 6))):
        pos0, image0 = c._store(st, 4)
        pos0.fill_(float("nan"))
        image0.fill_(12345)
        for slot, k in ((0, 0), (2, 1), (1, 2)):  # (filled out of order; slot 3 stays empty)
            s.put(pos_t[k], img_t[k])
            c._scatter(st, pos0, image0, slot)
        s.put(pos_t[3], img_t[3])
        w = c._row_width()
        dtype = torch.int64 if isinstance(c, compute.MeanSquaredDisplacement) else torch.float64
        ring = torch.full((4, w), 7, dtype=dtype, device=st.device)
        c._launch_slots(ring.data_ptr(), st, pos0, image0, 4, 0b0111)
        ring = ring.cpu().numpy()
        for slot in range(3):
            one = torch.full((1, w), 7, dtype=dtype, device=st.device)
            c._launch_slots(one.data_ptr(), st, pos0[slot:slot + 1], image0[slot:slot + 1], 1, 1)
            assert np.array_equal(_bits(ring[slot]), _bits(one.cpu().numpy()[0])), (type(c).__name__, slot)
        assert not np.array_equal(_bits(ring[0]), _bits(ring[1])) and not np.array_equal(_bits(ring[1]), _bits(ring[2]))
        assert np.array_equal(_bits(ring[3]), np.zeros(w, dtype=np.int64))
        # and against the reference, so that the slots are the origins they are meant to be
        if isinstance(c, compute.MeanSquaredDisplacement):
            member = np.isin(types, (1, 2))
            for slot, k in ((0, 0), (2, 1), (1, 2)):
                d = ref.displacements(pos_t[3], img_t[3], pos_t[k], img_t[k], TILTED)
                A = ref.magnitudes(pos_t[3], img_t[3], pos_t[k], img_t[k], TILTED)
                assert np.all(np.abs(ring[slot][:NS].view(np.float64) - ref.moments(d, member)) <= ref.moments_bound(A, member))


# ---------------------------------------------------------------------------
# the recorders inside Simulation.run
# ---------------------------------------------------------------------------
RUN_N, RUN_STEPS, RUN_DT, PERIOD = 512, 400, 0.05, 40


def _free_flight(recorders):
    """The free flight of tests/test_gpu_box_wrap.py: 512 particles in the tilt3 box, |v| dt of 1 to 1.4 (0.2 of an edge),
    no forces, NVE; every particle crosses many faces along every axis."""
    L, tilt, _ = box_cases.BOXES["tilt3"]
    rng = np.random.default_rng(404)
    x0 = rng.uniform(-0.5, 0.5, (RUN_N, 3)) @ ref.box_ref.box_matrix(L, tilt).T
    u = rng.normal(size=(RUN_N, 3))
    v = u / np.linalg.norm(u, axis=1)[:, None] * rng.uniform(20.0, 28.0, (RUN_N, 1))
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(azp.Snapshot.from_arrays(x0, azp.Box(L[0], L[1], L[2], *tilt), typeid=np.arange(RUN_N) % 2, types=("A", "B"),
                                                            velocity=v))
    sim.operations.tuners.clear()  # (the saved states are compared by row)
    sim.operations.integrator = azp.Integrator(dt=RUN_DT, forces=[], methods=[azp.ConstantVolume()])
    msd = compute.MeanSquaredDisplacement(azp.Type(["A"]), num_bins=20, r_max=400.0)
    fs = compute.SelfIntermediateScattering(azp.All(), 2.2, 5)
    sim.operations.add(msd)
    sim.operations.add(fs)
    recs = None
    if recorders:
        recs = (compute.MeanSquaredDisplacementRecorder(msd, PERIOD, origins=4, origin_every=2),
                compute.SelfIntermediateScatteringRecorder(fs, PERIOD, origins=4, origin_every=2))
        for r in recs:
            sim.operations.add(r)
    return sim, msd, fs, recs, v


def test_recorders_in_a_run():
    import torch

    sim, msd, fs, (rec_m, rec_f), v = _free_flight(True)
    sim.run(RUN_STEPS)
    steps = list(range(PERIOD, RUN_STEPS + 1, PERIOD))
    assert list(rec_m.timesteps) == steps and list(rec_f.timesteps) == steps and len(steps) == 10
    # origins at the firings 0, 2, 4, 6, 8: the fifth overwrites slot 0
    origin_steps = np.full((10, 4), -1, dtype=np.int64)
    slots = [-1] * 4
    for k, t in enumerate(steps):
        if k % 2 == 0:
            slots[(k // 2) % 4] = t
        origin_steps[k] = slots
    assert origin_steps[8, 0] == 360 and origin_steps[7, 0] == 40 and origin_steps[0, 1] == -1
    for rec in (rec_m, rec_f):
        assert np.array_equal(rec.origin_timesteps, origin_steps)
        lags, samples, _ = compute.average_over_origins(steps, origin_steps, np.zeros((10, 4, 0)))
        assert np.array_equal(rec.lags, lags) and np.array_equal(rec.samples_per_lag, samples)
        # (origin 40 is held up to row 320, origin 120 up to row 400: lags up to 280; 2 + 4 + 6 + 16 filled pairs)
        assert list(lags) == list(range(0, 281, 40)) and samples[0] == 5 and samples.sum() == (origin_steps >= 0).sum() == 28
    # the same run without recorders, stopped at every firing: its states are the ones the rows were written from
    plain, msd2, fs2, _, _ = _free_flight(False)
    saved = {}
    for t in steps:
        plain.run(PERIOD)
        assert plain.timestep == t
        saved[t] = (plain.state.pos.clone(), plain.state.image.clone())
    assert np.array_equal(_bits(sim.state.pos.cpu().numpy()), _bits(plain.state.pos.cpu().numpy()))
    assert np.array_equal(sim.state.image.cpu().numpy(), plain.state.image.cpu().numpy())
    assert np.array_equal(_bits(sim.state.vel.cpu().numpy()), _bits(plain.state.vel.cpu().numpy()))
    image = plain.state.image.cpu().numpy()
    assert np.all((image != 0).sum(axis=0) > RUN_N // 2) and np.abs(image).max() > 10
    table_m = rec_m._host_rows(np.int64)
    table_f = rec_f._host_rows(np.float64)
    n_vec = len(fs.vectors)
    assert table_m.shape == (10, 4, NS + 2 + 20) and table_f.shape == (10, 4, 2 * n_vec + 2) and n_vec > 20
    st = plain.state
    for k, t in enumerate(steps):
        for slot in range(4):
            t0 = origin_steps[k, slot]
            if t0 < 0:
                assert not table_m[k, slot].any() and not table_f[k, slot].any()
                continue
            st.pos.copy_(saved[int(t0)][0])
            st.image.copy_(saved[int(t0)][1])
            msd2.set_origin()
            fs2.set_origin()
            st.pos.copy_(saved[t][0])
            st.image.copy_(saved[t][1])
            assert np.array_equal(_bits(table_m[k, slot]), _bits(msd2._read("row"))), (t, t0)
            assert np.array_equal(_bits(table_f[k, slot]), _bits(fs2._read("row"))), (t, t0)
            if t0 == t:  # lag 0: exactly nothing moved
                sums = table_m[k, slot][:NS].view(np.float64)
                assert sums[0] == RUN_N // 2 and not sums[1:].any() and table_m[k, slot][NS + 2] == RUN_N // 2
                assert np.array_equal(table_f[k, slot], np.concatenate([np.full(n_vec, float(RUN_N)), np.zeros(n_vec), [RUN_N, 0.0]]))
    tm, tf = rec_m.table, rec_f.table
    assert tm["msd"].shape == (10, 4) and tm["msd_tensor"].shape == (10, 4, 3, 3) and tm["van_hove_counts"].shape == (10, 4, 20)
    assert tm["msd"][0, 0] == 0.0 and tm["msd"][1, 0] > 0.0 and tf["vector_scattering"].shape == (10, 4, n_vec)
    assert np.array_equal(tf["vector_scattering"][0, 0], np.ones(n_vec)) and np.array_equal(tf["num_particles"][0], [RUN_N, 0, 0, 0])
    # msd(lag) of a free flight is <|v|^2> (lag dt)^2. Tolerance: tests/test_gpu_box_wrap.py holds the unwrapped position
    # after n steps to n x 2 x 3.6e-15 of x0 + v n dt per component (per step one rounding of the FMA x + dt v and one
    # per shift of the wrap, of coordinates below 16). A displacement is the difference of two such positions, at most 400
    # steps each: e = 2 x 400 x 7.2e-15 = 5.8e-12 per component, plus the compute's own 6 u A with A below 2 (|d| + |H| 3)
    # < 1200: 8e-13; e = 7e-12 covers both. msd moves by at most the mean of sum_a (2 |v_a| lag dt e + e^2) over the
    # group, the summation by depth u msd (24 x 1.1e-16, counted as 1e-14 msd), and the expectation itself, evaluated
    # in float64, by a few u.
    in_a = np.arange(RUN_N) % 2 == 0
    e = 7e-12
    lags = rec_m.lags
    want = (v[in_a] ** 2).sum(axis=1).mean() * (lags * RUN_DT) ** 2
    tol = np.array([(2.0 * np.abs(v[in_a]) * lag * RUN_DT * e + e * e).sum(axis=1).mean() for lag in lags]) + 1e-14 * want
    got = rec_m.msd
    print("msd(lag) against <v^2> (lag dt)^2: worst |error| / tolerance %.3g" % (np.abs(got - want)[1:] / tol[1:]).max())
    assert got[0] == 0.0 and np.all(np.abs(got - want) <= tol)
    assert np.allclose(rec_m.msd_components.sum(axis=1), got, rtol=1e-14) and np.isnan(rec_m.non_gaussian[0])
    assert rec_m.van_hove.shape == (len(lags), 20) and rec_f.scattering.shape == (len(lags), 5)
    sc = rec_f.scattering
    assert np.array_equal(sc[0][~np.isnan(sc[0])], np.ones((~np.isnan(sc[0])).sum())) and np.nanmax(np.abs(sc[1:])) < 0.5
    # another box: refused until reset()
    from azplugins_amd.update import BoxResize

    L = box_cases.BOXES["tilt3"][0]
    BoxResize.update(sim.state, azp.Box(1.01 * L[0], L[1], L[2], *box_cases.BOXES["tilt3"][1]))
    for rec in (rec_m, rec_f):
        with pytest.raises(_lib.AzpError, match="reset"):
            rec._record(sim, 401)
        assert len(rec.timesteps) == 10
        rec.reset()
        rec._record(sim, 401)
        assert list(rec.timesteps) == [401] and list(rec.lags) == [0] and np.array_equal(rec.origin_timesteps, [[401, -1, -1, -1]])
    torch.cuda.synchronize()


def test_collective_intermediate_scattering_from_the_recorded_amplitudes():
    """StructureFactorRecorder.intermediate_scattering is the host function on the table the recorder already keeps."""
    pos0, image0, pos, image, types, tags = _two_times(300, TILTED, 61)
    s = _System(TILTED, pos0, image0, types, tags)
    sf = s.add(compute.StructureFactor(azp.Type(["A"]), azp.All(), 2.0, 6))
    rec = compute.StructureFactorRecorder(sf, 1)
    assert rec.intermediate_scattering[0].shape == (0,)
    rec._record(s.sim, 0)
    s.put(pos, image)
    rec._record(s.sim, 5)
    rec._record(s.sim, 10)
    lags, F = rec.intermediate_scattering
    amp, n_a = rec.amplitudes, int((types == 0).sum())
    assert list(lags) == [0, 5, 10] and F.shape == (3, 65) and amp.shape == (3, 2, 65)
    assert np.array_equal(F, compute.intermediate_scattering_from_amplitudes(amp, [0, 5, 10], (n_a, 300))[1])
    norm = np.sqrt(n_a * 300.0)
    assert np.allclose(F[2], (amp[2, 0] * np.conj(amp[0, 1])).real / norm, rtol=1e-14, atol=0)  # (the one pair of lag 10)
    assert np.allclose(F[0], rec._per_vector("s").mean(axis=0), rtol=1e-13, atol=1e-13)  # (lag 0: the static S_AB; terms of order 1)


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
def test_refusals_when_read():
    import torch

    pos0, image0, pos, image, types, tags = _two_times(300, CUBE, 51)
    s = _System(CUBE, pos0, image0, types, tags)
    sim, st = s.sim, s.sim.state
    msd = compute.MeanSquaredDisplacement(azp.All(), num_bins=10, r_max=50.0)
    fs = compute.SelfIntermediateScattering(azp.All(), 2.0, 4)
    for c, read in ((msd, lambda: msd.msd), (fs, lambda: fs.scattering)):
        with pytest.raises(compute.DataAccessError):
            read()
        s.add(c)
        assert c.origin_timestep is None
        read()  # (the first read takes the origin)
        assert c.origin_timestep == 0
    assert msd.msd == 0.0 and np.array_equal(fs.vector_scattering, np.ones(len(fs.vectors))) and np.nanmax(np.abs(fs.imaginary)) == 0.0
    # a forged tag: the slot of the tag it replaced has no particle
    good = st.tag[7].item()
    st.tag[7] = 300
    for c, read in ((msd, lambda: msd.msd), (msd, lambda: msd.displacements), (fs, lambda: fs.scattering)):
        with pytest.raises(_lib.AzpError, match="permutation"):
            read()
    assert msd._read_row("row", "int64").cpu().numpy()[0, NS] == 1
    st.tag[7] = good
    assert msd.msd == 0.0
    # a decomposed run
    sim.domain = object()
    for read in (lambda: msd.msd, lambda: fs.scattering, msd.set_origin):
        with pytest.raises(_lib.AzpError, match="decomposed"):
            read()
    sim.domain = None
    # a box that changed after the origin was taken
    sim.state.box = azp.Box(8.5)
    for read in (lambda: msd.msd, lambda: msd.displacements, lambda: fs.scattering):
        with pytest.raises(_lib.AzpError, match="new origin"):
            read()
    msd.set_origin()
    fs.set_origin()
    assert msd.msd == 0.0 and fs.num_particles == 300
    # not periodic on every axis: the scattering only; two-dimensional: both
    sim.state.box = azp.Box(8.0, 8.0, 8.0, periodic=(True, True, False))
    msd.set_origin()
    assert msd.num_particles == 300
    with pytest.raises(_lib.AzpError, match="periodic"):
        fs.scattering
    sim.state.box = azp.Box(8.0, 8.0, 0.0)
    for read in (lambda: msd.msd, lambda: fs.scattering):
        with pytest.raises(_lib.AzpError, match="3-D"):
            read()
    # a replaced state drops the origin
    sim.create_state_from_snapshot(azp.Snapshot.from_arrays(pos0, _box(CUBE), types=TYPE_NAMES))
    assert msd.origin_timestep is None and msd.msd == 0.0 and msd.origin_timestep == 0
    torch.cuda.synchronize()
