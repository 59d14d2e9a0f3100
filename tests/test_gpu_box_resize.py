"""``azp_box_resize`` (csrc/box_resize.hip) through the C ABI against tests/box_resize_ref.py, and ``update.BoxResize`` /
``State.set_box`` through ``Simulation.run``: neighbor lists, steppers and recorders have to follow a box that changes.

BOUND = 8.5 ulp of a coordinate in [8, 16) = 8.5 * 1.78e-15 = 1.51e-14 absolute per component, from the arithmetic that
include/azp.h fixes. All coordinates, all partial sums of the map and all shift products stay below 16 (asserted), so
every rounding below is at most half an ulp of that binade, 8.9e-16.

* The map of a selected row. The kernel evaluates x' = fma(M02, z, fma(M01, y, M00 * x)): three roundings. The reference
  evaluates M00 x + M01 y + M02 z with plain products and sums: five. The six numbers of M are the same (both take them
  from ``update.box_resize_matrix``), so the two results are at most 8 half-ulps = 4 ulp apart; y' (two against three
  roundings) and z' (one against one, the same bits) are closer.
* The wrap. A selected row takes at most one shift per axis, and x collects up to three (z's carry Lz xz, y's carry
  Ly xy, its own Lx). A tilted shift is one FMA in the kernel and a product and a difference in numpy: the product's
  rounding and the two results' roundings, 1.5 ulp per shift, 4.5 ulp for x (tests/test_gpu_box_wrap.py counts the same
  shifts; its boxes make most products exact, these do not). Together 8.5 ulp.
* A row that is not selected has no map. Its shift by k lattice vectors is fma(-k, (Lz xz), x) in the kernel and
  x - k * (Lz xz) in numpy, with (Lz xz) rounded once in both: again at most 1.5 ulp per shift and 4.5 ulp for x; the one-shift
  wrap behind it moves nothing, because no end point lies on a face. Within the same bound.

Both sides must take the same branches: the shift counts are read off fractional coordinates, so a row within rounding of
a face could be shifted by one and not by the other. As in tests/box_cases.py no REFERENCE end point lies within 1e-9
(fractional) of a face of the new box; the seeds are chosen for that on the CPU (tests/test_box_resize.py) and every
case asserts it again. No row is left out of any comparison.

The fractional coordinates of a selected row move by at most BOUND as well (modulo whole images): a deviation d of a
position is d (1 + |xy| + |xz - xy yz|) / Lx <= 2 d / 3.6 in fractional x, and computing the two fractional coordinates
adds a few ulp of 16 / 3.6 -- both below BOUND. Measured maxima per case: profiles/box_resize.md."""

import ctypes as C

import numpy as np
import pytest

import box_ref
import box_resize_ref as ref
from azplugins_amd import _lib

pytestmark = pytest.mark.gpu

BOUND = 8.5 * float(np.spacing(8.0))
ULP_HALF = float(np.spacing(0.5))
FORCE_TOL = 1e-10  # of the largest force: what tests/test_gpu_auto_plan.py (TOL) holds PerturbedLJ forces to across list rebuilds


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a)).to("cuda:0")  # (a copy: the cases are read-only)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def _launch(c, old, new, masked, with_image, block_size=0):
    import torch

    N = c["pos"].shape[0]
    type_w = c["typeid"].astype(np.int64).view(np.float64)
    t = dict(pos=_dev(np.c_[c["pos"], type_w]), vel=_dev(c["vel"]), image=_dev(np.array(c["image"])), mask=_dev(ref.MASK))
    a = _lib.BoxResizeArgs()
    a.d_pos = t["pos"].data_ptr()
    a.d_image = t["image"].data_ptr() if with_image else None
    a.d_type_mask = t["mask"].data_ptr() if masked else None
    a.N, a.ntypes, a.block_size = N, 3, block_size
    M = ref.matrix(old, new)
    a.M[:] = (M[0, 0], M[0, 1], M[0, 2], M[1, 1], M[1, 2], M[2, 2])
    a.box = _lib.make_box(*new)
    _lib.check(_lib.lib().azp_box_resize(C.byref(a), _lib.raw_stream("cuda:0")), "azp_box_resize")
    torch.cuda.synchronize()
    return {k: t[k].cpu().numpy() for k in ("pos", "vel", "image")}


CASES = ([(p, 1037, False) for p in ref.PAIRS] + [(p, 1037, True) for p in ref.SHRUNK]
         + [("tilt3_to_tilt3", 1, False), ("tilt3_x0.3", 1, True)])


@pytest.mark.parametrize("pair_id,N,masked", CASES)
def test_kernel_against_reference(pair_id, N, masked):
    old, new = ref.ALL_PAIRS[pair_id]
    c = ref.case(pair_id, N, masked)
    want_pos, want_image, sel = ref.resize(c["pos"], c["image"], c["typeid"], ref.MASK if masked else None, old, new)
    # the conditions the comparison rests on, from the reference alone
    margin = ref.face_distance(want_pos, new)
    assert margin > ref.FACE_MARGIN, margin
    M, x, y, z = ref.matrix(old, new), c["pos"][:, 0], c["pos"][:, 1], c["pos"][:, 2]
    partial = [M[0, 0] * x, M[0, 1] * y, M[0, 2] * z, M[0, 0] * x + M[0, 1] * y, M[1, 1] * y, M[1, 2] * z, c["pos"],
               ref.affine(c["pos"], M), want_pos]
    assert max(np.abs(p).max() for p in partial) < 16.0
    (Lx, Ly, Lz), (xy, xz, yz), _ = new
    shifts = int(np.abs(want_image - c["image"]).max())  # (a shift by k lattice vectors is k times such a product)
    assert shifts <= 2 and shifts * max(Lx, Ly, Lz, abs(Lz * yz), abs(Lz * xz), abs(Ly * xy)) < 16.0
    if N > 1:
        counts = ref.near_face_counts(want_pos, new)
        assert min(counts.values()) >= ref.MIN_NEAR, counts
    got = _launch(c, old, new, masked, with_image=True)
    # 1. the image counters, exactly
    np.testing.assert_array_equal(got["image"], want_image)
    # 2. what the kernel must not touch
    np.testing.assert_array_equal(_bits(got["pos"][:, 3]), c["typeid"].astype(np.int64))
    np.testing.assert_array_equal(_bits(got["vel"]), _bits(c["vel"]))
    # 3. every row within BOUND
    dev = np.abs(got["pos"][:, :3] - want_pos)
    f0, f1 = box_ref.fractional(c["pos"], old[0], old[1]), box_ref.fractional(got["pos"][:, :3], new[0], new[1])
    d = (f1 - f0)[sel]
    for k in range(3):
        if new[2][k]:
            d[:, k] -= np.rint(d[:, k])
    print("%s N=%d %s: largest deviation %.3e (selected %.3e, unselected %.3e; bound %.3e), largest change of a selected row's "
          "fractional coordinates %.3e; nearest face %.2e; %d of %d rows shifted"
          % (pair_id, N, "Type mask" if masked else "All", dev.max(), dev[sel].max() if sel.any() else 0.0,
             dev[~sel].max() if (~sel).any() else 0.0, BOUND, np.abs(d).max() if sel.any() else 0.0, margin,
             int((want_image != c["image"]).any(axis=1).sum()), N))
    assert dev.max() <= BOUND
    # 4. a selected row keeps its fractional coordinates; an unselected one its position, up to whole lattice vectors
    if sel.any():
        assert np.abs(d).max() <= BOUND
    shift = (got["image"] - c["image"]).astype(np.float64) @ box_ref.box_matrix(new[0], new[1]).T
    if (~sel).any():
        assert np.abs(got["pos"][~sel, :3] + shift[~sel] - c["pos"][~sel]).max() <= BOUND
    # 5. every periodic fractional coordinate in [-0.5, 0.5); a non-periodic axis is scaled but not wrapped
    for k in range(3):
        if new[2][k]:
            assert f1[:, k].min() >= -0.5 - 4 * ULP_HALF and f1[:, k].max() < 0.5 + 4 * ULP_HALF, k
        else:
            assert np.array_equal(got["image"][:, k], c["image"][:, k])
            assert np.abs(f1[sel, k] - f0[sel, k]).max() <= BOUND if sel.any() else True
    # 6. d_image = NULL: the same positions bit for bit, the counters untouched; and another launch shape changes nothing
    bare = _launch(c, old, new, masked, with_image=False)
    assert np.array_equal(_bits(bare["pos"]), _bits(got["pos"])) and np.array_equal(bare["image"], c["image"])
    narrow = _launch(c, old, new, masked, with_image=True, block_size=64)
    assert np.array_equal(_bits(narrow["pos"]), _bits(got["pos"])) and np.array_equal(narrow["image"], got["image"])


def test_no_particles_is_no_launch():
    import torch

    a = _lib.BoxResizeArgs()  # (no arrays at all)
    a.box = _lib.make_box((6.0, 7.0, 8.0))
    a.M[:] = (1.0, 0.0, 0.0, 1.0, 0.0, 1.0)
    _lib.check(_lib.lib().azp_box_resize(C.byref(a), _lib.raw_stream("cuda:0")), "azp_box_resize")
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# through Simulation.run: 576 particles of PerturbedLJ (r_cut 2.5, buffer 0.4) at rho* = 0.58 in a cube of edge 10
# ---------------------------------------------------------------------------------------------------------------------
L0, R_CUT, BUFFER, DT = 10.0, 2.5, 0.4, 0.002
SHRINK = 0.95  # (the edge stays above 2 (r_cut + buffer) = 5.8)


def _start(shell=False):
    """Jittered 8 x 8 x 9 lattice and velocities. The first plane of the lattice lies in a face of the box, so that
    particles cross faces from the first step on; ``shell``: the last plane lies 0.1 inside the upper faces instead and
    the jitter is 0.03, so that no particle crosses a face in a few steps, but some lie outside a box 3 % smaller."""
    rng = np.random.default_rng(576)
    if shell:
        g = [(np.arange(n) + 1) * (L0 / n) - 0.5 * L0 - 0.1 for n in (8, 8, 9)]
    else:
        g = [np.arange(n) * (L0 / n) - 0.5 * L0 for n in (8, 8, 9)]
    X, Y, Z = np.meshgrid(*g, indexing="ij")
    xyz = np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1) + rng.uniform(-1.0, 1.0, (576, 3)) * (0.03 if shell else 0.1)
    xyz -= L0 * np.floor(xyz / L0 + 0.5)
    return xyz, rng.normal(0.0, 2.0, (576, 3))


def _sim(xyz=None, box=None, velocity=None, methods="nve", timestep=1):
    """The system (or one made of ``xyz`` in ``box``), its list and its pair force. The run tests start at timestep 1, so
    that in ``run(20)`` a ``Periodic(5)`` fires at the start of the steps 5, 10, 15 and 20: four resizes, the last one to
    the final box of a ramp that ends at 20."""
    import azplugins_amd as azp
    from azplugins_amd import flow, minimize, thermostats

    x0, v0 = _start()
    sim = azp.Simulation(device="cuda:0", seed=3)
    sim.create_state_from_snapshot(azp.Snapshot.from_arrays(x0 if xyz is None else xyz, azp.Box.cube(L0) if box is None else box,
                                                            velocity=v0 if velocity is None else velocity))
    sim.operations.tuners.clear()  # rows are compared by index
    nl = azp.nlist.Cell(buffer=BUFFER)
    plj = azp.pair.PerturbedLennardJones(nlist=nl, default_r_cut=R_CUT, mode="shift")
    plj.params[("A", "A")] = dict(epsilon=1.0, sigma=1.0, attraction_scale_factor=0.5)
    if methods == "fire":
        sim.operations.integrator = minimize.FIRE(dt=DT, force_tol=1e-7, angmom_tol=1e-7, energy_tol=1e-12, forces=[plj],
                                                  methods=[azp.ConstantVolume()])
    else:
        m = {"nve": lambda: azp.ConstantVolume(), "bussi": lambda: azp.ConstantVolume(thermostat=thermostats.Bussi(kT=1.0, tau=0.1)),
             "langevin": lambda: flow.Langevin(filter=azp.All(), kT=1.0, flow_field=flow.ConstantFlow(velocity=(0.3, 0.0, 0.0)))}[methods]()
        sim.operations.integrator = azp.Integrator(dt=DT, forces=[plj], methods=[m])
    sim.timestep = timestep
    return sim, nl, plj


def _compression(sim, final=None):
    import azplugins_amd as azp
    from azplugins_amd import update, variant

    final = azp.Box.cube(SHRINK * L0) if final is None else final
    u = update.BoxResize(azp.Periodic(5), variant.box.Interpolate(sim.state.box, final, variant.Ramp(0, 1, 0, 20)))
    sim.operations.add(u)
    return final


def _host(sim):
    st = sim.state
    return dict(pos=st.pos[: st.N].cpu().numpy(), vel=st.vel[: st.N].cpu().numpy(), image=st.image[: st.N].cpu().numpy())


def _fractional(pos, box):
    return box_ref.fractional(pos[:, :3], (box.Lx, box.Ly, box.Lz), (box.xy, box.xz, box.yz))


def _assert_in_box(pos, box):
    f = _fractional(pos, box)
    assert f.min() >= -0.5 - 4 * ULP_HALF and f.max() < 0.5 + 4 * ULP_HALF, (f.min(), f.max())


def _assert_forces_of_a_fresh_simulation(sim, plj, pos=None):
    """The forces of ``sim`` against those of a new simulation made of its positions (or ``pos``) and its box."""
    got = np.array(plj.forces)
    fresh, _, plj2 = _sim(xyz=(_host(sim)["pos"] if pos is None else pos)[:, :3], box=sim.state.box)
    fresh.run(0)
    want = np.array(plj2.forces)
    err, scale = np.abs(got - want).max(), np.abs(want).max()
    print("forces against a fresh simulation: %.3e of the largest force %.3e (tolerance %.0e)" % (err / scale, scale, FORCE_TOL))
    assert np.all(np.isfinite(got)) and scale > 1.0 and err <= FORCE_TOL * scale


def test_resize_during_a_run():
    import azplugins_amd as azp

    sim, nl, plj = _sim()
    final = _compression(sim)
    sim.run(0)
    builds = [nl.num_builds]
    for _ in range(4):  # steps 1-5, 6-10, 11-15, 16-20: the resize opens the last step of each
        sim.run(5)
        builds.append(nl.num_builds)
    assert sim.timestep == 21 and all(b > a for a, b in zip(builds, builds[1:])), builds
    assert sim.state.box == final and sim.state.box_generation == 4
    _assert_in_box(_host(sim)["pos"], final)
    _assert_forces_of_a_fresh_simulation(sim, plj)
    assert azp.Box.cube(SHRINK * L0).Lx > 2.0 * (R_CUT + BUFFER)


def test_constant_box_changes_nothing():
    from azplugins_amd import update, variant

    runs = []
    for with_updater in (False, True):
        sim, nl, plj = _sim()
        if with_updater:
            sim.operations.add(update.BoxResize(5, variant.box.Constant(sim.state.box)))
        sim.run(20)
        runs.append((_host(sim), nl.num_builds, sim.state.box_generation, sim.state.type_generation))
    (a, builds_a, *gen_a), (b, builds_b, *gen_b) = runs
    assert builds_a == builds_b and gen_a == gen_b == [0, 0]
    for k in a:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k


def test_split_runs_are_one_run():
    finals = []
    for runs in ((20,), (8, 12)):
        sim, nl, plj = _sim()
        _compression(sim)
        for n in runs:
            sim.run(n)
        finals.append((_host(sim), np.array(plj.forces), nl.num_builds, sim.state.box))
    (a, fa, builds_a, box_a), (b, fb, builds_b, box_b) = finals
    assert box_a == box_b and builds_a == builds_b
    for k in a:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k
    assert np.array_equal(_bits(fa), _bits(fb))


def test_shear_leaves_fused_mode():
    import azplugins_amd as azp

    sim, nl, plj = _sim()
    final = _compression(sim, final=azp.Box(L0, L0, L0, xy=0.4))
    sim.run(0)
    assert nl.fused_active == plj.takes_plan_from_cells()  # (an untilted box with one tile-kernel consumer: fused)
    sim.run(4)
    assert nl.fused_active == plj.takes_plan_from_cells() and not sim.state.box.is_triclinic
    builds = nl.num_builds
    sim.run(1)  # step 5 opens with the first resize: xy = 0.1
    assert sim.state.box.xy == pytest.approx(0.1, abs=1e-15) and nl.num_builds == builds + 1
    assert not nl.fused_active and nl.has_hoomd_rows
    sim.run(15)
    assert sim.state.box == final and not nl.fused_active
    _assert_in_box(_host(sim)["pos"], final)
    _assert_forces_of_a_fresh_simulation(sim, plj)


@pytest.mark.parametrize("methods", ["nve", "bussi", "langevin", "fire"])
def test_steppers_follow_the_box(methods):
    """A compression by 5 % at step 5 of run(10), run step by step. After every step all particles are inside the box of
    that moment; a particle whose fractional coordinates never jumped (none moves by a tenth of the box in a step, and the
    resize keeps fractional coordinates) crossed no face, so its image counters are still zero, and one that jumped once
    has a counter of +-1. A stepper that kept the box it was started with wraps at the old faces and fails all three."""
    import azplugins_amd as azp
    from azplugins_amd import update, variant

    sim, nl, plj = _sim(methods=methods, timestep=0)
    new = azp.Box.cube(SHRINK * L0)
    sim.operations.add(update.BoxResize(azp.Periodic(10, phase=5), variant.box.Constant(new)))
    sim.run(0)
    f_prev = _fractional(_host(sim)["pos"], sim.state.box)
    jumps = np.zeros(f_prev.shape, dtype=np.int64)
    crossed_after = 0
    for step in range(10):
        sim.run(1)
        assert sim.state.box == (new if step >= 5 else azp.Box.cube(L0))
        h = _host(sim)
        _assert_in_box(h["pos"], sim.state.box)
        f = _fractional(h["pos"], sim.state.box)
        jumps += np.rint(f_prev - f).astype(np.int64)  # (+1: left through the upper face)
        assert np.abs((f - f_prev) - np.rint(f - f_prev)).max() < 0.1
        crossed_after += int(np.rint(f_prev - f).any(axis=1).sum()) if step >= 5 else 0
        f_prev = f
    h = _host(sim)
    np.testing.assert_array_equal(h["image"], jumps)
    stayed = ~jumps.any(axis=1)
    print("%s: %d particles crossed a face, %d crossings after the resize" % (methods, int((~stayed).sum()), crossed_after))
    assert stayed.sum() > 400 and not h["image"][stayed].any()
    assert crossed_after >= 3  # (what the test rests on: particles did pass through the new faces)
    assert sim.state.box_generation == 1 and np.all(np.isfinite(h["pos"]))


def test_recorders_keep_the_volume_of_their_rows():
    """ThermodynamicRecorder and RDFRecorder with Periodic(5) across the compression: every row equals, bit for bit, what
    the computes report in an identical run stopped at that step -- the box there is the box of that step, not the last."""
    from azplugins_amd import compute

    def make(record):
        import azplugins_amd as azp

        sim, nl, plj = _sim()
        _compression(sim)
        thermo = compute.ThermodynamicQuantities(azp.All())
        rdf = compute.RadialDistributionFunction(azp.All(), azp.All(), r_max=3.0, num_bins=30)
        sim.operations.add(thermo)
        sim.operations.add(rdf)
        recs = (compute.ThermodynamicRecorder(thermo, 5), compute.RDFRecorder(rdf, 5)) if record else ()
        for r in recs:
            sim.operations.add(r)
        return sim, thermo, rdf, recs

    sim, _, _, (trec, rrec) = make(True)
    sim.run(20)
    assert trec.timesteps.tolist() == rrec.timesteps.tolist() == [5, 10, 15, 20]
    table, frames, mean = trec.table, rrec.rdf, rrec.mean_rdf
    volumes = [(L0 * (1.0 - s) + SHRINK * L0 * s) ** 3 for s in (0.0, 0.25, 0.5, 0.75)]  # the resize at t follows the row of t
    assert table["volume"] == pytest.approx(volumes, rel=1e-14) and len(set(table["volume"].tolist())) == 4
    ref_sim, thermo, rdf, _ = make(False)
    counts, pairs = [], []
    for row, n in enumerate((4, 5, 5, 5)):
        ref_sim.run(n)
        assert ref_sim.timestep == trec.timesteps[row]
        for name in ("volume", "pressure", "pressure_tensor", "potential_energy", "kinetic_energy"):
            want = np.asarray(getattr(thermo, name))
            got = np.asarray(table[name][row])
            assert got.tobytes() == want.astype(got.dtype).tobytes(), (row, name, got, want)
        assert np.array_equal(_bits(frames[row]), _bits(rdf.rdf)), row
        counts.append(rdf.counts.astype(np.float64) * ref_sim.state.box.volume)
        pairs.append(rdf.num_pairs)
    # the mean over frames of different volumes: each frame's counts with its own volume
    shells = (4.0 * np.pi / 3.0) * np.diff(np.linspace(0.0, 3.0, 31) ** 3)
    assert mean == pytest.approx(np.sum(counts, axis=0) / (sum(pairs) * shells), rel=1e-13)
    assert frames[:, 10:].min() > 0.0


@pytest.mark.parametrize("how", ["update", "assign"])
def test_between_runs(how):
    import azplugins_amd as azp
    from azplugins_amd import update

    xyz, v = _start(shell=True)
    sim, nl, plj = _sim(xyz=xyz, velocity=0.25 * v)  # (at most 0.02 in five steps: the last plane stays 0.05 inside)
    sim.run(5)
    before, builds = _host(sim), nl.num_builds
    # no particle has crossed a face since the list was built (one that has would be a box length from where the list saw
    # it, and the distance check, run in the new box, would ask for a rebuild by accident)
    assert not before["image"].any() and builds == 1
    new = azp.Box.cube(0.97 * L0)
    if how == "update":
        update.BoxResize.update(sim.state, new)
    else:
        sim.state.box = new
    assert sim.state.box == new and sim.state.box_generation == 1
    sim.run(0)
    assert nl.num_builds == builds + 1
    after = _host(sim)
    assert np.array_equal(_bits(after["vel"]), _bits(before["vel"]))
    if how == "update":
        _assert_in_box(after["pos"], new)
        d = _fractional(after["pos"], new) - _fractional(before["pos"], azp.Box.cube(L0))
        assert np.abs(d - np.rint(d)).max() <= BOUND
        _assert_forces_of_a_fresh_simulation(sim, plj)
    else:
        assert np.array_equal(_bits(after["pos"]), _bits(before["pos"])) and np.array_equal(after["image"], before["image"])
        wrapped, _ = ref.multi_wrap(before["pos"][:, :3], None, ((new.Lx, new.Ly, new.Lz), (0.0, 0.0, 0.0), (1, 1, 1)))
        assert np.abs(wrapped - before["pos"][:, :3]).max() > 1.0  # (some particle did lie outside the new box)
        _assert_forces_of_a_fresh_simulation(sim, plj, pos=wrapped)
    sim.run(3)  # and the run goes on in the new box
    _assert_in_box(_host(sim)["pos"], new)


def test_refusals():
    import azplugins_amd as azp
    from azplugins_amd import update, variant

    sim, nl, plj = _sim()
    st = sim.state
    before = _host(sim)
    with pytest.raises(azp.AzpError, match="periodic flags"):
        update.BoxResize.update(st, azp.Box(9.0, periodic=(1, 1, 0)))
    with pytest.raises(azp.AzpError, match="not positive and finite"):
        update.BoxResize.update(st, azp.Box(9.0, 0.0, 9.0))
    with pytest.raises(azp.AzpError, match="does not have"):
        update.BoxResize.update(st, azp.Box(9.0), filter=azp.Type("Z"))
    u = update.BoxResize(1, variant.box.Constant(azp.Box(9.0)))
    sim.operations.add(u)
    sim.domain = object()  # (a stand-in: the updater refuses before it looks at it)
    with pytest.raises(azp.AzpError, match="decomposed"):
        u._update(sim, 0)
    sim.domain = None
    assert st.box == azp.Box.cube(L0) and st.box_generation == 0
    after = _host(sim)
    assert all(np.array_equal(after[k].view(np.int32), before[k].view(np.int32)) for k in before)
