"""compute.ThermodynamicField on the GPU (csrc/thermo_field.hip): every word of the row against the numpy
restatement ``thermo_field_ref`` bit for bit, the row under reads and reorderings, the existing computes on the same
state, the forces' virials and energies per bin, the in-run recorder and the refusals of the C ABI.

Bounds. A sum of this compute differs from the exact sum of its (rounded) terms by at most
``thermo_field_ref.bound`` = (6 L + F + 1) 2^-53 sum|term| (L tree levels, F forces); ThermodynamicQuantities
documents 256 x 2^-53 sum|term| (thermo_ref.REL_BOUND); the velocity field adds its four-wave, chunked sums in at most
as many additions as thermo's reduction, so the same 256 x 2^-53 is used for it."""

import ctypes as C

import numpy as np
import pytest

import thermo_field_ref as ref
import thermo_ref

import azplugins_amd as azp
from azplugins_amd import _lib, compute
from azplugins_amd import synthetic as syn

pytestmark = pytest.mark.gpu

TYPE_NAMES = ("A", "B", "C")  # (no particle is of type C)
CUBE = ((8.0, 8.0, 8.0), (0.0, 0.0, 0.0))      # the boxes of tests/test_gpu_displacement.py
TILTED = ((9.0, 10.0, 11.0), (0.3, -0.2, 0.4))
BOXES = {"cube": CUBE, "tilted": TILTED}
FIELDS = {"cartesian": compute.CartesianThermodynamicField, "cylindrical": compute.CylindricalThermodynamicField}
CODES = {"cartesian": ref.CARTESIAN, "cylindrical": ref.CYLINDRICAL}
U = 2.0**-53


def _box(box):
    (Lx, Ly, Lz), (xy, xz, yz) = box
    return azp.Box(Lx, Ly, Lz, xy, xz, yz)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _particles(n, box, seed):
    """Positions strictly inside the box (fractional coordinates within +-0.49: the kernels' wrap moves nothing),
    velocities with a drift, masses, types 0 / 1 and randomly permuted tags."""
    rng = np.random.default_rng(seed)
    (Lx, Ly, Lz), (xy, xz, yz) = box
    f = rng.uniform(-0.49, 0.49, size=(n, 3))
    h = np.array([[Lx, xy * Ly, xz * Lz], [0.0, Ly, yz * Lz], [0.0, 0.0, Lz]])
    pos = f @ h.T
    vel = rng.normal(size=(n, 3)) + np.array([0.7, -0.4, 0.2])
    mass = rng.uniform(0.5, 2.0, size=n)
    return pos, vel, mass, rng.integers(0, 2, size=n), rng.permutation(n)


class _System:
    """A state whose row i holds the particle data given for row i and carries tag ``tags[i]``."""

    def __init__(self, box, pos, vel, mass, types, tags):
        import torch

        n = len(pos)
        snap = azp.Snapshot.from_arrays(np.ascontiguousarray(pos), _box(box), typeid=np.asarray(types), types=TYPE_NAMES,
                                        velocity=np.ascontiguousarray(vel))
        snap.particles.mass[:] = mass
        self.sim = sim = azp.Simulation(device="cuda:0", seed=1)
        sim.create_state_from_snapshot(snap)
        st = sim.state
        st.tag[:n] = torch.from_numpy(np.asarray(tags, dtype=np.int32)).to(st.device)
        st.order_generation += 1
        self.pos, self.tags, self.types = np.asarray(pos), np.asarray(tags), np.asarray(types)
        self.vel4 = np.concatenate([vel, np.asarray(mass)[:, None]], axis=1)

    def add(self, c):
        self.sim.operations.computes.append(c)
        return c

    def want(self, kind, num_bins, lower, upper, member=None):
        b = ref.bins(self.pos, CODES[kind], num_bins, lower, upper)
        n_bins = int(np.prod([k for k in num_bins if k > 0], dtype=np.int64))
        return ref.row(b, self.tags, member, ref.terms(self.vel4), self.types, len(TYPE_NAMES), n_bins), b


def _flat(field):
    s = field.sums
    return s.reshape(-1, s.shape[-1])


# ---------------------------------------------------------------------------------------------------------------------
# 1. bit for bit against the restatement
# ---------------------------------------------------------------------------------------------------------------------
ONE_BIN = {"cartesian": ((0, 0, 0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), "cylindrical": ((1, 0, 0), (0.0, 0.0, 0.0), (100.0, 0.0, 0.0))}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
@pytest.mark.parametrize("box_name", sorted(BOXES))
@pytest.mark.parametrize("kind", sorted(FIELDS))
def test_one_bin_at_the_level_boundaries(kind, box_name, n):
    s = _System(BOXES[box_name], *_particles(n, BOXES[box_name], 100 + n))
    grid = ONE_BIN[kind]
    field = s.add(FIELDS[kind](*grid))
    got = _flat(field)
    want, b = s.want(kind, *grid)
    assert (b == 0).all() and got.shape == (1, 21)
    assert np.array_equal(_bits(got), _bits(want))
    assert got[0, 0] == n and field.num_particles.reshape(-1).tolist() == [n]
    assert field.counts.reshape(-1).tolist() == [int((s.types == t).sum()) for t in range(3)]


GRID = {"cartesian": ((7, 5, 3), (-3.5, -2.0, -3.0), (3.5, 3.0, 1.5)),
        "cylindrical": ((7, 5, 3), (0.5, 0.0, -3.0), (3.5, 2.0 * np.pi, 1.5))}


def _edge_system(kind, box_name, n=300, seed=7):
    box = BOXES[box_name]
    pos, vel, mass, types, tags = _particles(n, box, seed)
    lo, hi = np.array(GRID[kind][1]), np.array(GRID[kind][2])
    # particles exactly on bin edges, on the lower bound (counted) and on the upper bound (excluded)
    if kind == "cartesian":
        pos[0] = (lo[0], 0.1, 0.2)
        pos[1] = (hi[0], 0.1, 0.2)
        pos[2] = (-1.5, lo[1], -1.5)
        pos[3] = (0.5, 1.0, hi[2])
        pos[4] = (lo[0] + 3.0, lo[1] + 2.0, lo[2] + 1.5)
        pos[5] = (0.0, hi[1], 0.0)
    else:
        # (y = 0, x > 0: theta = 0 and r = x exactly)
        pos[0] = (lo[0], 0.0, 0.2)
        pos[1] = (hi[0], 0.0, 0.2)
        pos[2] = (1.0, 0.0, lo[2])
        pos[3] = (1.5, 0.0, hi[2])
        pos[4] = (0.25, 0.0, 0.0)  # inside the inner bound
        pos[5] = (2.0, 0.0, -1.5)
    return _System(box, pos, vel, mass, types, tags)


@pytest.mark.parametrize("box_name", sorted(BOXES))
@pytest.mark.parametrize("kind", sorted(FIELDS))
def test_field_with_edges_empty_bins_and_filters(kind, box_name):
    s = _edge_system(kind, box_name)
    grid = GRID[kind]
    fields = {"all": s.add(FIELDS[kind](*grid)), "a": s.add(FIELDS[kind](*grid, filter=azp.Type(["A"]))),
              "none": s.add(FIELDS[kind](*grid, filter=azp.Type(["C"])))}
    members = {"all": None, "a": s.types == 0, "none": np.zeros(len(s.types), dtype=bool)}
    for name, field in fields.items():
        want, b = s.want(kind, *grid, member=members[name])
        got = _flat(field)
        assert got.shape == (105, 21) and field.sums.shape == (7, 5, 3, 21)
        assert np.array_equal(_bits(got), _bits(want)), name
    want, b = s.want(kind, *grid)
    assert b[0] >= 0 and b[1] == -1 and b[3] == -1 and (b == -1).sum() > 100  # (edges, the upper bound, outside)
    assert (want[:, 0] == 0).any() and (want[:, 0] > 1).any()  # (empty bins and shared ones)
    assert b[2] >= 0 and (b[5] == -1 if kind == "cartesian" else b[5] >= 0)
    assert not _bits(_flat(fields["none"])).any()  # (+0.0 in every word)
    assert fields["a"].counts[..., 1].sum() == 0 and fields["a"].counts[..., 0].sum() == ((b >= 0) & (s.types == 0)).sum()
    assert fields["all"].counts.dtype == np.int64 and fields["all"].counts.sum() == (b >= 0).sum()


@pytest.mark.parametrize("kind", sorted(FIELDS))
def test_more_bins_than_particles(kind):
    s = _System(TILTED, *_particles(500, TILTED, 9))
    grid = ((20, 20, 20), (-4.0, -4.0, -4.0), (4.0, 4.0, 4.0)) if kind == "cartesian" else ((20, 20, 20), (0.0, 0.0, -4.0), (4.0, 2.0 * np.pi, 4.0))
    field = s.add(FIELDS[kind](*grid))
    want, b = s.want(kind, *grid)
    got = _flat(field)
    assert got.shape == (8000, 21) and np.array_equal(_bits(got), _bits(want))
    assert 100 < (want[:, 0] > 0).sum() < 500


# ---------------------------------------------------------------------------------------------------------------------
# 2. bit-identical under reads and reordering
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(FIELDS))
def test_reads_and_reorderings_change_no_bit(kind):
    import torch

    s = _System(TILTED, *_particles(3000, TILTED, 11))
    coarse = ((2, 0, 2), (-4.0 if kind == "cartesian" else 0.0, 0.0, -5.0), (4.0, 0.0, 5.0))  # (bins of several runs of 64)
    grids = [ONE_BIN[kind], GRID[kind], coarse]
    fields = [s.add(FIELDS[kind](*g)) for g in grids]
    first = [_flat(f).copy() for f in fields]
    for f, a in zip(fields, first):
        assert np.array_equal(_bits(a), _bits(_flat(f)))
    st = s.sim.state
    n = st.N
    # any permutation of the rows that carries the tags
    perm = torch.from_numpy(np.random.default_rng(12).permutation(n)).to(st.device)
    for name in ("pos", "vel", "tag", "image"):
        a = getattr(st, name)
        a[:n] = a[:n].index_select(0, perm)
    st.position_generation += 1
    st.order_generation += 1
    for f, a in zip(fields, first):
        assert np.array_equal(_bits(a), _bits(_flat(f)))
    tag0 = st.tag[:n].cpu().numpy().copy()
    azp.ParticleSorter(particles_per_block=16).sort(s.sim)
    assert not np.array_equal(st.tag[:n].cpu().numpy(), tag0)
    for f, a in zip(fields, first):
        assert np.array_equal(_bits(a), _bits(_flat(f)))
    assert first[0][0, 0] == n and (first[1][:, 0] > 0).sum() > 50 and (first[2][:, 0] > 128).all()


# ---------------------------------------------------------------------------------------------------------------------
# 3. against the existing computes on the same state
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(FIELDS))
def test_velocities_against_the_velocity_field(kind):
    s = _System(TILTED, *_particles(3000, TILTED, 13))
    grid = GRID[kind]
    field = s.add(FIELDS[kind](*grid))
    vf_cls = compute.CartesianVelocityFieldCompute if kind == "cartesian" else compute.CylindricalVelocityFieldCompute
    vf = s.add(vf_cls(*grid, filter=azp.All()))
    got, want = field.velocities, vf.velocities
    assert got.shape == want.shape == (7, 5, 3, 3)
    if kind == "cylindrical":
        # (the local-basis velocity is the velocity field's own kernel: the same words)
        assert np.array_equal(_bits(got), _bits(want))
        return
    b = ref.bins(s.pos, CODES[kind], *grid)
    p = np.abs(s.vel4[:, 3:4] * s.vel4[:, :3])
    for k in range(105):
        sel = b == k
        if not sel.any():
            assert not got.reshape(105, 3)[k].any()
            continue
        m = s.vel4[sel, 3].sum()
        # |P / M - P' / M'| <= (e_P + |v| e_M) / M to first order, each compute with its own bound on its sums
        e_tree = ref.bound(1.0, int(sel.sum()), 0)
        e_sum = e_tree + thermo_ref.REL_BOUND
        tol = e_sum * (p[sel].sum(axis=0) / m + np.abs(want.reshape(105, 3)[k])) * 1.01 + 4 * U * np.abs(want.reshape(105, 3)[k])
        err = np.abs(got.reshape(105, 3)[k] - want.reshape(105, 3)[k])
        assert (err <= tol).all(), (k, err, tol)


def test_one_bin_against_thermodynamic_quantities():
    s = _System(TILTED, *_particles(3000, TILTED, 14))
    field = s.add(compute.CartesianThermodynamicField((0, 0, 0), (0, 0, 0), (0, 0, 0), filter=azp.Type(["A"])))
    thermo = s.add(compute.ThermodynamicQuantities(azp.Type(["A"])))
    row = _flat(field)[0]
    sums = thermo._sums().cpu().numpy()[0]
    sel = s.types == 0
    mag = np.abs(ref.terms(s.vel4[sel])).sum(axis=0)
    assert row[0] == sums[0] == sel.sum() and row[18:].tolist() == [sel.sum(), 0, 0]
    # slots 2-17 of the field are thermo's 1-16 (thermo has no mass slot)
    for mine, theirs in zip(range(2, 18), range(1, 17)):
        tol = (ref.bound(mag[mine], int(sel.sum()), 0) + thermo_ref.REL_BOUND * mag[mine])
        assert abs(row[mine] - sums[theirs]) <= tol, (mine, row[mine], sums[theirs], tol)
    assert abs(row[1] - s.vel4[sel, 3].sum()) <= ref.bound(mag[1], int(sel.sum()), 0) + 4 * U * mag[1]
    assert np.array_equal(row[11:18], np.zeros(7))  # (no forces)


# ---------------------------------------------------------------------------------------------------------------------
# 4. with forces
# ---------------------------------------------------------------------------------------------------------------------
def _velocities(n, seed, kT=1.0):
    tag = np.arange(n, dtype=np.uint64)
    v = np.stack([syn.normal(seed, tag, c) for c in range(3)], axis=1) * np.sqrt(kT)
    return v - v.mean(axis=0)


def _liquid(bonded, seed=1):
    """N = 512 PerturbedLJ liquid (FCC 8 x 4 x 4 cells at rho* = 0.8), optionally with DoubleWell bonds (a second force)."""
    cfg = syn.config_north_star(ncell=(8, 4, 4))
    n = cfg["xyz"].shape[0]
    assert n == 512
    bonds = np.stack([np.arange(0, n, 4), np.arange(1, n, 4)], axis=1).astype(np.uint32) if bonded else None
    snap = azp.Snapshot.from_arrays(cfg["xyz"], cfg["L"], velocity=_velocities(n, 91), bonds=bonds)
    snap.particles.mass[:] = 0.5 + 1.5 * syn.u01(82, np.arange(n, dtype=np.uint64), 0)
    sim = azp.Simulation(device="cuda:0", seed=seed)
    sim.create_state_from_snapshot(snap)
    plj = azp.pair.PerturbedLennardJones(nlist=azp.nlist.Cell(buffer=0.3), default_r_cut=cfg["r_cut"], mode="shift")
    plj.params[("A", "A")] = cfg["params"]
    forces = [plj]
    if bonded:
        dw = azp.bond.DoubleWell()
        dw.params["A-A"] = dict(r_0=1.0, r_1=1.5, U_1=1.0, U_tilt=0.5)
        forces.append(dw)
    sim.operations.integrator = azp.Integrator(dt=0.004, forces=forces, methods=[azp.ConstantVolume()])
    return sim, cfg


def _tiling(cfg, num_bins=(4, 0, 3)):
    L = cfg["L"]
    return num_bins, tuple(-0.5 * float(x) for x in L), tuple(0.5 * float(x) for x in L)


@pytest.mark.parametrize("bonded", [False, True])
def test_virials_and_energies_per_bin(bonded):
    sim, cfg = _liquid(bonded)
    forces = sim.operations.integrator.forces
    grid = _tiling(cfg)
    field = compute.CartesianThermodynamicField(*grid, streaming="keep")
    sim.operations.add(field)
    assert all(not f.compute_virial for f in forces)
    with pytest.raises(azp.AzpError, match=r"sim\.run\(0\)"):
        field.potential_energy_density
    sim.run(0)
    assert all(f.compute_virial for f in forces)  # (the field turned the virial pass on)
    st = sim.state
    n = st.N
    pos, vel4 = st.pos[:n, :3].cpu().numpy(), st.vel[:n].cpu().numpy()
    tags = st.tag[:n].cpu().numpy().view(np.uint32).astype(np.int64)
    f_arr = [f._force[:n].cpu().numpy() for f in forces]
    v_arr = [f._virial.cpu().numpy() for f in forces]
    b = ref.bins(pos, ref.CARTESIAN, *grid)
    assert (b >= 0).all()  # (the field tiles the box)
    want = ref.row(b, tags, None, ref.terms(vel4, f_arr, v_arr), np.zeros(n, dtype=np.int64), 1, 12)
    got = _flat(field)
    assert got.shape == (12, 19) and np.array_equal(_bits(got), _bits(want))
    assert np.abs(got[:, 11:17]).min(axis=0).max() > 0.0 and (got[:, 17] != 0.0).all()
    # summed over a field that tiles the box, pressure x volume is the whole system's
    thermo = compute.ThermodynamicQuantities(azp.All())
    sim.operations.add(thermo)
    p_field = (field.pressure_tensor * field.bin_volumes[..., None]).reshape(12, 6).sum(axis=0)
    p_box = np.array(thermo.pressure_tensor) * st.box.volume
    mag = np.abs(ref.terms(vel4, f_arr, v_arr)).sum(axis=0)
    mag_w = sum(np.abs(v).sum(axis=1) for v in v_arr)
    for c in range(6):
        m = mag[5 + c] + mag_w[c]
        # the tree's bound + thermo's + the 12 x 2 roundings of dividing by V_bin, multiplying back and adding the bins
        tol = (ref.bound(1.0, n, len(forces)) + thermo_ref.REL_BOUND + 40 * U) * m
        assert abs(p_field[c] - p_box[c]) <= tol, (c, p_field[c], p_box[c], tol)
    assert field.bin_volumes.sum() == pytest.approx(st.box.volume, rel=1e-14)
    assert field.pressure.shape == (4, 3) and np.isfinite(field.kinetic_temperature).all()
    # a force evaluated without virials: the pressure is refused, the energies are not
    forces[0].compute_virial = False
    sim.operations.remove(field)
    sim.operations.remove(thermo)
    sim.run(0)
    sim.operations.add(field)
    with pytest.raises(azp.AzpError, match="without virials"):
        field.pressure
    with pytest.raises(azp.AzpError, match="without virials"):
        field.pressure_tensor
    assert np.isfinite(field.potential_energy_density).all()


def test_cylindrical_field_without_r_binning_refuses_volumes():
    s = _System(CUBE, *_particles(200, CUBE, 15))
    field = s.add(compute.CylindricalThermodynamicField((0, 4, 0), (0.0, 0.0, 0.0), (0.0, 2.0 * np.pi, 0.0)))
    assert field.counts.sum() == 200 and field.kinetic_temperature.shape == (4,)
    for name in ("bin_volumes", "number_density", "mass_density", "pressure", "potential_energy_density"):
        with pytest.raises(azp.AzpError, match="r coordinate"):
            getattr(field, name)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the recorder
# ---------------------------------------------------------------------------------------------------------------------
def _final(sim):
    st = sim.state
    order = np.argsort(st.tag[: st.N].cpu().numpy().view(np.uint32))
    return st.pos[: st.N].cpu().numpy()[order], st.vel[: st.N].cpu().numpy()[order]


def test_recorder_in_a_run():
    plain, cfg = _liquid(False)
    plain.run(20)
    grid = _tiling(cfg, (4, 0, 2))
    sim, _ = _liquid(False)
    field = compute.CartesianThermodynamicField(*grid)
    rec = compute.ThermodynamicFieldRecorder(field, 5)
    sim.operations.add(field)
    sim.operations.writers.append(rec)
    sim.run(20)
    for a, b in zip(_final(plain), _final(sim)):
        assert np.array_equal(_bits(a), _bits(b))  # (the virial pass and the recorder change no bit of the trajectory)
    assert rec.timesteps.tolist() == [5, 10, 15, 20]
    table = rec.table
    assert table["sums"].shape == (4, 4, 2, 19) and table["pressure_tensor"].shape == (4, 4, 2, 6) and table["counts"].shape == (4, 4, 2, 1)
    twin, _ = _liquid(False)
    twin_field = compute.CartesianThermodynamicField(*grid)
    twin.operations.add(twin_field)
    for k in range(4):
        twin.run(5)
        assert np.array_equal(_bits(table["sums"][k]), _bits(twin_field.sums)), k
        assert np.array_equal(_bits(table["pressure"][k]), _bits(twin_field.pressure))
        assert np.array_equal(_bits(table["kinetic_temperature"][k]), _bits(twin_field.kinetic_temperature))
    mean = rec.mean()
    want = compute.thermo_field_quantities(table["sums"].reshape(4, 8, 19).sum(axis=0), np.repeat(field.bin_volumes.reshape(1, 8), 4, axis=0).sum(axis=0), "subtract")
    for name, value in want.items():
        assert np.array_equal(mean[name].reshape(value.shape), value), name
    assert mean["num_particles"].sum() == 4 * 512
    # a width change with rows recorded is refused; reset() forgets
    field.num_bins = (4, 0, 3)
    with pytest.raises(azp.AzpError, match="reset"):
        rec._record(sim, 25)
    rec.reset()
    assert rec.timesteps.size == 0 and rec.table == {}
    sim.run(5)
    assert rec.timesteps.size == 1 and rec.table["sums"].shape == (1, 4, 3, 19)


def test_recorder_normalises_each_row_with_its_own_volume():
    sim, cfg = _liquid(False)
    L = [float(x) for x in cfg["L"]]
    grid = ((0, 0, 2), (0.0, 0.0, -1.0), (0.0, 0.0, 1.0))
    field = compute.CartesianThermodynamicField(*grid)
    rec = compute.ThermodynamicFieldRecorder(field, 2)
    sim.operations.add(field)
    sim.operations.writers.append(rec)
    sim.operations.updaters.append(azp.update.BoxResize(azp.Periodic(1), lambda t: azp.Box(L[0] * (1.0 + 0.002 * t), L[1], L[2])))
    sim.run(6)
    assert rec.timesteps.tolist() == [2, 4, 6]
    table = rec.table
    # (the row of timestep t is recorded before the updater of that step runs: the box of t - 1)
    want = [(L[0] * (1.0 + 0.002 * (t - 1))) * L[1] * 1.0 for t in (2, 4, 6)]
    np.testing.assert_allclose(table["bin_volumes"], np.repeat(np.array(want)[:, None], 2, axis=1), rtol=1e-14)
    assert np.array_equal(table["mass_density"], table["sums"][..., 1] / table["bin_volumes"])
    assert len(set(table["bin_volumes"][:, 0].tolist())) == 3


# ---------------------------------------------------------------------------------------------------------------------
# 6. the refusals of the C ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_errors_through_the_abi():
    import torch

    dev = torch.device("cuda:0")
    n = 100
    pos = torch.zeros((n, 4), dtype=torch.float64, device=dev)
    vel = torch.ones((n, 4), dtype=torch.float64, device=dev)
    tag = torch.arange(n, dtype=torch.int32, device=dev)
    keys = torch.zeros(n, dtype=torch.int64, device=dev)
    out = torch.full((8 * 19 + 1,), 7.0, dtype=torch.float64, device=dev)
    lib = _lib.lib()
    stream = _lib.raw_stream(dev)

    def args(num_bins=(2, 2, 2)):
        a = _lib.ThermoFieldArgs()
        a.d_pos, a.d_vel, a.d_tag, a.d_keys = pos.data_ptr(), vel.data_ptr(), tag.data_ptr(), keys.data_ptr()
        a.N, a.ntypes, a.coordinates = n, 1, _lib.COORDINATES_CARTESIAN
        a.box = _lib.make_box(8.0)
        for d in range(3):
            a.num_bins[d], a.lower[d], a.upper[d] = num_bins[d], -4.0, 4.0
        a.d_out = out.data_ptr()
        return a

    need = C.c_uint64(0)
    a = args()
    assert lib.azp_thermo_field_scratch_size(C.byref(a), C.byref(need)) == 0 and need.value > 0
    scratch = torch.zeros(need.value, dtype=torch.uint8, device=dev)

    def run(a, scratch_bytes):
        a.d_scratch, a.scratch_bytes = scratch.data_ptr(), scratch_bytes
        rc = lib.azp_thermo_field_keys(C.byref(a), stream)
        if rc != 0:
            return rc
        skeys, order = torch.sort(keys)
        a.d_sorted_keys, a.d_order = skeys.data_ptr(), order.data_ptr()
        rc = lib.azp_thermo_field_sums(C.byref(a), stream)
        torch.cuda.synchronize()
        return rc

    too_many = args((2048, 2048, 2048))
    assert lib.azp_thermo_field_scratch_size(C.byref(too_many), C.byref(need)) == -4  # AZP_ERROR_TOO_MANY_BINS
    assert run(too_many, scratch.numel()) == -4
    assert run(args(), scratch.numel() - 1) == -1  # a scratch one byte short
    nine = args()
    nine.n_forces = 9
    assert run(nine, scratch.numel()) == -1
    bad = args()
    bad.upper[1] = -4.0
    assert run(bad, scratch.numel()) == -1
    assert (out.cpu().numpy() == 7.0).all()  # (nothing was written)
    assert run(args(), scratch.numel()) == 0
    got = out.cpu().numpy()
    assert got[-1] == 7.0 and got[:-1].reshape(8, 19)[:, 0].sum() == n  # (all at the origin: one bin)
    assert got[:-1].reshape(8, 19)[7].tolist()[:2] == [n, n]
