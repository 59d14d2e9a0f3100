"""azplugins_amd.angle on the GPU against the float64 NumPy reference (tests/angle_ref.py). The bound is the project's
FP64 parity bound (tests/test_gpu_parity.py): 1e-10 of the largest component of the array, and every output finite."""

import ctypes as C
import math

import numpy as np
import pytest

import angle_cases as cases
import angle_ref as ref
import azplugins_amd as azp
from azplugins_amd import _lib
from azplugins_amd.state import build_angle_table

pytestmark = pytest.mark.gpu

TOL = 1e-10
POTENTIALS = ("Harmonic", "CosineSquared")


def _close(got, want, what):
    """max |got - want| <= 1e-10 max |want|, all finite; prints the figure."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.all(np.isfinite(got)), what
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    print("%s: max deviation %.3e, largest component %.3e" % (what, err, scale))
    assert err <= TOL * scale, "%s: %g > %g" % (what, err, TOL * scale)


def _sim(name, params, xyz, angles, typeid, box, virial=True, types=None, velocity=None, extra_forces=(), dt=0.0, **snap_kw):
    types = types if types is not None else ["T%d" % t for t in range(len(params))]
    snap = azp.Snapshot.from_arrays(xyz, box, angles=angles, angle_typeid=typeid, angle_types=types, velocity=velocity, **snap_kw)
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(snap)
    sim.operations.tuners.clear()
    f = getattr(azp.angle, name)()
    for t, p in zip(types, params):
        f.params[t] = p
    f.compute_virial = virial
    sim.operations.integrator = azp.Integrator(dt=dt, forces=[f] + list(extra_forces), methods=[azp.ConstantVolume()])
    return sim, f


def _check_against(f, out, what, rows=None):
    rows = slice(None) if rows is None else rows
    _close(f.forces, out["force"][rows], what + " forces")
    _close(f.energies, out["energies"][rows], what + " energies")
    if f.compute_virial:
        for r, label in enumerate(("xx", "xy", "xz", "yy", "yz", "zz")):
            _close(f.virials[:, r], out["virial"][rows, r], "%s virial %s" % (what, label))


# ---------------------------------------------------------------------------------------------------------------------
def test_known_answer_and_across_a_periodic_face():
    """The hand-derived case of tests/test_angle.py through Simulation, then shifted so that a sits across the +x face
    and c across the +y face of the box."""
    want_f = np.array([[0.0, -5.0 * math.pi / 3.0, 0.0], [5.0 * math.pi / 6.0, 5.0 * math.pi / 3.0, 0.0], [-5.0 * math.pi / 6.0, 0.0, 0.0]])
    want_u = 5.0 * (math.pi / 6.0) ** 2
    base = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 2.0, 0.0]])
    shifted = base + np.array([9.5, 9.0, 0.0])
    shifted[0, 0] -= 20.0
    shifted[2, 1] -= 20.0
    assert shifted[0, 0] == -9.5 and shifted[2, 1] == -9.0
    W = np.outer(base[0] - base[1], want_f[0]) + np.outer(base[2] - base[1], want_f[2])   # dab (x) F_a + dcb (x) F_c
    for what, xyz in (("known answer", base), ("known answer across the faces", shifted)):
        sim, f = _sim("Harmonic", [dict(k=10.0, t0=2.0 * math.pi / 3.0)], xyz, [(0, 1, 2)], [0], (20.0, 20.0, 20.0))
        sim.run(0)
        _close(f.forces, want_f, what + " forces")
        _close(f.energies, np.full(3, want_u / 3.0), what + " energies")
        assert abs(f.energy - want_u) <= TOL * want_u
        _close(f.virials.sum(axis=0), np.array([W[0, 0], W[0, 1], W[0, 2], W[1, 1], W[1, 2], W[2, 2]]), what + " virial")


@pytest.mark.parametrize("box", ["cubic", "triclinic"])
@pytest.mark.parametrize("name", POTENTIALS)
def test_parity_system(name, box):
    xyz, angles, typeid, L, tilt = cases.parity_system(box)
    out = cases.parity_reference(name, box)
    sim, f = _sim(name, cases.PARAMS, xyz, angles, typeid, azp.Box(L[0], L[1], L[2], *tilt))
    sim.run(0)
    tab = sim.state.angle_table()
    assert tab["width"] == 15 and int(tab["n_angles"][363]) == 15 and int(tab["n_angles"][4]) == 3
    _check_against(f, out, "%s %s" % (name, box))
    # particles without angles: exact zeros everywhere
    assert not f.forces[364:].any() and not f.energies[364:].any() and not f.virials[364:].any()
    assert np.abs(out["force"]).max() > 10.0 and np.abs(out["virial"]).max() > 10.0


@pytest.mark.parametrize("name", POTENTIALS)
def test_edge_angles(name):
    """theta = pi exactly with t0 = pi and with t0 = 2, theta = 5e-4 (sin theta under the 1e-3 floor: dU/dc is divided
    by the floor, not by sin theta) and theta = 1e-2 (above it)."""
    xyz, angles, typeid, L = cases.edge_system()
    out = ref.evaluate(name, cases.PARAMS_EDGE, xyz, angles, typeid, L)
    sim, f = _sim(name, cases.PARAMS_EDGE, xyz, angles, typeid, L)
    sim.run(0)
    _check_against(f, out, name + " edge angles")
    assert not f.forces[:6].any()            # collinear: no force whatever t0 is
    assert not f.energies[:3].any() and f.energies[3] > 0.0
    if name == "Harmonic":
        # the floor: |F_a| = k (t0 - theta) / 1e-3 * sin(theta) / |dab|, not k (t0 - theta) / |dab|
        th = 5e-4
        assert abs(np.linalg.norm(f.forces[6]) - 10.0 * (2.0 - th) / 1e-3 * math.sin(th)) < 1e-6


def _direct(name, xyz, angles, typeid, L, tilt, n_local, compute_virial=True, block_size=0):
    """The C entry point on a table for the first n_local rows; output buffers span ALL rows and start as NaN."""
    import torch

    n = xyz.shape[0]
    pos = torch.from_numpy(np.ascontiguousarray(np.c_[xyz, np.zeros(n)])).to("cuda:0")   # rows of (x, y, z, w)
    tab = build_angle_table(torch.from_numpy(np.asarray(angles, dtype=np.int64)).to("cuda:0"),
                            torch.from_numpy(np.asarray(typeid, dtype=np.int64)).to("cuda:0"), n_local)
    force = torch.full((n, 4), float("nan"), dtype=torch.float64, device="cuda:0")
    virial = torch.full((6, n), float("nan"), dtype=torch.float64, device="cuda:0")
    pot = getattr(azp.angle, name)()
    params = torch.from_numpy(np.stack([pot._pack(p) for p in cases.PARAMS])).to("cuda:0")
    a = _lib.AngleArgs()
    a.d_force, a.d_virial, a.virial_pitch = force.data_ptr(), virial.data_ptr(), n
    a.N, a.n_max, a.d_pos = n_local, n, pos.data_ptr()
    a.box = _lib.make_box(L, tilt)
    a.d_gpu_anglelist, a.d_gpu_n_angles, a.pitch = tab["table"].data_ptr(), tab["n_angles"].data_ptr(), tab["pitch"]
    a.n_angle_types, a.compute_virial, a.block_size = len(cases.PARAMS), int(compute_virial), block_size
    _lib.check(getattr(_lib.lib(), pot._entry)(C.byref(a), params.data_ptr(), torch.cuda.current_stream().cuda_stream), pot._entry)
    torch.cuda.synchronize()
    return force.cpu().numpy(), virial.cpu().numpy()


@pytest.mark.parametrize("name", POTENTIALS)
def test_ghost_rows(name):
    """The last 60 rows are ghosts: the 307 locals get the whole-system reference (every angle with a local member is
    in their table), and no row from 307 on is written, in the force or in the virial."""
    xyz, angles, typeid, L, tilt = cases.parity_system("cubic")
    out = cases.parity_reference(name, "cubic")
    n_local = 307
    force, virial = _direct(name, xyz, angles, typeid, L, tilt, n_local)
    _close(force[:n_local, :3], out["force"][:n_local], name + " ghost rows: local forces")
    _close(force[:n_local, 3], out["energies"][:n_local], name + " ghost rows: local energies")
    _close(virial[:, :n_local].T, out["virial"][:n_local], name + " ghost rows: local virials")
    assert np.isnan(force[n_local:]).all() and np.isnan(virial[:, n_local:]).all()
    # and through State: ghosts declared by n_local
    snap = azp.Snapshot.from_arrays(xyz, L, angles=angles, angle_typeid=typeid, angle_types=["T0", "T1"])
    st = azp.State(snap, "cuda:0", n_local=n_local)
    assert st.N == n_local and st.n_ghost == 60 and st.angle_table()["table"].shape[1] == n_local


def test_empty_topology():
    xyz = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    snap = azp.Snapshot.from_arrays(xyz, (10.0, 10.0, 10.0))
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(snap)
    f = azp.angle.Harmonic()
    f.compute_virial = True
    sim.operations.integrator = azp.Integrator(dt=0.0, forces=[f])
    sim.run(0)
    assert sim.state.n_angles == 0
    assert f.forces.shape == (3, 3) and not f.forces.any() and not f.energies.any() and not f.virials.any()


@pytest.mark.parametrize("name", POTENTIALS)
def test_deterministic_and_block_sizes(name):
    """Two compute() calls leave the same bits, and so do block sizes 64, 128 and 256 (one lane per particle sums its
    entries in table order whatever the block is)."""
    xyz, angles, typeid, L, tilt = cases.parity_system("triclinic")
    sim, f = _sim(name, cases.PARAMS, xyz, angles, typeid, azp.Box(L[0], L[1], L[2], *tilt))
    sim.run(0)
    first = (f.force_tensor.clone(), f._virial.clone())
    f.compute(0)
    assert (f.force_tensor == first[0]).all() and (f._virial == first[1]).all()
    for bs in (64, 128, 256):
        f.block_size = bs
        f.force_tensor.fill_(float("nan"))
        f.compute(0)
        assert _lib.last_launch()["block_size"] == bs
        assert (f.force_tensor == first[0]).all() and (f._virial == first[1]).all(), bs
    f.block_size = 96
    with pytest.raises(azp.AzpError):
        f.compute(0)


@pytest.mark.parametrize("name", POTENTIALS)
def test_sorter_reindexes_angles(name):
    xyz, angles, typeid, L, tilt = cases.parity_system("cubic")
    out = cases.parity_reference(name, "cubic")
    sim, f = _sim(name, cases.PARAMS, xyz, angles, typeid, L)
    sim.run(0)
    order = azp.ParticleSorter(particles_per_block=16).sort(sim).cpu().numpy()
    assert (order != np.arange(order.size)).sum() > 300      # the sort did move the particles
    f.compute(0)
    tag = sim.state.tag.cpu().numpy().view(np.uint32).astype(np.int64)
    assert np.array_equal(tag, order)
    assert np.array_equal(tag[sim.state.angle_group.astype(np.int64)], angles)   # the members by tag are what they were
    got = dict(force=np.zeros((order.size, 3)), energies=np.zeros(order.size), virial=np.zeros((order.size, 6)))
    got["force"][tag], got["energies"][tag], got["virial"][tag] = f.forces, f.energies, f.virials
    _close(got["force"], out["force"], name + " after the sort: forces by tag")
    _close(got["energies"], out["energies"], name + " after the sort: energies by tag")
    _close(got["virial"], out["virial"], name + " after the sort: virials by tag")


# ---------------------------------------------------------------------------------------------------------------------
# in a run
# ---------------------------------------------------------------------------------------------------------------------
BOND_PARAMS = dict(r_0=1.0, r_1=1.5, U_1=1.0, U_tilt=0.5)
NVE_STEPS, NVE_DT = 20, 0.002
# worst position deviation of the same 20-step comparison with the DoubleWell bonds ALONE, nve_deviation(oracle, False),
# measured on the MI355X (three runs, the same figure; the bond and NVE kernels are those of the parent commit), times 10
NVE_BONDS_ONLY_DEVIATION = 4.440892e-16
NVE_BOUND = 10.0 * NVE_BONDS_ONLY_DEVIATION


def nve_deviation(oracle, with_angles):
    """20 velocity-Verlet steps of the 40 chains of the parity system (DoubleWell bonds, optionally Harmonic angles) on
    the GPU and in NumPy (bond forces from the oracle, angle forces from angle_ref): worst position deviation."""
    xyz, angles, typeid, L, tilt = cases.parity_system("cubic")
    n = cases.N_CHAINS * cases.CHAIN_LEN
    xyz, angles, typeid = xyz[:n], angles[:cases.N_CHAINS * (cases.CHAIN_LEN - 2)], typeid[:cases.N_CHAINS * (cases.CHAIN_LEN - 2)]
    bonds = cases.chain_bonds()
    vel0 = np.random.default_rng(5).normal(size=(n, 3)) * 0.5
    vel0 -= vel0.mean(axis=0)
    snap = azp.Snapshot.from_arrays(xyz, L, velocity=vel0, bonds=bonds, angles=angles, angle_typeid=typeid, angle_types=["T0", "T1"])
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(snap)
    sim.operations.tuners.clear()
    dw = azp.bond.DoubleWell()
    dw.params["A-A"] = BOND_PARAMS
    forces = [dw]
    if with_angles:
        ha = azp.angle.Harmonic()
        ha.params["T0"], ha.params["T1"] = cases.PARAMS
        forces.append(ha)
    sim.operations.integrator = azp.Integrator(dt=NVE_DT, forces=forces, methods=[azp.ConstantVolume()])
    sim.run(NVE_STEPS)
    got = sim.state.pos[:, :3].cpu().numpy()

    box = oracle.make_box(L)
    bp = oracle.pack_bond_params("DoubleWell", BOND_PARAMS)
    btype = np.zeros(len(bonds), dtype=np.uint32)

    def force(x):
        fb, bad = oracle.bond_forces("DoubleWell", np.c_[x, np.zeros(n)], box, bonds, btype, bp)
        assert bad == 0
        f = fb[:, :3].copy()
        if with_angles:
            f += ref.evaluate("Harmonic", cases.PARAMS, x, angles, typeid, L)["force"]
        return f

    x, v = xyz.copy(), vel0.copy()   # unit masses; positions are left unwrapped, the comparison takes the minimum image
    f = force(x)
    for _ in range(NVE_STEPS):
        v += 0.5 * NVE_DT * f
        x += NVE_DT * v
        f = force(x)
        v += 0.5 * NVE_DT * f
    d = got - x
    d -= np.asarray(L) * np.round(d / np.asarray(L))
    assert np.all(np.isfinite(got)) and np.abs(x - xyz).max() > 1e-3     # the particles did move
    return float(np.abs(d).max())


def test_nve_run_with_bonds_and_angles(oracle):
    """20 NVE steps, dt = 0.002, chains with DoubleWell bonds and Harmonic angles, against the NumPy velocity-Verlet.
    The bound is 10 x the worst position deviation of the same comparison with the bonds alone (angles add one more
    rounding-level force per step). Measured on the MI355X: bonds alone 4.44e-16 (half an ulp of a coordinate between
    2 and 4), so the bound is 4.44e-15; bonds + angles 8.88e-16."""
    dev = nve_deviation(oracle, with_angles=True)
    print("NVE, bonds + angles: worst position deviation %.3e (bound %.3e)" % (dev, NVE_BOUND))
    assert dev <= NVE_BOUND


@pytest.mark.parametrize("name", POTENTIALS)
def test_thermo_picks_up_energy_and_virial(name):
    """ThermodynamicQuantities with the angle force alone: the potential energy and the pressure equal the reference's
    sums to 1e-10 relative. An angle potential depends on directions only, so the trace of its virial is zero by
    Euler's theorem (sum_k r_k . F_k = 0) and the scalar pressure holds the kinetic part alone; the particles are given
    velocities for that reason, and the six components of the pressure tensor, where the angle virial does not cancel,
    are held to 1e-10 of the largest of them as well."""
    from azplugins_amd import compute

    xyz, angles, typeid, L, tilt = cases.parity_system("cubic")
    out = cases.parity_reference(name, "cubic")
    vel = np.random.default_rng(9).normal(size=xyz.shape)
    sim, f = _sim(name, cases.PARAMS, xyz, angles, typeid, L, virial=False, velocity=vel)
    thermo = compute.ThermodynamicQuantities(azp.All())
    sim.operations.add(thermo)
    sim.run(0)
    assert f.compute_virial   # the compute turned it on
    volume = L[0] * L[1] * L[2]
    rows = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    K = np.array([(vel[:, r] * vel[:, c]).sum() for r, c in rows])   # unit masses
    W = out["virial"].sum(axis=0)
    want_tensor = (K + W) / volume
    want_p = (want_tensor[0] + want_tensor[3] + want_tensor[5]) / 3.0
    assert abs(W[0] + W[3] + W[5]) < 1e-10 * np.abs(W).max() and np.abs(W).max() > 0.1 * np.abs(K).max()
    print("%s: U %.15g vs %.15g, P %.15g vs %.15g" % (name, thermo.potential_energy, out["energy"], thermo.pressure, want_p))
    assert abs(thermo.potential_energy - out["energy"]) <= TOL * abs(out["energy"])
    assert abs(thermo.pressure - want_p) <= TOL * abs(want_p)
    _close(np.array(thermo.pressure_tensor), want_tensor, name + " pressure tensor")


@pytest.mark.parametrize("method", ["langevin", "brownian"])
def test_runs_under_the_flow_methods(method):
    """The angle force in Integrator.forces under flow.Langevin and flow.Brownian: the run goes through and stays
    finite (the integration itself is pinned in tests/test_gpu_flow.py)."""
    from azplugins_amd import flow

    xyz, angles, typeid, L, tilt = cases.parity_system("cubic")
    sim, f = _sim("Harmonic", cases.PARAMS, xyz, angles, typeid, L, virial=False)
    field = flow.ConstantFlow(velocity=(0.0, 0.0, 0.0))
    cls = flow.Langevin if method == "langevin" else flow.Brownian
    m = cls(filter=azp.All(), kT=1.0, flow_field=field)
    m.gamma["A"] = 1.0
    sim.operations.integrator = azp.Integrator(dt=0.001, forces=[f], methods=[m])
    sim.run(5)
    assert np.all(np.isfinite(sim.state.pos.cpu().numpy())) and np.all(np.isfinite(f.forces)) and np.abs(f.forces).max() > 0.0
