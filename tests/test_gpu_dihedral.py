"""azplugins_amd.dihedral on the GPU against the float64 NumPy reference (tests/dihedral_ref.py). The bound is the
project's FP64 parity bound (tests/test_gpu_parity.py): 1e-10 of the largest component of the array, and every output
finite."""

import ctypes as C
import math

import numpy as np
import pytest

import angle_ref
import dihedral_cases as cases
import dihedral_ref as ref
import azplugins_amd as azp
from azplugins_amd import _lib
from azplugins_amd.state import build_dihedral_table

pytestmark = pytest.mark.gpu

TOL = 1e-10
POTENTIALS = ("Periodic", "OPLS")
BATCH = 3   # csrc/dihedral_forces.hip: table entries past the third go through the kernel's tail loop


def _close(got, want, what):
    """max |got - want| <= 1e-10 max |want|, all finite; prints the figure."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.all(np.isfinite(got)), what
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    print("%s: max deviation %.3e, largest component %.3e" % (what, err, scale))
    assert err <= TOL * scale, "%s: %g > %g" % (what, err, TOL * scale)


def _sim(name, params, xyz, dihedrals, typeid, box, virial=True, types=None, velocity=None, dt=0.0):
    types = types if types is not None else ["T%d" % t for t in range(len(params))]
    snap = azp.Snapshot.from_arrays(xyz, box, dihedrals=dihedrals, dihedral_typeid=typeid, dihedral_types=types, velocity=velocity)
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(snap)
    sim.operations.tuners.clear()
    f = getattr(azp.dihedral, name)()
    for t, p in zip(types, params):
        f.params[t] = p
    f.compute_virial = virial
    sim.operations.integrator = azp.Integrator(dt=dt, forces=[f], methods=[azp.ConstantVolume()])
    return sim, f


def _check_against(f, out, what):
    _close(f.forces, out["force"], what + " forces")
    _close(f.energies, out["energies"], what + " energies")
    for r, label in enumerate(("xx", "xy", "xz", "yy", "yz", "zz")):
        _close(f.virials[:, r], out["virial"][:, r], "%s virial %s" % (what, label))


# ---------------------------------------------------------------------------------------------------------------------
def test_known_answer_and_across_periodic_faces():
    """The hand-derived case of tests/test_dihedral.py through Simulation, then shifted so that a sits across the +x
    face and d across the +y face of the box."""
    want_f = np.array([[0.0, -5.0, 0.0], [0.0, 5.0, 0.0], [5.0, 0.0, 0.0], [-5.0, 0.0, 0.0]])
    base = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, 1.0, 1.0]])
    shifted = base + np.array([9.5, 9.5, 0.0])
    shifted[0, 0] -= 20.0
    shifted[3, 1] -= 20.0
    assert shifted[0, 0] == -9.5 and shifted[3, 1] == -9.5
    # W = (-b1) (x) F_a + b2 (x) F_c + (b2 + b3) (x) F_d with b1 = (-1, 0, 0), b2 = (0, 0, 1), b3 = (0, 1, 0)
    W = np.outer([1.0, 0.0, 0.0], want_f[0]) + np.outer([0.0, 0.0, 1.0], want_f[2]) + np.outer([0.0, 1.0, 1.0], want_f[3])
    assert W[0, 0] + W[1, 1] + W[2, 2] == 0.0
    for what, xyz in (("known answer", base), ("known answer across the faces", shifted)):
        sim, f = _sim("Periodic", [dict(k=10.0, d=1, n=1, phi0=0.0)], xyz, [(0, 1, 2, 3)], [0], (20.0, 20.0, 20.0))
        sim.run(0)
        _close(f.forces, want_f, what + " forces")
        _close(f.energies, np.full(4, 1.25), what + " energies")
        assert abs(f.energy - 5.0) <= TOL * 5.0
        _close(f.virials.sum(axis=0), np.array([W[0, 0], W[0, 1], W[0, 2], W[1, 1], W[1, 2], W[2, 2]]), what + " virial")


@pytest.mark.parametrize("box", ["cubic", "triclinic"])
@pytest.mark.parametrize("name", POTENTIALS)
def test_parity_system(name, box):
    xyz, dihedrals, typeid, L, tilt = cases.parity_system(box)
    out = cases.parity_reference(name, box)
    sim, f = _sim(name, cases.PARAMS[name], xyz, dihedrals, typeid, azp.Box(L[0], L[1], L[2], *tilt))
    sim.run(0)
    tab = sim.state.dihedral_table()
    # the centre particles of the branched cluster take six turns of the tail loop, an interior chain bead one, an end bead none
    assert tab["width"] == 9 > BATCH and int(tab["n_dihedrals"][cases.CENTRE[0]]) == int(tab["n_dihedrals"][cases.CENTRE[1]]) == 9
    assert int(tab["n_dihedrals"][4]) == 4 and int(tab["n_dihedrals"][cases.RING[0]]) == 4 and int(tab["n_dihedrals"][0]) == 1
    _check_against(f, out, "%s %s" % (name, box))
    # particles without dihedrals: exact zeros everywhere
    lone = list(cases.LONE)
    assert not f.forces[lone].any() and not f.energies[lone].any() and not f.virials[lone].any()
    assert np.abs(out["force"]).max() > 10.0 and np.abs(out["virial"]).max() > 1.0


@pytest.mark.parametrize("case", list(cases.PARAMS_EDGE))
def test_planar_edge_dihedrals(case):
    """phi exactly 0 and exactly pi (four coplanar members: n1 and n2 parallel or antiparallel, sin phi = 0 exactly) and
    pi - 1e-9 and -(pi - 1e-9), either side of the cut of atan2, with Periodic n = 1, 2, 3 (two of them with a non-zero
    phi0) and OPLS, with one dihedral at phi = 1 for the scale of the comparison (tests/dihedral_cases.py says why). The
    gradient has no 1 / sin phi, so nothing is floored."""
    name, params = cases.PARAMS_EDGE[case]
    xyz, dihedrals, L = cases.edge_system()
    out = ref.evaluate(name, [params], xyz, dihedrals, [0] * 5, L)
    assert out["phi"][0] == 0.0 and out["phi"][1] == math.pi
    assert abs(out["phi"][2] - (math.pi - 1e-9)) < 1e-15 and abs(out["phi"][3] + (math.pi - 1e-9)) < 1e-15
    assert abs(out["phi"][4] - 1.0) < 1e-15 and np.abs(out["force"][16:]).max() > 1.0
    sim, f = _sim(name, [params], xyz, dihedrals, [0] * 5, L)
    sim.run(0)
    _check_against(f, out, case + " planar edge cases")
    if case in ("Periodic-n1", "OPLS"):
        assert not f.forces[:8].any()       # U'(0) = U'(pi) = 0 where every term is a cosine of a multiple of phi
    else:
        assert np.abs(f.forces[:4]).max() > 0.1 and np.abs(f.forces[4:8]).max() > 0.1   # phi0 != 0: a force at 0 and at pi
    # continuity across the cut: the two dihedrals at +-(pi - 1e-9) have the same energy to 1e-8 of it
    assert abs(f.energies[8] - f.energies[12]) <= 1e-7 * max(abs(f.energies[8]), 1.0)


def _direct(name, xyz, dihedrals, typeid, L, tilt, n_local, compute_virial=True, block_size=0):
    """The C entry point on a table for the first n_local rows; output buffers span ALL rows and start as NaN."""
    import torch

    n = xyz.shape[0]
    pos = torch.from_numpy(np.ascontiguousarray(np.c_[xyz, np.zeros(n)])).to("cuda:0")   # rows of (x, y, z, w)
    tab = build_dihedral_table(torch.from_numpy(np.asarray(dihedrals, dtype=np.int64)).to("cuda:0"),
                               torch.from_numpy(np.asarray(typeid, dtype=np.int64)).to("cuda:0"), n_local)
    force = torch.full((n, 4), float("nan"), dtype=torch.float64, device="cuda:0")
    virial = torch.full((6, n), float("nan"), dtype=torch.float64, device="cuda:0")
    pot = getattr(azp.dihedral, name)()
    params = torch.from_numpy(np.stack([pot._pack(pot.params._validate(p)) for p in cases.PARAMS[name]])).to("cuda:0")
    a = _lib.DihedralArgs()
    a.d_force, a.d_virial, a.virial_pitch = force.data_ptr(), virial.data_ptr(), n
    a.N, a.n_max, a.d_pos = n_local, n, pos.data_ptr()
    a.box = _lib.make_box(L, tilt)
    a.d_gpu_dihedrallist, a.d_gpu_n_dihedrals, a.pitch = tab["table"].data_ptr(), tab["n_dihedrals"].data_ptr(), tab["pitch"]
    a.n_dihedral_types, a.compute_virial, a.block_size = len(cases.PARAMS[name]), int(compute_virial), block_size
    _lib.check(getattr(_lib.lib(), pot._entry)(C.byref(a), params.data_ptr(), torch.cuda.current_stream().cuda_stream), pot._entry)
    torch.cuda.synchronize()
    return force.cpu().numpy(), virial.cpu().numpy()


@pytest.mark.parametrize("name", POTENTIALS)
def test_ghost_rows(name):
    """The last 70 rows are ghosts (the tail of the chains, the ring, the branched cluster): the 305 locals get the
    whole-system reference (every dihedral with a local member is in their table), and no row from 305 on is written,
    in the force or in the virial."""
    xyz, dihedrals, typeid, L, tilt = cases.parity_system("cubic")
    out = cases.parity_reference(name, "cubic")
    n_local = 305
    force, virial = _direct(name, xyz, dihedrals, typeid, L, tilt, n_local)
    _close(force[:n_local, :3], out["force"][:n_local], name + " ghost rows: local forces")
    _close(force[:n_local, 3], out["energies"][:n_local], name + " ghost rows: local energies")
    _close(virial[:, :n_local].T, out["virial"][:n_local], name + " ghost rows: local virials")
    assert np.isnan(force[n_local:]).all() and np.isnan(virial[:, n_local:]).all()
    # and through State: ghosts declared by n_local
    snap = azp.Snapshot.from_arrays(xyz, L, dihedrals=dihedrals, dihedral_typeid=typeid, dihedral_types=["T0", "T1"])
    st = azp.State(snap, "cuda:0", n_local=n_local)
    assert st.N == n_local and st.n_ghost == 70 and st.dihedral_table()["table"].shape[1] == n_local


def test_empty_topology():
    xyz = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    snap = azp.Snapshot.from_arrays(xyz, (10.0, 10.0, 10.0))
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(snap)
    f = azp.dihedral.OPLS()
    f.compute_virial = True
    sim.operations.integrator = azp.Integrator(dt=0.0, forces=[f])
    sim.run(0)
    assert sim.state.n_dihedrals == 0
    assert f.forces.shape == (4, 3) and not f.forces.any() and not f.energies.any() and not f.virials.any()


@pytest.mark.parametrize("name", POTENTIALS)
def test_deterministic_and_block_sizes(name):
    """Two compute() calls leave the same bits, and so do block sizes 64, 128 and 256 (one lane per particle sums its
    entries in table order whatever the block is); 96 is rejected."""
    xyz, dihedrals, typeid, L, tilt = cases.parity_system("triclinic")
    sim, f = _sim(name, cases.PARAMS[name], xyz, dihedrals, typeid, azp.Box(L[0], L[1], L[2], *tilt))
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
def test_sorter_reindexes_dihedrals(name):
    xyz, dihedrals, typeid, L, tilt = cases.parity_system("cubic")
    out = cases.parity_reference(name, "cubic")
    sim, f = _sim(name, cases.PARAMS[name], xyz, dihedrals, typeid, L)
    sim.run(0)
    order = azp.ParticleSorter(particles_per_block=16).sort(sim).cpu().numpy()
    assert (order != np.arange(order.size)).sum() > 300      # the sort did move the particles
    f.compute(0)
    tag = sim.state.tag.cpu().numpy().view(np.uint32).astype(np.int64)
    assert np.array_equal(tag, order)
    assert np.array_equal(tag[sim.state.dihedral_group.astype(np.int64)], dihedrals)   # the members by tag are what they were
    got = dict(force=np.zeros((order.size, 3)), energies=np.zeros(order.size), virial=np.zeros((order.size, 6)))
    got["force"][tag], got["energies"][tag], got["virial"][tag] = f.forces, f.energies, f.virials
    _close(got["force"], out["force"], name + " after the sort: forces by tag")
    _close(got["energies"], out["energies"], name + " after the sort: energies by tag")
    _close(got["virial"], out["virial"], name + " after the sort: virials by tag")


# ---------------------------------------------------------------------------------------------------------------------
# in a run
# ---------------------------------------------------------------------------------------------------------------------
BOND_PARAMS = dict(r_0=1.0, r_1=1.5, U_1=1.0, U_tilt=0.5)
ANGLE_PARAMS = dict(k=10.0, t0=2.0)
NVE_STEPS, NVE_DT = 20, 0.002
# worst position deviation of the same 20-step comparison with the DoubleWell bonds and the Harmonic angles ALONE,
# nve_deviation(oracle, False), measured on the MI355X (three runs, the same figure; the bond, angle and NVE kernels are those of the parent commit),
# times 10
NVE_BONDS_ANGLES_DEVIATION = 4.440892e-16
NVE_BOUND = 10.0 * NVE_BONDS_ANGLES_DEVIATION


def nve_deviation(oracle, with_dihedrals):
    """20 velocity-Verlet steps of the 40 chains of the parity system (DoubleWell bonds, Harmonic angles, optionally
    Periodic dihedrals) on the GPU and in NumPy (bond forces from the oracle, angle forces from angle_ref, dihedral
    forces from dihedral_ref): worst position deviation."""
    xyz, dihedrals, typeid, L, tilt = cases.parity_system("cubic")
    n = cases.N_CHAINS * cases.CHAIN_LEN
    nd = cases.N_CHAINS * (cases.CHAIN_LEN - 3)
    xyz, dihedrals, typeid = xyz[:n], dihedrals[:nd], typeid[:nd]
    assert dihedrals.max() == n - 1
    bonds, angles = cases.chain_bonds(), cases.chain_angles()
    atype = np.zeros(len(angles), dtype=np.uint32)
    vel0 = np.random.default_rng(5).normal(size=(n, 3)) * 0.5
    vel0 -= vel0.mean(axis=0)
    snap = azp.Snapshot.from_arrays(xyz, L, velocity=vel0, bonds=bonds, angles=angles, dihedrals=dihedrals, dihedral_typeid=typeid,
                                    dihedral_types=["T0", "T1"])
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(snap)
    sim.operations.tuners.clear()
    dw = azp.bond.DoubleWell()
    dw.params["A-A"] = BOND_PARAMS
    ha = azp.angle.Harmonic()
    ha.params["A-A-A"] = ANGLE_PARAMS
    forces = [dw, ha]
    if with_dihedrals:
        pd = azp.dihedral.Periodic()
        pd.params["T0"], pd.params["T1"] = cases.PARAMS["Periodic"]
        forces.append(pd)
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
        f += angle_ref.evaluate("Harmonic", [ANGLE_PARAMS], x, angles, atype, L)["force"]
        if with_dihedrals:
            f += ref.evaluate("Periodic", cases.PARAMS["Periodic"], x, dihedrals, typeid, L)["force"]
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


def test_nve_run_with_bonds_angles_and_dihedrals(oracle):
    """20 NVE steps, dt = 0.002, chains with DoubleWell bonds, Harmonic angles and Periodic dihedrals, against the NumPy
    velocity-Verlet. The bound is 10 x the worst position deviation of the same comparison with bonds and angles alone
    (dihedrals add one more rounding-level force per step). Measured on the MI355X: bonds + angles alone 4.44e-16 (half
    an ulp of a coordinate between 4 and 8), so the bound is 4.44e-15; bonds + angles + dihedrals 4.44e-16."""
    dev = nve_deviation(oracle, with_dihedrals=True)
    print("NVE, bonds + angles + dihedrals: worst position deviation %.3e (bound %.3e)" % (dev, NVE_BOUND))
    assert dev <= NVE_BOUND


@pytest.mark.parametrize("name", POTENTIALS)
def test_thermo_picks_up_energy_and_virial(name):
    """ThermodynamicQuantities with the dihedral force alone: the potential energy and the pressure tensor equal the
    reference's sums to 1e-10 relative. A torsion potential depends on directions only, so the trace of its virial is
    zero and the scalar pressure holds the kinetic part alone; the particles are given velocities for that reason, and
    the six components of the pressure tensor, where the dihedral virial does not cancel, are held to 1e-10 of the
    largest of them."""
    from azplugins_amd import compute

    xyz, dihedrals, typeid, L, tilt = cases.parity_system("cubic")
    out = cases.parity_reference(name, "cubic")
    vel = np.random.default_rng(9).normal(size=xyz.shape) * 0.2
    sim, f = _sim(name, cases.PARAMS[name], xyz, dihedrals, typeid, L, virial=False, velocity=vel)
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
    """The dihedral force in Integrator.forces under flow.Langevin and flow.Brownian: the run goes through and stays
    finite (the integration itself is pinned in tests/test_gpu_flow.py)."""
    from azplugins_amd import flow

    xyz, dihedrals, typeid, L, tilt = cases.parity_system("cubic")
    sim, f = _sim("Periodic", cases.PARAMS["Periodic"], xyz, dihedrals, typeid, L, virial=False)
    field = flow.ConstantFlow(velocity=(0.0, 0.0, 0.0))
    cls = flow.Langevin if method == "langevin" else flow.Brownian
    m = cls(filter=azp.All(), kT=1.0, flow_field=field)
    m.gamma["A"] = 1.0
    sim.operations.integrator = azp.Integrator(dt=0.001, forces=[f], methods=[m])
    sim.run(5)
    assert np.all(np.isfinite(sim.state.pos.cpu().numpy())) and np.all(np.isfinite(f.forces)) and np.abs(f.forces).max() > 0.0
