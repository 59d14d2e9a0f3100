"""compute.ThermodynamicQuantities and ThermodynamicRecorder on the GPU (csrc/thermo.hip): the reduction against exact
sums (tests/thermo_ref.py), the properties end to end against the CPU oracle's energies and virials, the virial switch,
a recorder that must not change the trajectory, recorded rows against the properties of fresh runs, and a decomposed
run on two ranks.

Error bound of the reduction (``thermo_ref.REL_BOUND`` = 256 * 2^-53 relative to the sum of the magnitudes of a slot's
terms): derived from the kernel's addition depth (<= 200 for N <= 2^24), not measured."""

import os
import socket

import numpy as np
import pytest

import helpers as H
import reduction_ref as red
import thermo_ref as ref
from azplugins_amd import synthetic as syn

pytestmark = pytest.mark.gpu

PARITY_TOL = 1e-10  # tests/test_gpu_parity.py: energies and per-particle virials against the oracle


def _table_force_class():
    from azplugins_amd.force import Force

    class TableForce(Force):
        """A force whose per-particle force / energy and virial rows are given arrays (a custom force)."""

        def __init__(self, force, virial):
            super().__init__()
            self._f, self._w = force, virial

        def compute(self, timestep=None):
            import torch

            self._require()
            self._ensure_buffers()
            self._force.copy_(torch.from_numpy(self._f))
            self._virial.copy_(torch.from_numpy(self._w))

    return TableForce


def _gas(N, seed, n_forces, drift=(1.0e3, -7.0e2, 2.5e2)):
    """Ideal gas of two populated types (and an empty third), non-uniform masses, a common drift far above the thermal
    speed, rotational state with a third of the inertia components zero, and ``n_forces`` table forces."""
    import azplugins_amd as azp

    rng = np.random.default_rng(seed)
    L = 20.0
    typeid = rng.integers(0, 2, N)
    snap = azp.Snapshot.from_arrays(rng.uniform(-0.5 * L, 0.5 * L, (N, 3)), [L, L, L], typeid=typeid, types=("A", "B", "C"),
                                    velocity=rng.normal(size=(N, 3)) + np.asarray(drift), orientation=syn.random_quaternions(N, seed + 1),
                                    moment_inertia=rng.uniform(0.5, 2.0, (N, 3)) * (rng.uniform(size=(N, 3)) > 1.0 / 3.0),
                                    angmom=rng.normal(size=(N, 4)))
    snap.particles.mass[:] = rng.uniform(0.5, 2.0, N)
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(snap)
    sim.operations.tuners.clear()
    cls = _table_force_class()
    forces = [cls(rng.normal(size=(N, 4)) * 10.0 ** k, rng.normal(size=(6, N)) * 3.0 ** k) for k in range(n_forces)]
    sim.operations.integrator = azp.Integrator(dt=0.001, forces=forces)
    return sim


def _host_terms(sim, select):
    st = sim.state
    N = st.N
    forces = sim.operations.integrator.forces
    return ref.terms(st.vel[:N].cpu().numpy(), select, [f._force.cpu().numpy() for f in forces],
                     [f._virial.cpu().numpy() for f in forces], st.orientation[:N].cpu().numpy(), st.angmom[:N].cpu().numpy(),
                     st.inertia[:N].cpu().numpy())


def _check_row(got, terms, what):
    want, mag = ref.exact(terms)
    print("%s: slot | got | exact | |err| / sum|term| (bound %.3g)" % (what, ref.REL_BOUND))
    for k in range(ref.NSUMS):
        err = abs(got[k] - want[k])
        print("  %2d %.17g %.17g %.3g" % (k, got[k], want[k], err / mag[k] if mag[k] else err))
    for k in range(ref.NSUMS):
        if k in (0, 18, 19):
            assert got[k] == want[k], (what, k)
        else:
            assert abs(got[k] - want[k]) <= ref.REL_BOUND * mag[k], (what, k, got[k], want[k], mag[k])


# ---------------------------------------------------------------------------------------------------------------------
# 1. the reduction against exact sums
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_forces", [1, 2, 8])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 10007, 2**20])
def test_reduction_against_exact_sums(N, n_forces):
    import torch

    import azplugins_amd as azp
    from azplugins_amd import compute

    sim = _gas(N, seed=100 + N % 97 + n_forces, n_forces=n_forces)
    filters = {"All": azp.All(), "A": azp.Type(["A"]), "C": azp.Type(["C"])}
    thermos = {k: compute.ThermodynamicQuantities(f) for k, f in filters.items()}
    for t in thermos.values():
        sim.operations.add(t)
    sim.run(0)
    typeid = sim.state.typeid_host
    select = {"All": np.ones(N, bool), "A": typeid == 0, "C": typeid == 2}
    assert not select["C"].any()
    for key, thermo in thermos.items():
        first = thermo._sums().clone()
        second = thermo._sums().clone()
        torch.cuda.synchronize()
        assert torch.equal(first.view(torch.int64), second.view(torch.int64)), "two calls differ in bits"
        got = first.cpu().numpy()[0]
        if key == "C":
            assert not got.any()  # a filter that selects nothing
            assert thermo.num_particles == 0 and thermo.kinetic_temperature == 0.0 and thermo.pressure == 0.0
            continue
        _check_row(got, _host_terms(sim, select[key]), "N=%d forces=%d filter=%s" % (N, n_forces, key))
        assert thermo.num_particles == int(select[key].sum())
        assert thermo.linear_momentum == (got[1], got[2], got[3])


@pytest.mark.parametrize("n_forces", [1, 3])
@pytest.mark.parametrize("N", [1, 64, 65, 257, 10007, 524289])
def test_reduction_order_bit_for_bit(N, n_forces):
    """The row is the documented tree (csrc/azp_reduce.hpp, restated in tests/reduction_ref.py) over the per-particle
    terms, in every bit. 65 and 257 put the tail in a second wave and a second workgroup; 524,289 is the smallest N with
    two particles per lane: 1,025 partials, 17 trips of the fold's lanes."""
    import azplugins_amd as azp
    from azplugins_amd import compute

    sim = _gas(N, seed=300 + N % 89 + n_forces, n_forces=n_forces)
    thermos = {"All": compute.ThermodynamicQuantities(azp.All()), "A": compute.ThermodynamicQuantities(azp.Type(["A"]))}
    for t in thermos.values():
        sim.operations.add(t)
    sim.run(0)
    st = sim.state
    forces = sim.operations.integrator.forces
    select = {"All": np.ones(N, bool), "A": st.typeid_host == 0}
    for key, thermo in thermos.items():
        got = thermo._sums().cpu().numpy()[0]
        terms = ref.particle_terms(st.vel[:N].cpu().numpy(), select[key], [f._force.cpu().numpy() for f in forces],
                                   [f._virial.cpu().numpy() for f in forces], st.orientation[:N].cpu().numpy(),
                                   st.angmom[:N].cpu().numpy(), st.inertia[:N].cpu().numpy())
        want = red.tree_sum(terms)
        differ = np.flatnonzero(got.view(np.int64) != want.view(np.int64))
        print("N=%d forces=%d filter=%s: slots that differ in bits: %s" % (N, n_forces, key, differ.tolist()))
        for k in differ:
            print("  %2d %r %r" % (k, got[k], want[k]))
        assert differ.size == 0, (key, differ.tolist())
        assert got[0] == select[key].sum() and (N < 64 or got[16] != 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# 2. end to end against the oracle
# ---------------------------------------------------------------------------------------------------------------------
def _velocities(n, seed, kT=1.3):
    tag = np.arange(n, dtype=np.uint64)
    v = np.stack([syn.normal(seed, tag, c) for c in range(3)], axis=1) * np.sqrt(kT)
    return v - v.mean(axis=0)


def _chains_sim():
    import azplugins_amd as azp

    cfg = syn.config_chains(16, 12, 12, 16)
    n = cfg["xyz"].shape[0]
    snap = azp.Snapshot.from_arrays(cfg["xyz"], cfg["L"], bonds=cfg["bonds"], velocity=_velocities(n, 81))
    snap.particles.mass[:] = 0.5 + 1.5 * syn.u01(82, np.arange(n, dtype=np.uint64), 0)
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(snap)
    nl = azp.nlist.Cell(buffer=0.4)
    plj = azp.pair.PerturbedLennardJones(nlist=nl, default_r_cut=3.0, mode="shift")
    plj.params[("A", "A")] = cfg["params"]
    dw = azp.bond.DoubleWell()
    dw.params["A-A"] = cfg["bond_params"]
    sim.operations.integrator = azp.Integrator(dt=0.001, forces=[plj, dw], methods=[azp.ConstantVolume()])
    return sim, cfg


def _chains_oracle(oracle, cfg):
    pos = syn.pos4(cfg["xyz"])
    box = oracle.make_box(cfg["L"])
    N = pos.shape[0]
    n_excl = np.zeros(N, dtype=np.uint32)
    excl = np.zeros((N, 2), dtype=np.uint32)
    for a_, b_ in cfg["bonds"]:
        for me, other in ((a_, b_), (b_, a_)):
            excl[me, n_excl[me]] = other
            n_excl[me] += 1
    onl = oracle.build_nlist(pos, box, 3.4, half=True, exclusions=(n_excl, excl))
    f_pair, v_pair = oracle.pair_forces("PerturbedLennardJones", pos, box, onl,
                                        oracle.pack_pair_params("PerturbedLennardJones", cfg["params"]), 3.0, mode="shift", half=True,
                                        virial=True)
    f_bond, bad, v_bond = oracle.bond_forces("DoubleWell", pos, box, cfg["bonds"], np.zeros(len(cfg["bonds"]), dtype=np.uint32),
                                             oracle.pack_bond_params("DoubleWell", cfg["bond_params"]), virial=True)
    assert bad == 0
    return [f_pair, f_bond], [v_pair, v_bond]


COLLOID_RADIUS = (0.0, 0.3)


def _colloid_params(i, j):
    return dict(A=40.0 + 5 * (i + j), a_1=COLLOID_RADIUS[i], a_2=COLLOID_RADIUS[j], sigma=0.5)


def _colloid_sim():
    import azplugins_amd as azp

    pos, L, typeid = H.lattice_config(10, 1.6, 0.16, seed=21, ntypes=2)
    n = pos.shape[0]
    snap = azp.Snapshot.from_arrays(pos[:, :3], L, typeid=typeid, types=("A", "B"), velocity=_velocities(n, 83))
    snap.particles.mass[:] = np.where(typeid == 0, 1.0, 3.5)
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(snap)
    nl = azp.nlist.Cell(buffer=0.3)
    pot = azp.pair.Colloid(nlist=nl, default_r_cut=3.2, mode="shift")
    names = ("A", "B")
    for i in range(2):
        for j in range(i, 2):
            pot.params[(names[i], names[j])] = _colloid_params(i, j)
    sim.operations.integrator = azp.Integrator(dt=0.001, forces=[pot], methods=[azp.ConstantVolume()])
    return sim, dict(pos=pos, L=L, typeid=typeid)


def _colloid_oracle(oracle, cfg):
    box = oracle.make_box(cfg["L"])
    params = np.array([oracle.pack_pair_params("Colloid", _colloid_params(min(i, j), max(i, j))) for i in range(2) for j in range(2)])
    onl = oracle.build_nlist(cfg["pos"], box, 3.5, ntypes=2, half=True)
    f, v = oracle.pair_forces("Colloid", cfg["pos"], box, onl, params, 3.2, 0.0, "shift", ntypes=2, half=True, virial=True)
    return [f], [v]


@pytest.mark.parametrize("system", ["chains", "colloid"])
def test_end_to_end_against_oracle(oracle, system):
    import azplugins_amd as azp
    from azplugins_amd import compute

    sim, cfg = _chains_sim() if system == "chains" else _colloid_sim()
    filters = [azp.All()] + ([azp.Type(["B"])] if system == "colloid" else [])
    thermos = [compute.ThermodynamicQuantities(f) for f in filters]
    for t in thermos:
        sim.operations.add(t)
    sim.run(0)
    f_ref, v_ref = _chains_oracle(oracle, cfg) if system == "chains" else _colloid_oracle(oracle, cfg)
    st = sim.state
    N = st.N
    V = float(np.prod(cfg["L"]))
    typeid = st.typeid_host
    vel = st.vel[:N].cpu().numpy()
    for flt, thermo in zip(filters, thermos):
        sel = np.ones(N, bool) if isinstance(flt, azp.All) else typeid == 1
        t = ref.terms(vel, sel, f_ref, v_ref)
        want, mag = ref.exact(t)
        assert thermo.num_particles == int(sel.sum()) and thermo.volume == pytest.approx(V, rel=1e-15)
        u = thermo.potential_energy
        print("%s %r: U %.17g oracle %.17g rel %.3g" % (system, flt, u, want[16], abs(u - want[16]) / mag[16]))
        assert abs(u - want[16]) <= PARITY_TOL * mag[16]
        P = thermo.pressure_tensor
        assert isinstance(P, tuple) and len(P) == 6
        for c in range(6):
            w = P[c] * V - want[4 + c]  # (K_ab from the exact host sum of the velocities the kernel read)
            print("  W[%d] %.17g oracle %.17g rel %.3g" % (c, w, want[10 + c], abs(w - want[10 + c]) / mag[10 + c]))
            assert abs(w - want[10 + c]) <= PARITY_TOL * mag[10 + c] + 4 * ref.REL_BOUND * mag[4 + c]
        assert mag[10] > 0 and mag[16] > 0  # (virials and energies that matter)
        assert thermo.pressure == pytest.approx((P[0] + P[3] + P[5]) / 3.0, rel=1e-15)
        half_trace = 0.5 * (want[4] + want[7] + want[9])
        assert abs(thermo.kinetic_energy - half_trace) <= ref.REL_BOUND * 0.5 * (mag[4] + mag[7] + mag[9])
        assert thermo.kinetic_energy == thermo.translational_kinetic_energy and thermo.rotational_degrees_of_freedom == 0
        for c, p in enumerate(thermo.linear_momentum):
            assert abs(p - want[1 + c]) <= ref.REL_BOUND * mag[1 + c]
        n_g = int(sel.sum())
        assert thermo.translational_degrees_of_freedom == pytest.approx(3 * n_g - 3 * n_g / N, rel=1e-15)
        assert thermo.kinetic_temperature == pytest.approx(2 * thermo.kinetic_energy / thermo.degrees_of_freedom, rel=1e-15)
    assert thermos[0].kinetic_temperature == pytest.approx(sim.kinetic_temperature(), rel=1e-12)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the virial switch
# ---------------------------------------------------------------------------------------------------------------------
def test_virial_switch_and_force_limit():
    import azplugins_amd as azp
    from azplugins_amd import compute

    sim, _ = _chains_sim()
    forces = sim.operations.integrator.forces
    sim.run(2)
    assert [f.compute_virial for f in forces] == [False, False]  # without the compute nothing changes
    thermo = compute.ThermodynamicQuantities(azp.All())
    sim.operations.add(thermo)
    assert [f.compute_virial for f in forces] == [False, False]
    assert thermo.kinetic_temperature > 0.0 and np.isfinite(thermo.potential_energy)  # (these need no virial)
    for name in ("pressure", "pressure_tensor"):
        with pytest.raises(azp.AzpError, match=r"sim\.run\(0\)"):
            getattr(thermo, name)
    sim.run(0)
    assert [f.compute_virial for f in forces] == [True, True]
    assert np.isfinite(thermo.pressure) and thermo.pressure != 0.0
    sim.operations.remove(thermo)
    with pytest.raises(compute.DataAccessError):
        thermo.pressure
    # nine forces
    sim9, _ = _chains_sim()
    sim9.operations.integrator.forces = [azp.bond.DoubleWell() for _ in range(9)]
    sim9.operations.add(compute.ThermodynamicQuantities(azp.All()))
    with pytest.raises(azp.AzpError, match="at most 8 forces"):
        sim9.run(0)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the recorder does not perturb the run; 5. rows are the properties
# ---------------------------------------------------------------------------------------------------------------------
def _liquid_sim(ncell=12):
    import azplugins_amd as azp

    cfg = syn.config_north_star(ncell=ncell)
    n = cfg["xyz"].shape[0]
    snap = azp.Snapshot.from_arrays(cfg["xyz"], cfg["L"], velocity=_velocities(n, 91, kT=1.0))
    sim = azp.Simulation(device="cuda:0", seed=3)
    sim.create_state_from_snapshot(snap)  # (the default ParticleSorter stays in sim.operations.tuners)
    assert len(sim.operations.tuners) == 1
    nl = azp.nlist.Cell(buffer=cfg["r_buff"])
    plj = azp.pair.PerturbedLennardJones(nlist=nl, default_r_cut=cfg["r_cut"], mode="shift")
    plj.params[("A", "A")] = cfg["params"]
    sim.operations.integrator = azp.Integrator(dt=0.004, forces=[plj], methods=[azp.ConstantVolume()])
    return sim


def _tpm_sim():
    import azplugins_amd as azp

    cfg = syn.config_tpm(10, 10, 20)
    n = cfg["xyz"].shape[0]
    snap = azp.Snapshot.from_arrays(cfg["xyz"], cfg["L"], velocity=_velocities(n, 61, kT=2.0), orientation=cfg["orientation"],
                                    moment_inertia=np.tile(np.array([0.1, 0.12, 0.14]), (n, 1)))
    sim = azp.Simulation(device="cuda:0", seed=3)
    sim.create_state_from_snapshot(snap)
    nl = azp.nlist.Cell(buffer=cfg["r_buff"])
    pot = azp.pair.TwoPatchMorse(nlist=nl, default_r_cut=cfg["r_cut"], mode="shift")
    pot.params[("A", "A")] = cfg["params"]
    sim.operations.integrator = azp.Integrator(dt=0.004, forces=[pot], methods=[azp.ConstantVolume()], integrate_rotational_dof=True)
    return sim


def _langevin_sim():
    import azplugins_amd as azp
    from azplugins_amd import flow

    cfg = syn.config_north_star(ncell=10)
    n = cfg["xyz"].shape[0]
    snap = azp.Snapshot.from_arrays(cfg["xyz"], cfg["L"], velocity=_velocities(n, 93, kT=1.0))
    snap.particles.mass[:] = 0.5 + 1.5 * syn.u01(94, np.arange(n, dtype=np.uint64), 0)
    sim = azp.Simulation(device="cuda:0", seed=77)
    sim.create_state_from_snapshot(snap)
    nl = azp.nlist.Cell(buffer=cfg["r_buff"])
    plj = azp.pair.PerturbedLennardJones(nlist=nl, default_r_cut=cfg["r_cut"], mode="shift")
    plj.params[("A", "A")] = cfg["params"]
    m = flow.Langevin(filter=azp.All(), kT=1.2, flow_field=flow.ParabolicFlow(mean_velocity=0.8, separation=float(cfg["L"][1])),
                      default_gamma=2.0)
    sim.operations.integrator = azp.Integrator(dt=0.002, forces=[plj], methods=[m])
    return sim


SYSTEMS = {"nve_liquid": _liquid_sim, "tpm_rotational": _tpm_sim, "langevin_parabolic": _langevin_sim}


def _final_state(sim):
    import torch

    torch.cuda.synchronize()
    st = sim.state
    out = dict(pos=st.pos, vel=st.vel, image=st.image, orientation=st.orientation, angmom=st.angmom, tag=st.tag)
    if st.accel is not None:
        out["accel"] = st.accel
    return {k: v.clone() for k, v in out.items()}


@pytest.mark.parametrize("system", sorted(SYSTEMS))
def test_recorder_does_not_perturb_the_run(system):
    import torch

    import azplugins_amd as azp
    from azplugins_amd import compute

    finals = {}
    for period in (None, 7, 1):
        sim = SYSTEMS[system]()
        rec = None
        if period is not None:
            thermo = compute.ThermodynamicQuantities(azp.All())
            sim.operations.add(thermo)
            rec = compute.ThermodynamicRecorder(thermo, azp.Periodic(period))
            sim.operations.add(rec)
        sim.run(60)
        finals[period] = _final_state(sim)
        assert sim.timestep == 60
        if rec is not None:
            assert rec.timesteps.tolist() == list(range(period, 61, period))
            table = rec.table
            assert np.all(np.isfinite(table["pressure"])) and np.all(table["kinetic_temperature"] > 0.0)
            assert np.all(table["num_particles"] == sim.state.N)
            if system == "tpm_rotational":
                assert np.all(table["rotational_degrees_of_freedom"] == 3 * sim.state.N) and np.all(table["rotational_kinetic_energy"] > 0)
    base = finals[None]
    assert not torch.equal(base["vel"], SYSTEMS[system]().state.vel)  # (the run moved the system)
    for period in (7, 1):
        assert finals[period].keys() == base.keys()
        for name, want in base.items():
            assert torch.equal(finals[period][name], want), "recorder at period %d changed %s" % (period, name)


def test_rows_are_the_properties():
    import azplugins_amd as azp
    from azplugins_amd import compute

    def make(with_recorder):
        sim = _tpm_sim()
        thermo = compute.ThermodynamicQuantities(azp.All())
        sim.operations.add(thermo)
        rec = compute.ThermodynamicRecorder(thermo, azp.Periodic(7)) if with_recorder else None
        if rec is not None:
            sim.operations.add(rec)
        return sim, thermo, rec

    sim, thermo, rec = make(True)
    sim.run(21)
    assert rec.timesteps.tolist() == [7, 14, 21]
    table = rec.table
    assert set(table) == set(compute.THERMO_PROPERTIES)
    for row, t in enumerate((7, 14, 21)):
        fresh, fresh_thermo, _ = make(False)
        fresh.run(t)
        for name in compute.THERMO_PROPERTIES:
            want = np.asarray(getattr(fresh_thermo, name))
            got = np.asarray(table[name][row])
            assert got.shape == want.shape and got.tobytes() == want.astype(got.dtype).tobytes(), (t, name, got, want)
    # the last row is also what the recording simulation's own compute reports now
    for name in compute.THERMO_PROPERTIES:
        assert np.asarray(table[name][2]).tolist() == np.asarray(getattr(thermo, name)).tolist()
    sim.run(7)
    assert rec.timesteps.tolist() == [7, 14, 21, 28]
    again = rec.table
    for name in compute.THERMO_PROPERTIES:
        assert again[name].shape[0] == 4 and again[name][:3].tobytes() == table[name].tobytes()


def test_recorder_table_grows_by_doubling():
    import azplugins_amd as azp
    from azplugins_amd import compute

    sim = _liquid_sim(ncell=6)
    thermo = compute.ThermodynamicQuantities(azp.All())
    rec = compute.ThermodynamicRecorder(thermo, 1)
    sim.operations.add(thermo)
    sim.operations.add(rec)
    sim.run(64)
    first = rec.table
    assert rec._rows.shape[0] == 64
    sim.run(70)
    assert rec._rows.shape[0] == 256 and rec.timesteps.tolist() == list(range(1, 135))
    table = rec.table
    for name in compute.THERMO_PROPERTIES:
        assert table[name][:64].tobytes() == first[name].tobytes()  # (rows survive the growth)
    e = table["kinetic_energy"] + table["potential_energy"]
    assert np.abs(e - e[0]).max() < 1e-2 * np.abs(table["kinetic_energy"]).max()  # NVE: the recorded total energy holds to 1 %


# ---------------------------------------------------------------------------------------------------------------------
# 6. decomposed
# ---------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dd_snapshot():
    import azplugins_amd as azp

    cfg = syn.config_tpm(10, 10, 20)
    n = cfg["xyz"].shape[0]
    tag = np.arange(n, dtype=np.uint64)
    typeid = (syn.hash64(7, tag, 3) % np.uint64(2)).astype(np.int64)
    inertia = np.stack([0.1 + 0.1 * syn.u01(8, tag, c) for c in range(3)], axis=1) * (syn.u01(9, tag, 0) > 0.25)[:, None]
    snap = azp.Snapshot.from_arrays(cfg["xyz"], cfg["L"], typeid=typeid, types=("A", "B"), velocity=_velocities(n, 61, kT=2.0),
                                    orientation=cfg["orientation"], moment_inertia=inertia,
                                    angmom=np.stack([syn.normal(10, tag, c) for c in range(4)], axis=1))
    snap.particles.mass[:] = 0.5 + 1.5 * syn.u01(11, tag, 0)
    return snap, cfg


def _dd_integrator(azp, cfg):
    nl = azp.nlist.Cell(buffer=cfg["r_buff"])
    pot = azp.pair.TwoPatchMorse(nlist=nl, default_r_cut=cfg["r_cut"], mode="shift")
    for pair in (("A", "A"), ("A", "B"), ("B", "B")):
        pot.params[pair] = cfg["params"]
    return azp.Integrator(dt=0.004, forces=[pot], methods=[azp.ConstantVolume()], integrate_rotational_dof=True)


def _dd_thermos(azp):
    from azplugins_amd import compute

    return {"All": compute.ThermodynamicQuantities(azp.All()), "B": compute.ThermodynamicQuantities(azp.Type(["B"]))}


def _flat(thermo):
    from azplugins_amd import compute

    return np.concatenate([np.atleast_1d(np.asarray(getattr(thermo, name), dtype=np.float64)) for name in compute.THERMO_PROPERTIES])


def _dd_worker(rank, world, port, out_dir):
    import torch
    import torch.distributed as dist

    import azplugins_amd as azp
    from azplugins_amd import compute
    from azplugins_amd import decomposition as dd

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    snap, cfg = _dd_snapshot()
    dec = dd.Decomposition(cfg["L"], world, cfg["r_cut"] + cfg["r_buff"])
    local, n_global, topology = dd.distribute_snapshot(snap if rank == 0 else None, dec, root=0, device="cuda:0")
    sim, dom = dd.rank_simulation_from_snapshot(local, n_global, dec, rank, "cuda:0", seed=1, topology=topology)
    sim.operations.integrator = _dd_integrator(azp, cfg)
    thermos = _dd_thermos(azp)
    for t in thermos.values():
        sim.operations.add(t)
    rec = compute.ThermodynamicRecorder(thermos["All"], 1)
    sim.operations.add(rec)
    sim.run(0)
    out = {"prop_" + k: _flat(t) for k, t in thermos.items()}
    sim.run(2)
    table = rec.table
    out["rec_steps"] = rec.timesteps
    out["rec_last"] = np.concatenate([np.atleast_1d(np.asarray(table[name][-1], dtype=np.float64)) for name in compute.THERMO_PROPERTIES])
    out["now"] = _flat(thermos["All"])
    out["n_local"] = np.array([sim.state.N, sim.state.n_ghost])
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)
    dist.barrier()
    dist.destroy_process_group()


def test_decomposed_properties_match_single_domain(tmp_path):
    import torch.multiprocessing as mp

    import azplugins_amd as azp
    from azplugins_amd import compute

    world = 2
    mp.spawn(_dd_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    res = [dict(np.load(os.path.join(str(tmp_path), "rank%d.npz" % r))) for r in range(world)]
    for key in res[0]:
        if key != "n_local":
            assert np.array_equal(res[0][key], res[1][key]), "ranks disagree on %s" % key  # every rank gets the same result
    assert all(int(r["n_local"][1]) > 0 for r in res)  # (ghost rows exist and must not be counted)
    snap, cfg = _dd_snapshot()
    n = snap.particles.N
    assert sum(int(r["n_local"][0]) for r in res) == n
    assert res[0]["rec_steps"].tolist() == [1, 2]
    assert np.array_equal(res[0]["rec_last"], res[0]["now"])  # the recorder's reduced row is the properties' row

    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(snap)
    sim.operations.tuners.clear()
    sim.operations.integrator = _dd_integrator(azp, cfg)
    thermos = _dd_thermos(azp)
    for t in thermos.values():
        sim.operations.add(t)
    sim.run(0)
    st = sim.state
    V = float(np.prod(cfg["L"]))
    f = sim.operations.integrator.forces[0]
    eps = ref.REL_BOUND
    for key, thermo in thermos.items():
        sel = np.ones(n, bool) if key == "All" else st.typeid_host == 1
        _, mag = ref.exact(ref.terms(st.vel[:n].cpu().numpy(), sel, [f._force.cpu().numpy()], [f._virial.cpu().numpy()],
                                     st.orientation[:n].cpu().numpy(), st.angmom[:n].cpu().numpy(), st.inertia[:n].cpu().numpy()))
        ke_t = 0.5 * (mag[4] + mag[7] + mag[9])
        dof = thermo.degrees_of_freedom
        # the slots each property is made of, bounded by 256 * 2^-53 * sum |term| (the ranks re-associate the sum)
        bound = dict(num_particles=0.0, volume=0.0, translational_degrees_of_freedom=0.0, rotational_degrees_of_freedom=0.0,
                     degrees_of_freedom=0.0, translational_kinetic_energy=eps * ke_t, rotational_kinetic_energy=eps * mag[17],
                     kinetic_energy=eps * (ke_t + mag[17]), potential_energy=eps * mag[16],
                     kinetic_temperature=2.0 * eps * (ke_t + mag[17]) / dof,
                     pressure_tensor=np.array([eps * (mag[4 + c] + mag[10 + c]) / V for c in range(6)]),
                     pressure=eps * (mag[4] + mag[7] + mag[9] + mag[10] + mag[13] + mag[15]) / (3.0 * V),
                     linear_momentum=np.array([eps * mag[1 + c] for c in range(3)]))
        want = _flat(thermo)
        got = res[0]["prop_" + key]
        tol = np.concatenate([np.atleast_1d(np.asarray(bound[name], dtype=np.float64)) for name in compute.THERMO_PROPERTIES])
        err = np.abs(got - want)
        print("decomposed %s: |err| / bound:" % key, np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), err))
        assert got.shape == want.shape and np.all(err <= tol), (key, err, tol)
        assert thermo.rotational_degrees_of_freedom > 0 and thermo.num_particles == int(sel.sum())
