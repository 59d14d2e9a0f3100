"""Dihedrals in a domain-decomposed run: two ranks (two processes on one GPU, gloo for the collectives, as in
tests/test_gpu_angle_domain.py) run chains of 8 with PerturbedLJ, DoubleWell bonds, angle.Harmonic and
dihedral.Periodic. The box is 24 lattice cells long in x, so the rank face cuts every second chain in the middle:
dihedrals cross it, the dihedral table is rebuilt from the topology by tag after every migration, and the run must end
where the single-domain run ends (by tag). With a ghost shell that holds two bond lengths but not three, the far member
of such a dihedral is missing and the documented error is raised before anything is computed."""

import os
import socket

import numpy as np
import pytest

from azplugins_amd import synthetic as syn

pytestmark = pytest.mark.gpu

ANGLE_PARAMS = dict(k=5.0, t0=2.6)
DIHEDRAL_PARAMS = dict(k=0.5, d=1, n=1, phi0=0.0)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _config(narrow):
    cfg = syn.config_chains(24, 16, 16, 8)
    n = cfg["xyz"].shape[0]
    tag = np.arange(n, dtype=np.uint64)
    v = np.stack([syn.normal(71, tag, c) for c in range(3)], axis=1) * np.sqrt(1.2)
    cfg["vel"] = v - v.mean(axis=0)
    # Bonds that cannot grow past 1.35: DoubleWell minima at r_0 = 1.0 and 2 r_1 - r_0 = 1.25, b = r_1 - r_0 = 0.125, and
    # U(1.35) = U_1 ((1.35 - 1.125)^2 - b^2)^2 / b^4 = 4 (0.050625 - 0.015625)^2 / 0.00024414 = 20.07, seventeen times the
    # kT = 1.2 the velocities are drawn at. Three of them reach 3 x 1.35 = 4.05 at most, inside the shell of
    # r_cut + r_buff = 3.5 + 0.6 = 4.1. (The bonds of tests/test_gpu_angle_domain.py reach 1.7: three of them, 5.1, do not
    # fit its 3.8 shell.) The curvature at the minima, 8 U_1 / b^2 = 2048, gives omega dt = 0.18 at dt = 0.004.
    cfg["bond_params"] = dict(r_0=1.0, r_1=1.125, U_1=4.0, U_tilt=0.0)
    # narrow: the chains start straight along x with bonds between 0.97 and 1.19 (the lattice constant 1.077 and its
    # jitter), so a shell of 2.5 holds the bead two bonds away (2.38 at most) and not the one three bonds away (2.9 at least)
    cfg["r_cut"], cfg["r_buff"] = (2.3, 0.2) if narrow else (3.5, 0.6)
    cfg["steps"] = 80
    cfg["dt"] = 0.004
    # angles and dihedrals along the chains: consecutive bonds that share a bead
    b = np.asarray(cfg["bonds"], dtype=np.int64)
    second = {int(x): int(y) for x, y in b}
    cfg["angles"] = np.array([(x, y, second[y]) for x, y in b.tolist() if y in second])
    cfg["dihedrals"] = np.array([(x, y, z, second[z]) for x, y, z in cfg["angles"].tolist() if z in second])
    assert cfg["angles"].shape[0] == n // 8 * 6 and cfg["dihedrals"].shape[0] == n // 8 * 5
    return cfg


def _integrator(azp, cfg, nl):
    pot = azp.pair.PerturbedLennardJones(nlist=nl, default_r_cut=cfg["r_cut"], mode="shift")
    pot.params[("A", "A")] = cfg["params"]
    dw = azp.bond.DoubleWell()
    dw.params["A-A"] = cfg["bond_params"]
    ha = azp.angle.Harmonic()
    ha.params["A-A-A"] = ANGLE_PARAMS
    pd = azp.dihedral.Periodic()
    pd.params["A-A-A-A"] = DIHEDRAL_PARAMS
    return pot, pd, azp.Integrator(dt=cfg["dt"], forces=[pot, dw, ha, pd], methods=[azp.ConstantVolume()])


def _snapshot(azp, cfg):
    return azp.Snapshot.from_arrays(cfg["xyz"], cfg["L"], velocity=cfg["vel"], bonds=cfg["bonds"], angles=cfg["angles"],
                                    dihedrals=cfg["dihedrals"])


def _worker(rank, world, port, out_dir, narrow):
    import torch
    import torch.distributed as dist

    import azplugins_amd as azp
    from azplugins_amd import decomposition as dd

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    cfg = _config(narrow)
    dec = dd.Decomposition(cfg["L"], world, cfg["r_cut"] + cfg["r_buff"])
    assert dec.grid == (2, 1, 1)
    snap = _snapshot(azp, cfg) if rank == 0 else None
    local, n_global, topology = dd.distribute_snapshot(snap, dec, root=0, device="cuda:0")
    assert set(topology) == {"bond_tags", "bond_typeid", "bond_types", "angle_tags", "angle_typeid", "angle_types",
                             "dihedral_tags", "dihedral_typeid", "dihedral_types"}
    error = ""
    try:
        sim, dom = dd.rank_simulation_from_snapshot(local, n_global, dec, rank, "cuda:0", seed=1, topology=topology)
    except azp.AzpError as e:
        error = str(e)
    # the ranks agree on whether anyone failed before the first collective of the run
    failed = torch.tensor([1 if error else 0])
    dist.all_reduce(failed)
    if int(failed) == 0:
        nl = azp.nlist.Cell(buffer=cfg["r_buff"])
        pot, pd, sim.operations.integrator = _integrator(azp, cfg, nl)
        sim.run(cfg["steps"])
        torch.cuda.synchronize()
        st = sim.state
        N = st.N
        # dihedrals whose members sit on both sides of the face, as this rank sees them now
        g = st.dihedral_group.astype(np.int64)
        crossing = int(((g < N).any(axis=1) & (g >= N).any(axis=1)).sum())
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), tag=st.tag[:N].cpu().numpy().view(np.uint32), pos=st.pos[:N, :3].cpu().numpy(),
                 vel=st.vel[:N, :3].cpu().numpy(), rebuilds=np.array([dom.num_rebuilds]), crossing=np.array([crossing]),
                 dihedral_energy=np.array([pd.energy]))
    else:
        with open(os.path.join(out_dir, "rank%d.err" % rank), "w") as f:
            f.write(error)
    dist.barrier()
    dist.destroy_process_group()


def test_decomposed_run_with_dihedrals_matches_single_domain(tmp_path):
    import torch
    import torch.multiprocessing as mp

    import azplugins_amd as azp

    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), False), nprocs=world, join=True)
    cfg = _config(False)
    n = cfg["xyz"].shape[0]
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(_snapshot(azp, cfg))
    nl = azp.nlist.Cell(buffer=cfg["r_buff"])
    pot, pd, sim.operations.integrator = _integrator(azp, cfg, nl)
    sim.operations.tuners.clear()
    sim.run(cfg["steps"])
    torch.cuda.synchronize()
    tag = sim.state.tag.cpu().numpy().view(np.uint32).astype(np.int64)
    ref_pos, ref_vel = np.zeros((n, 3)), np.zeros((n, 3))
    ref_pos[tag] = sim.state.pos[:, :3].cpu().numpy()
    ref_vel[tag] = sim.state.vel[:, :3].cpu().numpy()
    got_pos, got_vel = np.full((n, 3), np.nan), np.full((n, 3), np.nan)
    rebuilds, crossing, energy = [], [], 0.0
    for r in range(world):
        d = np.load(os.path.join(str(tmp_path), "rank%d.npz" % r))
        got_pos[d["tag"].astype(np.int64)] = d["pos"]
        got_vel[d["tag"].astype(np.int64)] = d["vel"]
        rebuilds.append(int(d["rebuilds"][0]))
        crossing.append(int(d["crossing"][0]))
        energy += float(d["dihedral_energy"][0])
    assert min(rebuilds) >= 3, "the run must cross several neighbor-list rebuilds (with migration): %r" % rebuilds
    assert min(crossing) > 50, "dihedrals must cross the rank face: %r" % crossing
    L = np.asarray(cfg["L"])
    dx = got_pos - ref_pos
    dx -= L * np.round(dx / L)
    print("decomposed vs single domain: positions %.3e, velocities %.3e, rebuilds %r, crossing %r"
          % (np.abs(dx).max(), np.abs(got_vel - ref_vel).max(), rebuilds, crossing))
    # the bounds of tests/test_gpu_angle_domain.py
    assert np.all(np.isfinite(got_pos)) and np.abs(dx).max() < 1e-9, np.abs(dx).max()
    assert np.abs(got_vel - ref_vel).max() < 1e-8 * max(1.0, np.abs(ref_vel).max())
    # every dihedral's energy is shared out among its members' owners: the ranks' sums add up to the whole (one dihedral
    # of the 3,840 counted twice or dropped would show at 2.6e-4)
    assert abs(energy - pd.energy) < 1e-6 * abs(pd.energy) and pd.energy > 1.0


def test_ghost_shell_of_two_bonds_but_not_three_raises(tmp_path):
    import torch.multiprocessing as mp

    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), True), nprocs=world, join=True)
    for r in range(world):
        assert not os.path.exists(os.path.join(str(tmp_path), "rank%d.npz" % r))   # nothing was computed
        with open(os.path.join(str(tmp_path), "rank%d.err" % r)) as f:
            msg = f.read()
        # (the angles, two bonds long, were localized before the dihedrals without complaint)
        assert "dihedral" in msg and "narrower than three bond lengths" in msg, msg


def test_attach_domain_needs_the_dihedral_topology_by_tag():
    """As for bonds and angles: a state with index-based dihedrals only cannot be decomposed."""
    import azplugins_amd as azp

    class _Domain:
        names = ["pos", "vel", "tag", "image"]

    xyz = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 1.0, 0.0], [1.0, 1.0, 1.0]])
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(azp.Snapshot.from_arrays(xyz, (10.0, 10.0, 10.0), dihedrals=[(0, 1, 2, 3)]))
    with pytest.raises(azp.AzpError, match="set_global_dihedrals"):
        sim.attach_domain(_Domain())
