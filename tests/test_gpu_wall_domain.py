"""A wall potential in a domain-decomposed run (the pattern of tests/test_gpu_domain.py: two processes on one GPU,
gloo for the collectives): a PerturbedLJ liquid in a two-plane LJ93 slit, the planes across the axis the two ranks
split, so each rank holds one of them. Positions and velocities after 20 NVE steps equal the single-domain run's to
the tolerance test_gpu_domain.py uses for its PerturbedLJ case; ``wall_forces`` is the same on both ranks and equals the
single-domain value."""

import os
import socket

import numpy as np
import pytest

from azplugins_amd import synthetic as syn

pytestmark = pytest.mark.gpu

# 4 x the float64 deviation measured on the fixture: see tests/test_gpu_wall.py
BOUND = 4.0 * 1.790e-15
STEPS = 20


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _config():
    cfg = syn.config_plj_sc(12)  # 1728 particles
    n = cfg["xyz"].shape[0]
    tag = np.arange(n, dtype=np.uint64)
    v = np.stack([syn.normal(51, tag, c) for c in range(3)], axis=1) * np.sqrt(1.5)
    cfg["vel"] = v - v.mean(axis=0)
    cfg["dt"] = 0.005
    return cfg


def _walls(azp, cfg, which=(0, 1)):
    """The slit: planes one length inside the faces in x. Extrapolated below 0.8, so the particles of the periodic
    liquid that start behind or on a plane feel a finite push into the slit."""
    h = 0.5 * float(cfg["L"][0])
    planes = [azp.wall.Plane(origin=(-h + 1.0, 0, 0), normal=(1, 0, 0)), azp.wall.Plane(origin=(h - 1.0, 0, 0), normal=(-1, 0, 0))]
    wall = azp.wall.LJ93([planes[k] for k in which], mode="shift")
    wall.params["A"] = dict(epsilon=1.0, sigma=1.0, r_cut=3.0, r_extrap=0.8)
    return wall


def _integrator(azp, cfg, nl):
    pot = azp.pair.PerturbedLennardJones(nlist=nl, default_r_cut=cfg["r_cut"], mode="shift")
    pot.params[("A", "A")] = cfg["params"]
    wall = _walls(azp, cfg)
    return wall, azp.Integrator(dt=cfg["dt"], forces=[pot, wall], methods=[azp.ConstantVolume()])


def _worker(rank, world, port, out_dir):
    import torch
    import torch.distributed as dist

    import azplugins_amd as azp
    from azplugins_amd import decomposition as dd

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    cfg = _config()
    dec = dd.Decomposition(cfg["L"], world, cfg["r_cut"] + cfg["r_buff"])
    sim, dom = dd.rank_simulation(cfg, dec, rank, "cuda:0", seed=1)
    nl = azp.nlist.Cell(buffer=cfg["r_buff"])
    wall, sim.operations.integrator = _integrator(azp, cfg, nl)
    sim.run(0)
    wf0 = wall.wall_forces  # (collective: every rank reads it)
    sim.run(STEPS)
    wf1 = wall.wall_forces
    torch.cuda.synchronize()
    st = sim.state
    N = st.N
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), tag=st.tag[:N].cpu().numpy().view(np.uint32), pos=st.pos[:N, :3].cpu().numpy(),
             vel=st.vel[:N, :3].cpu().numpy(), wf0=wf0, wf1=wf1, grid=np.array(dec.grid), n_wall=np.array([np.count_nonzero(wall.energies)]))
    dist.barrier()
    dist.destroy_process_group()


def test_decomposed_run_with_walls_matches_single_domain(tmp_path):
    import torch
    import torch.multiprocessing as mp

    import azplugins_amd as azp

    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    cfg = _config()
    n = cfg["xyz"].shape[0]
    snap = azp.Snapshot.from_arrays(cfg["xyz"], cfg["L"], velocity=cfg["vel"])
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(snap)
    nl = azp.nlist.Cell(buffer=cfg["r_buff"])
    wall, sim.operations.integrator = _integrator(azp, cfg, nl)
    sim.operations.tuners.clear()
    sim.run(0)
    ref_wf0 = wall.wall_forces
    # sum_i |F_i^(w)| of each wall at the initial state, from a single-wall object
    totals = []
    for k in (0, 1):
        one = _walls(azp, cfg, which=(k,))
        s1 = azp.Simulation(device="cuda:0", seed=1)
        s1.create_state_from_snapshot(snap)
        s1.operations.integrator = azp.Integrator(dt=0.0, forces=[one])
        s1.run(0)
        totals.append(float(np.linalg.norm(one.forces, axis=1).sum()))
        assert np.count_nonzero(one.energies) > 100
    sim.run(STEPS)
    torch.cuda.synchronize()
    tag = sim.state.tag.cpu().numpy().view(np.uint32).astype(np.int64)
    ref_pos = np.zeros((n, 3))
    ref_vel = np.zeros((n, 3))
    ref_pos[tag] = sim.state.pos[:, :3].cpu().numpy()
    ref_vel[tag] = sim.state.vel[:, :3].cpu().numpy()
    got_pos = np.full((n, 3), np.nan)
    got_vel = np.full((n, 3), np.nan)
    ranks = [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in range(world)]
    for d in ranks:
        got_pos[d["tag"].astype(np.int64)] = d["pos"]
        got_vel[d["tag"].astype(np.int64)] = d["vel"]
        assert int(d["n_wall"][0]) > 100      # every rank has particles at a wall
        assert tuple(d["grid"]) == (2, 1, 1)  # the ranks split x: one plane each
    L = np.asarray(cfg["L"])
    dx = got_pos - ref_pos
    dx -= L * np.round(dx / L)
    assert np.all(np.isfinite(got_pos)) and np.abs(dx).max() < 1e-9, np.abs(dx).max()
    assert np.abs(got_vel - ref_vel).max() < 1e-8 * max(1.0, np.abs(ref_vel).max())
    # the wall forces: the same on both ranks, before and after the run
    assert np.array_equal(ranks[0]["wf0"], ranks[1]["wf0"]) and np.array_equal(ranks[0]["wf1"], ranks[1]["wf1"])
    # and the single-domain value within the bound, on the state both runs share bit for bit (the initial one: after
    # the run the positions agree to 1e-9 only, which the steep wall force turns into far more than the bound)
    got = ranks[0]["wf0"]
    assert got.shape == (2, 3) and abs(got[0, 0]) > 1.0 and abs(got[1, 0]) > 1.0
    for k in (0, 1):
        print("wall %d: decomposed %r single %r, sum |F| %.6g" % (k, got[k], ref_wf0[k], totals[k]))
        assert np.all(np.abs(got[k] - ref_wf0[k]) <= BOUND * totals[k])
    # after the run they still agree as closely as the trajectories do
    ref_wf1 = wall.wall_forces
    assert np.abs(ranks[0]["wf1"] - ref_wf1).max() < 1e-6 * max(totals)
