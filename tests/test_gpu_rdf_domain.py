"""compute.RadialDistributionFunction in a domain-decomposed run (the pattern of tests/test_gpu_wall_domain.py: two
processes on one GPU, gloo for the collectives): a PerturbedLJ liquid, r_max = r_cut. Each rank counts its own
particles against its own particles and ghosts; the rows are added over the ranks.

Exact equality with the single-domain counts is asserted on the INITIAL state, the only one the two runs share bit
for bit (after 20 steps their positions agree to 1e-9, as in the wall test). After the 20 steps the decomposed counts
are compared, exactly, with the numpy reference on the positions the ranks themselves hold: that is the check that
the ghosts still cover r_max after the particles have drifted."""

import os
import socket

import numpy as np
import pytest

import rdf_fixtures as fx
import rdf_ref

from azplugins_amd import synthetic as syn

pytestmark = pytest.mark.gpu

STEPS = 20
NUM_BINS = 60


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
    v = np.stack([syn.normal(52, tag, c) for c in range(3)], axis=1) * np.sqrt(1.5)
    cfg["vel"] = v - v.mean(axis=0)
    cfg["dt"] = 0.005
    return cfg


def _integrator(azp, cfg):
    pot = azp.pair.PerturbedLennardJones(nlist=azp.nlist.Cell(buffer=cfg["r_buff"]), default_r_cut=cfg["r_cut"], mode="shift")
    pot.params[("A", "A")] = cfg["params"]
    return azp.Integrator(dt=cfg["dt"], forces=[pot], methods=[azp.ConstantVolume()])


def _worker(rank, world, port, out_dir):
    import torch
    import torch.distributed as dist

    import azplugins_amd as azp
    from azplugins_amd import compute
    from azplugins_amd import decomposition as dd

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    cfg = _config()
    dec = dd.Decomposition(cfg["L"], world, cfg["r_cut"] + cfg["r_buff"])
    sim, dom = dd.rank_simulation(cfg, dec, rank, "cuda:0", seed=1)
    sim.operations.integrator = _integrator(azp, cfg)
    rdf = compute.RadialDistributionFunction(azp.All(), azp.All(), cfg["r_cut"], NUM_BINS)
    sim.operations.add(rdf)
    sim.run(0)
    row0 = rdf._read("row")  # (collective: every rank reads it)
    g0 = rdf.rdf
    # beyond the ghost coverage r_ghost - buffer = 3.0: refused on every rank, ahead of the collective
    far = compute.RadialDistributionFunction(azp.All(), azp.All(), cfg["r_cut"] + 0.2, NUM_BINS)
    sim.operations.add(far)
    try:
        far.counts
        refused = ""
    except azp.AzpError as e:
        refused = str(e)
    sim.run(STEPS)
    row1 = rdf._read("row")
    torch.cuda.synchronize()
    st = sim.state
    N = st.N
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), tag=st.tag[:N].cpu().numpy().view(np.uint32), pos=st.pos[:N, :3].cpu().numpy(),
             row0=row0, row1=row1, g0=g0, refused=np.array([refused]), n_ghost=np.array([st.n_ghost]), grid=np.array(dec.grid))
    dist.barrier()
    dist.destroy_process_group()


def test_decomposed_counts_equal_single_domain(tmp_path):
    import torch.multiprocessing as mp

    import azplugins_amd as azp
    from azplugins_amd import compute

    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    cfg = _config()
    n = cfg["xyz"].shape[0]
    snap = azp.Snapshot.from_arrays(cfg["xyz"], cfg["L"], velocity=cfg["vel"])
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(snap)
    sim.operations.integrator = _integrator(azp, cfg)
    sim.operations.tuners.clear()
    rdf = compute.RadialDistributionFunction(azp.All(), azp.All(), cfg["r_cut"], NUM_BINS)
    sim.operations.add(rdf)
    sim.run(0)
    single = rdf._read("row")
    ranks = [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in range(world)]
    for d in ranks:
        assert int(d["n_ghost"][0]) > 100 and tuple(d["grid"]) == (2, 1, 1)
        # the initial state: the decomposed row is the single-domain row, on every rank
        assert np.array_equal(d["row0"], single)
        assert np.array_equal(d["g0"], rdf.rdf)
        msg = str(d["refused"][0])
        assert "3.4" in msg and "0.4" in msg and "ghost" in msg, msg
    assert tuple(single[NUM_BINS:]) == (n, n, n, 0) and single[:NUM_BINS].sum() > 80 * n
    # after the run: the ranks agree, and the row is the reference's on the positions they hold
    assert np.array_equal(ranks[0]["row1"], ranks[1]["row1"])
    pos = np.full((n, 3), np.nan)
    for d in ranks:
        pos[d["tag"].astype(np.int64)] = d["pos"]
    assert np.all(np.isfinite(pos))
    box = (tuple(cfg["L"]), fx.ORTHO, fx.PBC)
    types = np.zeros(n, dtype=np.int64)
    assert rdf_ref.edge_pairs(pos, types, box, None, None, cfg["r_cut"], NUM_BINS) == 0
    assert np.array_equal(ranks[0]["row1"], rdf_ref.counts(pos, types, box, None, None, cfg["r_cut"], NUM_BINS))
    assert not np.array_equal(ranks[0]["row1"], single)  # (the liquid moved)
