"""compute.StructureFactor in a domain-decomposed run (the pattern of tests/test_gpu_rdf_domain.py: two processes on one
GPU, gloo for the collectives): each rank sums its owned particles in the global box, the rows are added over the
ranks. Both ranks return the same amplitudes, and they equal the single-domain ones within the sum of the two bounds
(the single-domain sum's and the sum of the ranks' bounds: the order of the additions differs, nothing else)."""

import os
import socket

import numpy as np
import pytest

import structure_factor_ref as ref

from azplugins_amd import synthetic as syn

pytestmark = pytest.mark.gpu

NUM_BINS = 9


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _config():
    return syn.config_plj_sc(12)  # 1728 particles


def _q_max(cfg):
    return 2.0 * np.pi * 4.5 / float(cfg["L"][0])


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
    rows = {}
    for path in (1, 2):
        sf = compute.StructureFactor(azp.All(), azp.All(), _q_max(cfg), NUM_BINS)
        sf.path = path
        sim.operations.add(sf)
        rows[path] = sf._read("row")  # (collective: every rank reads it)
        s = sf.structure_factor
    torch.cuda.synchronize()
    st = sim.state
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), row1=rows[1], row2=rows[2], s=s, n_own=np.array([st.N]),
             n_ghost=np.array([st.n_ghost]))
    dist.barrier()
    dist.destroy_process_group()


def test_decomposed_amplitudes_equal_single_domain():
    import tempfile

    import torch.multiprocessing as mp

    import azplugins_amd as azp
    from azplugins_amd import compute

    world = 2
    with tempfile.TemporaryDirectory() as tmp:
        mp.spawn(_worker, args=(world, _free_port(), tmp), nprocs=world, join=True)
        ranks = [dict(np.load(os.path.join(tmp, "rank%d.npz" % r))) for r in range(world)]
    cfg = _config()
    n = cfg["xyz"].shape[0]
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(azp.Snapshot.from_arrays(cfg["xyz"], cfg["L"]))
    box = (tuple(float(x) for x in cfg["L"]), (0.0, 0.0, 0.0))
    owned = [int(d["n_own"][0]) for d in ranks]
    assert sum(owned) == n and min(owned) > 0 and all(int(d["n_ghost"][0]) > 100 for d in ranks)
    for path in (1, 2):
        sf = compute.StructureFactor(azp.All(), azp.All(), _q_max(cfg), NUM_BINS)
        sf.path = path
        sim.operations.add(sf)
        single = sf._read("row")
        m = sf.vectors
        nv = len(m)
        key = "row%d" % path
        assert np.array_equal(ranks[0][key].view(np.int64), ranks[1][key].view(np.int64))  # the ranks agree bit for bit
        got = ranks[0][key]
        assert tuple(got[4 * nv:]) == (n, n, n, 0.0) == tuple(single[4 * nv:])
        b = ref.bound(m, n, ref.depth(n, nv), box) + sum(ref.bound(m, k, ref.depth(k, nv), box) for k in owned)
        err = np.abs(got[:4 * nv] - single[:4 * nv])
        print("path %d: worst difference %.3g, %.3g of the bound" % (path, err.max(), (err / np.tile(b, 4)).max()))
        assert np.all(err <= np.tile(b, 4)) and np.abs(single[:nv]).max() > 1.0
        # and the reference, within the ranks' bound
        re, im = ref.amplitudes(cfg["xyz"], box, m)
        rb = sum(ref.bound(m, k, ref.depth(k, nv), box) for k in owned)
        assert np.all(np.abs(got[:nv] - re) <= rb) and np.all(np.abs(got[nv:2 * nv] - im) <= rb)
    assert np.array_equal(ranks[0]["s"], ranks[1]["s"], equal_nan=True)
    assert np.allclose(ranks[0]["s"], sf.structure_factor, rtol=1e-9, atol=1e-12, equal_nan=True)
