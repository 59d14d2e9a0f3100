"""compute.ThermodynamicField in a domain-decomposed run (the pattern of tests/test_gpu_rdf_domain.py: two processes on
one GPU, gloo for the collectives): a PerturbedLJ liquid, a 3 x 2 x 2 Cartesian field that tiles the box. Each rank sums
its own particles bin by bin; the rows are added over the ranks.

On the INITIAL state (the only one the two runs share bit for bit) the counts equal the single-domain run's exactly
and the floating slots agree within twice the single-domain bound: a bin's sum is tree(members on rank 0) +
tree(members on rank 1) instead of one tree over all of them, each within its own bound of the exact sum of the same
terms. The kinematic slots (M, P, K) are compared with the single-domain field itself. A rank adds the pair terms of a
particle's force in another order than the single-domain run does, so its per-particle virials and energies are not
the same words: the slots W and U are compared with the restated single-domain tree over the per-particle values the
ranks themselves hold, which is the statement about this compute."""

import os
import socket

import numpy as np
import pytest

import thermo_field_ref as ref

from azplugins_amd import synthetic as syn

pytestmark = pytest.mark.gpu

NUM_BINS = (3, 2, 2)
STEPS = 10


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


def _grid(cfg):
    L = [float(x) for x in cfg["L"]]
    return NUM_BINS, tuple(-0.5 * x for x in L), tuple(0.5 * x for x in L)


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
    field = compute.CartesianThermodynamicField(*_grid(cfg), streaming="keep")
    rec = compute.ThermodynamicFieldRecorder(field, 5)
    sim.operations.add(field)
    sim.operations.writers.append(rec)
    sim.run(0)
    row0 = field.sums  # (collective: every rank reads it)
    pressure0 = field.pressure
    st = sim.state
    N = st.N
    force = sim.operations.integrator.forces[0]
    mine = dict(tag=st.tag[:N].cpu().numpy().view(np.uint32), pos=st.pos[:N, :3].cpu().numpy(), vel=st.vel[:N].cpu().numpy(),
                force=force._force[:N].cpu().numpy(), virial=force._virial.cpu().numpy()[:, :N], n_ghost=np.array([st.n_ghost]))
    sim.run(STEPS)
    calls = []
    reduce_sum = compute._all_reduce_sum
    compute._all_reduce_sum = lambda d, rows: (calls.append(tuple(rows.shape)), reduce_sum(d, rows))[1]
    table = rec.table
    compute._all_reduce_sum = reduce_sum
    torch.cuda.synchronize()
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), row0=row0, pressure0=pressure0, table_sums=table["sums"],
             table_counts=table["counts"], steps=rec.timesteps, calls=np.array(calls), **mine)
    dist.barrier()
    dist.destroy_process_group()


def test_decomposed_rows_match_single_domain(tmp_path):
    import torch.multiprocessing as mp

    import azplugins_amd as azp
    from azplugins_amd import compute

    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    cfg = _config()
    n = cfg["xyz"].shape[0]
    grid = _grid(cfg)
    snap = azp.Snapshot.from_arrays(cfg["xyz"], cfg["L"], velocity=cfg["vel"])
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(snap)
    sim.operations.integrator = _integrator(azp, cfg)
    sim.operations.tuners.clear()
    field = compute.CartesianThermodynamicField(*grid, streaming="keep")
    sim.operations.add(field)
    sim.run(0)
    single = field.sums.reshape(12, 19)
    ranks = [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in range(world)]
    assert np.array_equal(ranks[0]["row0"], ranks[1]["row0"]) and np.array_equal(ranks[0]["pressure0"], ranks[1]["pressure0"])
    got = ranks[0]["row0"].reshape(12, 19)
    assert all(int(d["n_ghost"][0]) > 100 for d in ranks)
    # the counts are exact
    assert np.array_equal(got[:, 0], single[:, 0]) and np.array_equal(got[:, 18], single[:, 18]) and got[:, 0].sum() == n
    # the per-particle values the ranks hold, by tag
    tag = np.concatenate([d["tag"] for d in ranks]).astype(np.int64)
    assert np.array_equal(np.sort(tag), np.arange(n))
    pos = np.concatenate([d["pos"] for d in ranks])
    vel = np.concatenate([d["vel"] for d in ranks])
    force = np.concatenate([d["force"] for d in ranks])
    virial = np.concatenate([d["virial"] for d in ranks], axis=1)
    terms = ref.terms(vel, [force], [virial])
    b = ref.bins(pos, ref.CARTESIAN, *grid)
    assert (b >= 0).all()
    want = ref.row(b, tag, None, terms, np.zeros(n, dtype=np.int64), 1, 12)
    assert np.array_equal(want[:, :11].view(np.uint64), single[:, :11].view(np.uint64))  # (the same initial state)
    for k in range(12):
        mag = np.abs(terms[b == k]).sum(axis=0)
        tol = 2.0 * ref.bound(mag, int((b == k).sum()), 1)
        err = np.abs(got[k, :18] - want[k, :18])
        print("bin %d: worst error / tolerance %.3g" % (k, (err[1:] / tol[1:]).max()))
        assert (err <= tol).all(), (k, err, tol)
        assert (np.abs(got[k, 1:11] - single[k, 1:11]) <= tol[1:11]).all()
    assert np.abs(got[:, 11:18]).min() > 0.0
    # the recorder: the rows of all ranks are added in one reduction, and every rank gets the same table
    for d in ranks:
        assert d["steps"].tolist() == [5, 10] and d["calls"].tolist() == [[2, 12 * 19]]
        assert d["table_sums"].shape == (2, 3, 2, 2, 19) and d["table_counts"].sum(axis=(1, 2, 3, 4)).tolist() == [n, n]
    assert np.array_equal(ranks[0]["table_sums"], ranks[1]["table_sums"])
