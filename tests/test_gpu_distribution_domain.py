"""compute.BondedDistribution in a domain-decomposed run: two ranks (two processes on one GPU, gloo for the collectives,
as in tests/test_gpu_angle_domain.py, with its chain configuration cut down to 24 x 8 x 8 cells: 192 chains of 8) run
40 steps with PerturbedLJ, DoubleWell bonds and angle.Harmonic. Every group is counted by the rank that owns its first
member, the rows are added over the ranks, and the angle and bond counts on each rank must EQUAL the single-domain
run's.

The two trajectories agree to 1e-9, not to the bit, so the comparison is guarded twice on the reference
(tests/distribution_ref.py) alone: every group's index lies at least 1e-9 from an integer in the single-domain end
state, and the reference counts of the decomposed end state (gathered by tag) are those of the single-domain end state
-- no coordinate changed its bin between the two trajectories."""

import os

import numpy as np
import pytest

import distribution_ref as R
import test_gpu_angle_domain as base
from azplugins_amd import synthetic as syn

pytestmark = pytest.mark.gpu

STEPS = 40
NUM_BINS = 32
BOND_RANGE = dict(r_min=0.8, r_max=1.6)


def _config():
    cfg = syn.config_chains(24, 8, 8, 8)
    n = cfg["xyz"].shape[0]
    tag = np.arange(n, dtype=np.uint64)
    v = np.stack([syn.normal(71, tag, c) for c in range(3)], axis=1) * np.sqrt(1.2)
    cfg["vel"] = v - v.mean(axis=0)
    cfg["bond_params"] = dict(r_0=1.0, r_1=1.25, U_1=4.0, U_tilt=0.0)   # (as the angle test: bonds that stay below 1.7)
    cfg["r_cut"], cfg["r_buff"] = 3.2, 0.6
    cfg["dt"] = 0.004
    b = np.asarray(cfg["bonds"], dtype=np.int64)
    second = {int(x): int(y) for x, y in b}
    cfg["angles"] = np.array([(x, y, second[y]) for x, y in b.tolist() if y in second])
    assert n == 1536 and cfg["angles"].shape[0] == n // 8 * 6
    return cfg


def _distributions(compute):
    return (compute.BondedDistribution("angle", NUM_BINS), compute.BondedDistribution("bond", NUM_BINS, **BOND_RANGE))


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
    assert dec.grid == (2, 1, 1)
    snap = base._snapshot(azp, cfg) if rank == 0 else None
    local, n_global, topology = dd.distribute_snapshot(snap, dec, root=0, device="cuda:0")
    sim, dom = dd.rank_simulation_from_snapshot(local, n_global, dec, rank, "cuda:0", seed=1, topology=topology)
    nl = azp.nlist.Cell(buffer=cfg["r_buff"])
    pot, ha, sim.operations.integrator = base._integrator(azp, cfg, nl)
    angles, bonds = _distributions(compute)
    sim.operations.add(angles)
    sim.operations.add(bonds)
    sim.run(STEPS)
    st = sim.state
    N = st.N
    # (each read adds the rows over the ranks: both ranks read in the same order)
    out = dict(angle_counts=angles.counts, angle_groups=angles.num_groups, bond_counts=bonds.counts, bond_outside=bonds.outside,
               bond_groups=bonds.num_groups)
    g = st.angle_group.astype(np.int64)
    crossing = int(((g < N).any(axis=1) & (g >= N).any(axis=1)).sum())
    torch.cuda.synchronize()
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), tag=st.tag[:N].cpu().numpy().view(np.uint32), pos=st.pos[:N, :3].cpu().numpy(),
             crossing=np.array([crossing]), n_local=np.array([N]), **out)
    dist.barrier()
    dist.destroy_process_group()


def _reference(cfg, pos):
    L = tuple(float(x) for x in cfg["L"])
    one = lambda groups: np.zeros(len(groups), dtype=np.int64)
    return (R.histogram("angle", pos, cfg["angles"], one(cfg["angles"]), 1, NUM_BINS, L),
            R.histogram("bond", pos, cfg["bonds"], one(cfg["bonds"]), 1, NUM_BINS, L, **BOND_RANGE))


def test_decomposed_counts_equal_the_single_domain_counts(tmp_path):
    import torch
    import torch.multiprocessing as mp

    import azplugins_amd as azp
    from azplugins_amd import compute

    world = 2
    mp.spawn(_worker, args=(world, base._free_port(), str(tmp_path)), nprocs=world, join=True)
    cfg = _config()
    n = cfg["xyz"].shape[0]
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(base._snapshot(azp, cfg))
    nl = azp.nlist.Cell(buffer=cfg["r_buff"])
    pot, ha, sim.operations.integrator = base._integrator(azp, cfg, nl)
    sim.operations.tuners.clear()
    angles, bonds = _distributions(compute)
    sim.operations.add(angles)
    sim.operations.add(bonds)
    sim.run(STEPS)
    torch.cuda.synchronize()
    tag = sim.state.tag.cpu().numpy().view(np.uint32).astype(np.int64)
    single_pos = np.zeros((n, 3))
    single_pos[tag] = sim.state.pos[:, :3].cpu().numpy()
    ranks = [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in range(world)]
    domain_pos = np.full((n, 3), np.nan)
    for d in ranks:
        domain_pos[d["tag"].astype(np.int64)] = d["pos"]
    assert np.all(np.isfinite(domain_pos)) and sum(int(d["n_local"][0]) for d in ranks) == n
    assert min(int(d["crossing"][0]) for d in ranks) > 20, "angles must cross the rank face"

    # the guards, on the reference alone
    ref_angle, ref_bond = _reference(cfg, single_pos)
    dom_angle, dom_bond = _reference(cfg, domain_pos)
    print("guards: angles %.3e, bonds %.3e" % (R.guard(ref_angle["index"]), R.guard(ref_bond["index"])))
    assert R.guard(ref_angle["index"]) > 1e-9 and R.guard(ref_bond["index"]) > 1e-9
    assert np.array_equal(dom_angle["counts"], ref_angle["counts"]) and np.array_equal(dom_bond["counts"], ref_bond["counts"])
    assert np.array_equal(dom_bond["outside"], ref_bond["outside"])
    assert np.abs(single_pos - cfg["xyz"]).max() > 1e-2           # the chains moved

    # the single-domain compute is the reference's, and every rank holds the same numbers
    assert np.array_equal(angles.counts, ref_angle["counts"]) and np.array_equal(bonds.counts, ref_bond["counts"])
    assert np.array_equal(bonds.outside, ref_bond["outside"])
    assert angles.num_groups.tolist() == [len(cfg["angles"])] and bonds.num_groups.tolist() == [len(cfg["bonds"])]
    for d in ranks:
        assert np.array_equal(d["angle_counts"], ref_angle["counts"]) and np.array_equal(d["bond_counts"], ref_bond["counts"])
        assert np.array_equal(d["bond_outside"], ref_bond["outside"])
        assert d["angle_groups"].tolist() == [len(cfg["angles"])] and d["bond_groups"].tolist() == [len(cfg["bonds"])]
    assert (ref_angle["counts"] > 0).sum() > 5 and (ref_bond["counts"] > 0).sum() > 5
