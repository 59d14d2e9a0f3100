"""pair.Table against the analytic potential it tabulates, on the north-star liquid (N = 2^20 jittered FCC, rho* = 0.8,
r_cut = 3.0, buffer 0.4): PerturbedLJ (epsilon = sigma = 1, lambda = 0.5) as pair.PerturbedLennardJones and as pair.Table
at widths 256, 1024 and 4096 on [0.8, 3.0). Tile kernel (plan compiled from the cells, static list) and generic kernel,
HIP events around --inner launches after a run-in, the potentials taking turns --reps times; medians and the ratio to the
analytic kernel. Rows for DESIGN 4.21 / profiles/pair_table.md.

    python tools/pair_table_probe.py [--side 64] [--reps 7] [--inner 20] [--widths 256 1024 4096]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import azplugins_amd as azp
from azplugins_amd import synthetic as syn

ap = argparse.ArgumentParser()
ap.add_argument("--side", type=int, default=64)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--inner", type=int, default=20)
ap.add_argument("--settle-ms", type=float, default=80.0)
ap.add_argument("--widths", type=int, nargs="*", default=[256, 1024, 4096])
args = ap.parse_args()

R_MIN, R_CUT = 0.8, 3.0
cfg = syn.config_north_star(args.side)
N = cfg["xyz"].shape[0]
lam = cfg["params"]["attraction_scale_factor"]


def plj(r):
    """U and F = -dU/dr of PerturbedLJ with epsilon = sigma = 1 (mode "none")."""
    r6 = r ** -6.0
    core = r < 2.0 ** (1.0 / 6.0)
    scale = np.where(core, 1.0, lam)
    return scale * 4.0 * (r6 * r6 - r6) + np.where(core, 1.0 - lam, 0.0), scale * 4.0 * (12.0 * r6 * r6 - 6.0 * r6) / r


def make(width):
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(azp.Snapshot.from_arrays(cfg["xyz"], cfg["L"]))
    nl = azp.nlist.Cell(buffer=cfg["r_buff"])
    if width is None:
        pot = azp.pair.PerturbedLennardJones(nlist=nl, default_r_cut=R_CUT)
        pot.params[("A", "A")] = cfg["params"]
    else:
        pot = azp.pair.Table(nlist=nl, default_r_cut=R_CUT)
        U, F = plj(R_MIN + (R_CUT - R_MIN) / width * np.arange(width))
        pot.params[("A", "A")] = dict(r_min=R_MIN, U=U, F=F)
    sim.operations.integrator = azp.Integrator(dt=0.005, forces=[pot])
    sim.run(0)
    return sim, nl, pot


def settle(pot, ms):
    # the chip's power controller cuts the clock 1-4 ms into a burst and recovers over ~50 ms
    # (profiles/r03_clock_transient.md): time at the sustained clock, as bench.py does
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < ms:
        for _ in range(20):
            pot.compute(0)
        torch.cuda.synchronize()


def timed(pot):
    settle(pot, args.settle_ms)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.inner):
        pot.compute(0)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.inner


names = ["analytic"] + ["width %d" % w for w in args.widths]
runs = [make(None)] + [make(w) for w in args.widths]
mean_n = runs[0][1].n_pairs / N
print("N=%d <n>=%.1f reps=%d inner=%d" % (N, mean_n, args.reps, args.inner))
f_ref = runs[0][2].force_tensor.clone()
for kernel in ("tile", "generic"):
    for _, _, pot in runs:
        pot.use_plan = kernel == "tile"
        pot.compute(0)
    times = {n: [] for n in names}
    for _ in range(args.reps):
        for n, (_, _, pot) in zip(names, runs):
            times[n].append(timed(pot))
    base = float(np.median(times["analytic"]))
    for n, (_, _, pot) in zip(names, runs):
        t = np.array(times[n])
        err = float((pot.force_tensor[:, :3] - f_ref[:, :3]).abs().max() / f_ref[:, :3].abs().max())
        launch = azp._lib.last_launch() if n == names[-1] else None
        print("%-8s %-11s median %.4f ms (min %.4f, max %.4f)  x%.3f of analytic  max|f - f_analytic|/max|f| = %.1e%s"
              % (kernel, n, np.median(t), t.min(), t.max(), np.median(t) / base, err,
                 "  last launch %s" % launch if launch else ""))
