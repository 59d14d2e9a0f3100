"""The harmonic angle kernel on the C3 topology (N = 1,048,576: 32,768 chains of 32 beads, 983,040 angles) next to the
DoubleWell bond kernel on the same state: time per launch, algorithmic bytes per particle and the share of the HBM peak
they amount to. Every call sits between its own pair of device events and the cases are interleaved.

    python tools/angle_probe.py --reps 200 --warmup 20 --out profiles/angle.md
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import azplugins_amd as azp
from azplugins_amd import synthetic as syn

HBM_PEAK = 8.0e12      # B/s, specification


def chain_angles(bonds):
    """Consecutive bonds that share a bead (the bonds of config_chains run along the chains)."""
    b = np.asarray(bonds, dtype=np.int64)
    nxt = np.full(int(b.max()) + 1, -1, dtype=np.int64)
    nxt[b[:, 0]] = b[:, 1]
    third = nxt[b[:, 1]]
    keep = third >= 0
    return np.stack([b[keep, 0], b[keep, 1], third[keep]], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="1/64 of C3 (a rehearsal size, not a measurement)")
    ap.add_argument("--out", default=None, help="write the report to this file as well")
    ap.add_argument("--skip-virial", action="store_true", help="leave the virial case out (a kernel trace names both harmonic "
                    "cases alike)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("angle_probe: no GPU; nothing is measured without one")

    cfg = syn.config_chains(32, 32, 16, 32) if args.small else syn.config_chains()
    angles = chain_angles(cfg["bonds"])
    N = cfg["xyz"].shape[0]
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(azp.Snapshot.from_arrays(cfg["xyz"], cfg["L"], bonds=cfg["bonds"], angles=angles))
    sim.operations.tuners.clear()
    dw = azp.bond.DoubleWell()
    dw.params["A-A"] = cfg["bond_params"]
    dw.defer_flag_check = True  # (as inside Simulation.run: no host round trip for the flag word behind every launch)
    ha = azp.angle.Harmonic()
    ha.params["A-A-A"] = dict(k=10.0, t0=2.6)
    cs = azp.angle.CosineSquared()
    cs.params["A-A-A"] = dict(k=10.0, t0=2.6)
    hv = azp.angle.Harmonic()
    hv.params["A-A-A"] = dict(k=10.0, t0=2.6)
    sim.operations.integrator = azp.Integrator(dt=0.001, forces=[dw, ha, cs, hv])
    sim.run(0)
    hv.compute_virial = True
    nb = 2.0 * len(cfg["bonds"]) / N
    na = 3.0 * len(angles) / N
    # algorithmic bytes per particle: own position row + entry count + table entries + force row (+ six virial rows);
    # the gathered partner rows are rows some lane of the launch reads as its own, so they are counted once
    cases = [("bond.DoubleWell", dw, 32 + 4 + 12 * nb + 32), ("angle.Harmonic", ha, 32 + 4 + 16 * na + 32),
             ("angle.CosineSquared", cs, 32 + 4 + 16 * na + 32), ("angle.Harmonic, virial", hv, 32 + 4 + 16 * na + 32 + 48)]
    if args.skip_virial:
        cases = cases[:3]
    times = {name: [] for name, _, _ in cases}
    for it in range(args.warmup + args.reps):
        for name, f, _ in cases:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f.compute(0)
            e1.record()
            if it >= args.warmup:
                times[name].append((e0, e1))
    torch.cuda.synchronize()
    lines = ["# The harmonic angle kernel on the C3 topology against the DoubleWell bond kernel", "",
             "Written by `python tools/angle_probe.py --reps %d --warmup %d`." % (args.reps, args.warmup), "",
             "device: %s, N = %d (C3: chains of 32 beads), %d bonds (%.4f table entries per particle), %d angles (%.4f entries "
             "per particle), %d timed calls per case after %d warm-up calls, every call between its own pair of device events, "
             "the cases interleaved. Bytes per particle are algorithmic: the lane's own position row (32 B), its entry count "
             "(4 B), its table entries (12 B per bond entry, 16 B per angle entry), the force row (32 B) and, where the virial "
             "is on, six virial rows (48 B); gathered partner rows are some other lane's own row and are not counted again. "
             "The share of the HBM peak is those bytes over the median time over 8.0 TB/s (specification; a float4 copy "
             "reaches 6.29 TB/s). The arrays of one call (%.0f MB for the angle kernel) fit the 256 MB Infinity Cache, so "
             "these are rates of repeated calls on a resident working set, as inside a run."
             % (torch.cuda.get_device_name(0), N, len(cfg["bonds"]), nb, len(angles), na, args.reps, args.warmup,
                cases[1][2] * N / 1e6), "",
             "| kernel | median us | min | p10 | p90 | max | x bond | B per particle | TB/s | of HBM peak |", "|---|---|---|---|---|---|---|---|---|---|"]
    med_bond = None
    for name, _, nbytes in cases:
        t = np.array([a.elapsed_time(b) * 1e3 for a, b in times[name]])
        med = float(np.median(t))
        med_bond = med if med_bond is None else med_bond
        rate = nbytes * N / (med * 1e-6)
        lines.append("| %s | %.1f | %.1f | %.1f | %.1f | %.1f | %.2f | %.1f | %.2f | %.1f %% |"
                     % (name, med, t.min(), np.percentile(t, 10), np.percentile(t, 90), t.max(), med / med_bond, nbytes, rate / 1e12,
                        100.0 * rate / HBM_PEAK))
    report = "\n".join(lines) + "\n"
    print(report)
    if args.out:
        with open(args.out, "w") as f:
            f.write(report)


if __name__ == "__main__":
    main()
