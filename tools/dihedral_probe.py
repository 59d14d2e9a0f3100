"""The dihedral kernels on the C3 topology (N = 1,048,576: 32,768 chains of 32 beads, 29 dihedrals per chain) next to
the harmonic angle kernel and the DoubleWell bond kernel on the same state: time per launch, algorithmic bytes per
particle, and the ratio of both to the angle kernel of the same run. Every call sits between its own pair of device
events and the cases are interleaved. No time is fixed in advance: the figure to judge is the time ratio to the angle
kernel beside the ratio of algorithmic bytes.

    python tools/dihedral_probe.py --reps 200 --warmup 20 --out profiles/dihedral.md
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


def chain_topology(bonds):
    """Angles and dihedrals of consecutive bonds that share a bead (the bonds of config_chains run along the chains)."""
    b = np.asarray(bonds, dtype=np.int64)
    nxt = np.full(int(b.max()) + 1, -1, dtype=np.int64)
    nxt[b[:, 0]] = b[:, 1]
    third = nxt[b[:, 1]]
    keep = third >= 0
    angles = np.stack([b[keep, 0], b[keep, 1], third[keep]], axis=1)
    fourth = nxt[angles[:, 2]]
    keep = fourth >= 0
    return angles, np.concatenate([angles[keep], fourth[keep, None]], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="1/64 of C3 (a rehearsal size, not a measurement)")
    ap.add_argument("--out", default=None, help="write the report to this file as well")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dihedral_probe: no GPU; nothing is measured without one")

    cfg = syn.config_chains(32, 32, 16, 32) if args.small else syn.config_chains()
    angles, dihedrals = chain_topology(cfg["bonds"])
    N = cfg["xyz"].shape[0]
    assert len(dihedrals) == N // 32 * 29
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(azp.Snapshot.from_arrays(cfg["xyz"], cfg["L"], bonds=cfg["bonds"], angles=angles, dihedrals=dihedrals))
    sim.operations.tuners.clear()
    dw = azp.bond.DoubleWell()
    dw.params["A-A"] = cfg["bond_params"]
    dw.defer_flag_check = True  # (as inside Simulation.run: no host round trip for the flag word behind every launch)
    ha = azp.angle.Harmonic()
    ha.params["A-A-A"] = dict(k=10.0, t0=2.6)

    def periodic():
        f = azp.dihedral.Periodic()
        f.params["A-A-A-A"] = dict(k=2.0, d=-1, n=3, phi0=0.5)
        return f

    def opls():
        f = azp.dihedral.OPLS()
        f.params["A-A-A-A"] = dict(k1=1.5, k2=-0.5, k3=0.8, k4=0.2)
        return f

    pe, op, pev, opv = periodic(), opls(), periodic(), opls()
    sim.operations.integrator = azp.Integrator(dt=0.001, forces=[dw, ha, pe, op, pev, opv])
    sim.run(0)
    pev.compute_virial = opv.compute_virial = True
    nb = 2.0 * len(cfg["bonds"]) / N
    na = 3.0 * len(angles) / N
    nd = 4.0 * len(dihedrals) / N
    # algorithmic bytes per particle (the formula of profiles/angle.md): own position row + entry count + table entries
    # + force row (+ six virial rows); the gathered partner rows are rows some lane of the launch reads as its own, so
    # they are counted once
    cases = [("bond.DoubleWell", dw, 32 + 4 + 12 * nb + 32), ("angle.Harmonic", ha, 32 + 4 + 16 * na + 32),
             ("dihedral.Periodic", pe, 32 + 4 + 16 * nd + 32), ("dihedral.OPLS", op, 32 + 4 + 16 * nd + 32),
             ("dihedral.Periodic, virial", pev, 32 + 4 + 16 * nd + 32 + 48), ("dihedral.OPLS, virial", opv, 32 + 4 + 16 * nd + 32 + 48)]
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
    lines = ["# The dihedral kernels on the C3 topology against the harmonic angle kernel", "",
             "Written by `python tools/dihedral_probe.py --reps %d --warmup %d`." % (args.reps, args.warmup), "",
             "device: %s, N = %d (C3: chains of 32 beads), %d bonds (%.4f table entries per particle), %d angles (%.4f), "
             "%d dihedrals (%.4f), %d timed calls per case after %d warm-up calls, every call between its own pair of device "
             "events, the cases interleaved. Bytes per particle are algorithmic: the lane's own position row (32 B), its entry "
             "count (4 B), its table entries (12 B per bond entry, 16 B per angle or dihedral entry), the force row (32 B) and, "
             "where the virial is on, six virial rows (48 B); gathered partner rows are some other lane's own row and are not "
             "counted again. The share of the HBM peak is those bytes over the median time over 8.0 TB/s (specification). The "
             "arrays of one call (%.0f MB for the dihedral kernel) fit the 256 MB Infinity Cache, so these are rates of repeated "
             "calls on a resident working set, as inside a run."
             % (torch.cuda.get_device_name(0), N, len(cfg["bonds"]), nb, len(angles), na, len(dihedrals), nd, args.reps, args.warmup,
                cases[2][2] * N / 1e6), "",
             "| kernel | median us | min | p10 | p90 | max | x angle (time) | B per particle | x angle (bytes) | TB/s | of HBM peak |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    stats = {}
    for name, _, nbytes in cases:
        t = np.array([a.elapsed_time(b) * 1e3 for a, b in times[name]])
        stats[name] = (float(np.median(t)), t.min(), np.percentile(t, 10), np.percentile(t, 90), t.max(), nbytes)
    med_angle, bytes_angle = stats["angle.Harmonic"][0], stats["angle.Harmonic"][5]
    spread = stats["angle.Harmonic"][3] / stats["angle.Harmonic"][2]
    for name, _, _ in cases:
        med, tmin, p10, p90, tmax, nbytes = stats[name]
        rate = nbytes * N / (med * 1e-6)
        lines.append("| %s | %.1f | %.1f | %.1f | %.1f | %.1f | %.2f | %.1f | %.2f | %.2f | %.1f %% |"
                     % (name, med, tmin, p10, p90, tmax, med / med_angle, nbytes, nbytes / bytes_angle, rate / 1e12, 100.0 * rate / HBM_PEAK))
    lines += ["", "The angle kernel's own spread in this run, p90 / p10, is %.3f." % spread, ""]
    for name in ("dihedral.Periodic", "dihedral.OPLS"):
        tr, br = stats[name][0] / med_angle, stats[name][5] / bytes_angle
        if tr > br * spread:
            lines.append("`%s` takes %.2f x the angle kernel's time for %.2f x its algorithmic bytes: the excess, %.2f, is beyond that "
                         "spread, so the kernel is not bound by its algorithmic bytes alone. What the resource report and the code "
                         "suggest (DESIGN 4.17): every table entry gathers three partner rows where an angle entry gathers two and "
                         "a lane holds %.1f entries where it holds %.1f, so a lane issues 12 scattered 32-byte row reads against 6 "
                         "(those rows are cache hits, not HBM traffic, but each is a request to the L2); the batch of 3 entries with "
                         "their 9 partner rows takes 124 VGPRs, 4 waves per SIMD as in the angle kernel (110), and an interior bead's "
                         "fourth entry costs two more dependent round trips in the tail loop, with no more waves than the angle kernel has to "
                         "cover that latency; and a dihedral costs two cross products, one reciprocal square root, one square root and "
                         "two reciprocals in FP64 plus the virial's three outer products, about twice the arithmetic of an angle."
                         % (name, tr, br, tr / br, nd, na))
        else:
            lines.append("`%s` takes %.2f x the angle kernel's time for %.2f x its algorithmic bytes: within that spread of the byte "
                         "ratio." % (name, tr, br))
    report = "\n".join(lines) + "\n"
    print(report)
    if args.out:
        with open(args.out, "w") as f:
            f.write(report)


if __name__ == "__main__":
    main()
