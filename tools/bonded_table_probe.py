"""The tabulated angle and dihedral kernels and the bonded-histogram kernel on the C3 chains (N = 1,048,576: 32,768
chains of 32 beads with angles and dihedrals along the chains), against the analytic kernels of the same kind on the
same state: time per launch and its ratio. Every call sits between its own pair of device events and the cases are
interleaved. No time is fixed in advance: the figures to judge are the ratios.

    python tools/bonded_table_probe.py --reps 200 --warmup 20 --out profiles/bonded_table.md
    python tools/bonded_table_probe.py --resources        # no GPU: VGPRs, scratch and waves per instance

``--resources`` compiles the three translation units for gfx950 with the compiler's own resource report
(``-Rpass-analysis=kernel-resource-usage``) and prints one row per kernel instance. ``AZP_LIB_PATH`` selects another
build of the library, e.g. ``make -C azplugins_amd/csrc variant NAME=db2 SRC=dihedral_forces
DEFS=-DAZP_DIHEDRAL_BATCH=2`` for the batch question; ``--label`` names it in the report.

The lattice chains of C3 are nearly straight: the bending angles lie within 0.3 of pi, so an angle table is read in
its last tenth only, while the dihedral angles of nearly collinear chains are spread over all of [-pi, pi]. ``--crumple``
displaces every bead by up to 0.35 lattice constants, which spreads the bending angles over about a third of the
table; both are reported."""
import argparse
import math
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

WIDTHS = (64, 1024, 16384)


def resources():
    """One row per kernel instance of the three translation units: VGPRs, scratch bytes per lane, waves per SIMD."""
    csrc = os.path.join(ROOT, "azplugins_amd", "csrc")
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for unit in ("angle_forces", "dihedral_forces", "bonded_histogram"):
            out = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-fast-math",
                                  "-ffp-contract=on", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                                  os.path.join(csrc, unit + ".hip"), "-o", os.path.join(tmp, unit + ".o")] + sys.argv[2:],
                                 stderr=subprocess.PIPE, stdout=subprocess.PIPE, universal_newlines=True, check=True).stderr
            name = None
            for line in out.splitlines():
                m = re.search(r"remark:\s+(Function Name|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\S+)", line)
                if not m:
                    continue
                if m.group(1) == "Function Name":
                    name = subprocess.run(["c++filt", m.group(2)], stdout=subprocess.PIPE, universal_newlines=True).stdout.strip()
                    name = re.sub(r"^void azp::|\(.*$", "", name).replace("azp::", "")
                    rows.append([name])
                else:
                    rows[-1].append(m.group(2))
    print("| instance | VGPRs | scratch B/lane | waves/SIMD |\n|---|---|---|---|")
    for r in rows:
        print("| `%s` | %s | %s | %s |" % tuple(r))


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


def sample(lo, hi, width, U, tau):
    x = np.linspace(lo, hi, width)
    return dict(U=U(x), tau=tau(x))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--resources":
        return resources()
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="1/64 of C3 (a rehearsal size, not a measurement)")
    ap.add_argument("--crumple", action="store_true", help="displace every bead by up to 0.35 a: bending angles over a third of the table")
    ap.add_argument("--label", default="", help="names the build of the library in the report")
    ap.add_argument("--out", default=None, help="write the report to this file as well")
    args = ap.parse_args()
    import torch

    import azplugins_amd as azp
    from azplugins_amd import compute
    from azplugins_amd import synthetic as syn

    if not torch.cuda.is_available():
        raise SystemExit("bonded_table_probe: no GPU; nothing is measured without one")
    cfg = syn.config_chains(32, 32, 16, 32) if args.small else syn.config_chains()
    xyz = cfg["xyz"]
    if args.crumple:
        a = 0.8 ** (-1.0 / 3.0)
        tag = np.arange(xyz.shape[0], dtype=np.uint64)
        xyz = syn.wrap(xyz + np.stack([(2.0 * syn.u01(97, tag, c) - 1.0) * 0.35 * a for c in range(3)], axis=1), cfg["L"])
    angles, dihedrals = chain_topology(cfg["bonds"])
    N = xyz.shape[0]
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(azp.Snapshot.from_arrays(xyz, cfg["L"], bonds=cfg["bonds"], angles=angles, dihedrals=dihedrals))
    sim.operations.tuners.clear()
    dw = azp.bond.DoubleWell()
    dw.params["A-A"] = cfg["bond_params"]
    dw.defer_flag_check = True  # (as inside Simulation.run: no host round trip for the flag word behind every launch)
    k, t0 = 10.0, 2.6
    ha = azp.angle.Harmonic()
    ha.params["A-A-A"] = dict(k=k, t0=t0)
    k1, k2, k3, k4 = 1.5, -0.5, 0.8, 0.2
    op = azp.dihedral.OPLS()
    op.params["A-A-A-A"] = dict(k1=k1, k2=k2, k3=k3, k4=k4)
    forces = [("bond.DoubleWell", dw, "bond"), ("angle.Harmonic", ha, "angle"), ("dihedral.OPLS", op, "dihedral")]
    for w in WIDTHS:
        at = azp.angle.Table()
        at.params["A-A-A"] = sample(0.0, math.pi, w, lambda t: 0.5 * k * (t - t0) ** 2, lambda t: -k * (t - t0))
        dt = azp.dihedral.Table()
        dt.params["A-A-A-A"] = sample(-math.pi, math.pi, w,
                                      lambda p: 0.5 * (k1 * (1 + np.cos(p)) + k2 * (1 - np.cos(2 * p)) + k3 * (1 + np.cos(3 * p)) + k4 * (1 - np.cos(4 * p))),
                                      lambda p: 0.5 * (k1 * np.sin(p) - 2 * k2 * np.sin(2 * p) + 3 * k3 * np.sin(3 * p) - 4 * k4 * np.sin(4 * p)))
        forces += [("angle.Table, width %d" % w, at, "angle"), ("dihedral.Table, width %d" % w, dt, "dihedral")]
    sim.operations.integrator = azp.Integrator(dt=0.001, forces=[f for _, f, _ in forces])
    sim.run(0)
    # the tables against the analytic kernels, once (harmonic tau is linear: exact; OPLS: within the interpolation error)
    check = ["angle.Table, width %d against angle.Harmonic: largest force deviation %.2e of %.2e"
             % (WIDTHS[-1], np.abs(forces[-2][1].forces - ha.forces).max(), np.abs(ha.forces).max()),
             "dihedral.Table, width %d against dihedral.OPLS: largest force deviation %.2e of %.2e"
             % (WIDTHS[-1], np.abs(forces[-1][1].forces - op.forces).max(), np.abs(op.forces).max())]
    hists = []
    for kind, kw in (("bond", dict(r_min=0.5, r_max=2.0)), ("angle", {}), ("dihedral", {})):
        for path, label in ((0, "LDS"), (2, "global atomics")):
            d = compute.BondedDistribution(kind, 256, **kw)
            d.path = path
            sim.operations.add(d)
            row = torch.empty((1, d._row_width()), dtype=torch.int64, device="cuda:0")
            hists.append(("histogram %s, 256 bins, %s" % (kind, label), d, row, kind))
    cases = [(name, f.compute, kind, (0,)) for name, f, kind in forces]
    cases += [(name, d._launch, kind, (row.data_ptr(),)) for name, d, row, kind in hists]
    times = {c[0]: [] for c in cases}
    for it in range(args.warmup + args.reps):
        for name, fn, _, fargs in cases:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(*fargs)
            e1.record()
            if it >= args.warmup:
                times[name].append((e0, e1))
    torch.cuda.synchronize()
    counts = {kind: int(row[0, 256 + 1].item()) for _, _, row, kind in hists}
    theta = compute.BondedDistribution("angle", 64)
    sim.operations.add(theta)
    used = int((theta.counts[0] > 0).sum())
    base = {"bond": "bond.DoubleWell", "angle": "angle.Harmonic", "dihedral": "dihedral.OPLS"}
    stats = {}
    for name, _, _, _ in cases:
        t = np.array([a.elapsed_time(b) * 1e3 for a, b in times[name]])
        stats[name] = (float(np.median(t)), t.min(), np.percentile(t, 10), np.percentile(t, 90), t.max())
    lines = ["## %s%s" % ("crumpled chains" if args.crumple else "lattice chains", (", " + args.label) if args.label else ""), "",
             "device: %s, N = %d, %d bonds, %d angles, %d dihedrals (counted by the histogram kernel: %d, %d, %d); the bending "
             "angles occupy %d of 64 equal bins of [0, pi]; %d timed calls per case after %d warm-up calls, every call between "
             "its own pair of device events, the cases interleaved."
             % (torch.cuda.get_device_name(0), N, len(cfg["bonds"]), len(angles), len(dihedrals), counts["bond"], counts["angle"],
                counts["dihedral"], used, args.reps, args.warmup), ""] + check + ["",
             "| kernel | median us | min | p10 | p90 | max | x analytic kernel of the kind |", "|---|---|---|---|---|---|---|"]
    for name, _, kind, _ in cases:
        med, tmin, p10, p90, tmax = stats[name]
        lines.append("| %s | %.1f | %.1f | %.1f | %.1f | %.1f | %.2f |" % (name, med, tmin, p10, p90, tmax, med / stats[base[kind]][0]))
    report = "\n".join(lines) + "\n"
    print(report)
    if args.out:
        with open(args.out, "a") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
