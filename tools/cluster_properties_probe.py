"""Event-timed cost of azp_cluster_properties (compute.ClusterProperties) on its own against the azp_cluster_compute call
on the same state, on the north-star liquid (FCC at rho* = 0.8, N = 2^20 for --ncell 64) in three regimes of the cluster
sizes, all in one process:

  liquid      a cut-off found by bisection on the device's own edge count for a mean coordination of --coordination
              (below percolation: many small clusters)
  one         a cut-off with a mean coordination near 12: one cluster of everything
  singletons  a cut-off below every distance: N clusters of one

  the Cluster call       Cluster(All(), r_max) with the representative rows asked for
  the properties call    azp_cluster_properties alone, on the labels that call left

Every figure is the median over --repeats windows of --calls calls, with the smallest and largest window. Two properties
calls on one state are compared bit for bit. The threshold below which lanes send their own atomics (AZP_CP_DIRECT in
csrc/cluster_properties.hip) is a compile-time constant: a candidate is a library of its own
(make -C azplugins_amd/csrc variant SRC=cluster_properties NAME=cpd4 DEFS=-DAZP_CP_DIRECT=4) run with
AZP_LIB_PATH=tools/libazp_cpd4.so and the --r-max that the first run printed.

Per-kernel times come from a kernel trace of one regime, which then times the properties call only:
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/cluster_properties_probe.py --only one --r-max a b c

  python tools/cluster_properties_probe.py [--ncell 64] [--calls 5] [--repeats 5] [--r-max a b c] [--label text]
                                           [--out profiles/cluster_properties_probe.md] [--only liquid|one|singletons]
"""

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REGIMES = ("liquid", "one", "singletons")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncell", type=int, default=64, help="FCC cells per side (64: N = 2^20)")
    ap.add_argument("--coordination", type=float, default=1.0, help="the mean coordination of the liquid regime")
    ap.add_argument("--r-max", type=float, nargs=3, default=None, help="the three cut-offs (skips the bisection)")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default=None, choices=REGIMES, help="one regime, the properties call only: for profiler runs")
    ap.add_argument("--label", default="", help="goes into every row (the library under test)")
    ap.add_argument("--out", default=None, help="write the markdown summary here")
    args = ap.parse_args()

    import torch

    import azplugins_amd as azp
    from azplugins_amd import compute
    from azplugins_amd import synthetic as syn

    if not torch.cuda.is_available():
        raise SystemExit("cluster_properties_probe: no GPU (the numbers come from a GPU run only)")

    def windows(fn):
        """ms per call: (median, min, max) over the windows."""
        for _ in range(args.warmup):
            fn()
        out = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) / args.calls)
        return float(np.median(out)), float(min(out)), float(max(out))

    cfg = syn.config_north_star(args.ncell)
    n = cfg["xyz"].shape[0]
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(azp.Snapshot.from_arrays(cfg["xyz"], cfg["L"]))
    rows = []

    def coordination(r_max):
        c = compute.Cluster(azp.All(), r_max)
        sim.operations.add(c)
        z = 2.0 * c.num_edges / n
        sim.operations.remove(c)
        return z

    def find_r_max(target):
        """Bisection on the device's own edge count, to two decimals (the coordination grows with r_max)."""
        lo, hi = 0.8, 1.6
        for _ in range(12):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if coordination(mid) < target else (lo, mid)
        return round(0.5 * (lo + hi), 2)

    r_maxes = args.r_max or (find_r_max(args.coordination), find_r_max(12.0), 0.8)
    print("r_max: %s" % " ".join("%.2f" % r for r in r_maxes), flush=True)
    ratios = {}
    for label, r_max in zip(REGIMES, r_maxes):
        if args.only not in (None, label):
            continue
        c = compute.Cluster(azp.All(), r_max)
        p = compute.ClusterProperties(c)
        sim.operations.add(c)
        sim.operations.add(p)
        row = torch.empty((1, 20), dtype=torch.float64, device="cuda:0")
        crow = torch.empty((1, c._row_width()), dtype=torch.int64, device="cuda:0")
        p._launch(row.data_ptr())  # the labels of this state, with the representative rows
        p._own_only = True
        t_props = windows(lambda: p._launch(row.data_ptr()))
        first, table = row.cpu().numpy()[0].copy(), p._table.clone()
        p._launch(row.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(first, row.cpu().numpy()[0]) and torch.equal(table[: int(first[0])], p._table[: int(first[0])]), "two calls differ"
        note = "%s%d clusters, the largest of %d (compact: %d), Rg %.3f" % (
            args.label + ": " if args.label else "", first[0], first[5], first[16], np.sqrt(max(first[15], 0.0)))
        c._want_rep = True  # (the Cluster call as ClusterProperties queues it: with the representative rows)
        t_cluster = None if args.only else windows(lambda: c._launch(crow.data_ptr()))
        c._want_rep = False
        for what, t in (("azp_cluster_properties", t_props), ("azp_cluster_compute", t_cluster)):
            if t is not None:
                rows.append(dict(what=what, regime=label, N=int(n), r_max=r_max, ms=t[0], ms_min=t[1], ms_max=t[2],
                                 note=note if what == "azp_cluster_properties" else ""))
                print(json.dumps(rows[-1]), flush=True)
        if t_cluster is not None:
            ratios[label] = (t_props[0], t_props[0] / t_cluster[0])
        sim.operations.remove(p)
        sim.operations.remove(c)

    lines = ["device: %s; N = %d; ms per call, median [min, max] over %d windows of %d calls" % (
        torch.cuda.get_device_name(0), n, args.repeats, args.calls), "", "| call | regime | r_max | ms per call | note |", "|---|---|---|---|---|"]
    for r in rows:
        lines.append("| `%s` | %s | %.2f | %.3f [%.3f, %.3f] | %s |" % (r["what"], r["regime"], r["r_max"], r["ms"], r["ms_min"], r["ms_max"], r["note"]))
    if ratios:
        lines += [""] + ["%s: properties / Cluster = %.2f" % (label, ratio) for label, (_, ratio) in ratios.items()]
        ms = [t for t, _ in ratios.values()]
        lines += ["the properties call, worst regime / best regime = %.2f" % (max(ms) / min(ms))]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
