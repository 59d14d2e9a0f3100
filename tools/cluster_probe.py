"""Event-timed cost of azp_cluster_compute (compute.Cluster) on the north-star liquid (FCC at rho* = 0.8, N = 2^20 for
--ncell 64), at two cut-offs found by bisection on the device's own edge count: a mean coordination near 2 (many small
clusters, the percolation regime) and near 12 (one cluster of everything), all in one process:

  the whole call                  Cluster(All(), r_max)
  order only / order + union      the same call stopped early (azp_cluster_args.stages = 1 / 2); their difference is the
                                  union pass alone
  the yardstick                   RadialDistributionFunction(All(), All(), r_max, 100) on the same state: the same
                                  candidates, one square root and one integer atomic per accepted pair

Every figure is the median over --repeats windows of --calls calls, with the smallest and largest window. Two calls on
one state are compared bit for bit, and the cells path against the all-pairs path at a small size.

  python tools/cluster_probe.py [--ncell 64] [--calls 5] [--repeats 5] [--out profiles/cluster_probe.md] [--only low|high]
"""

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncell", type=int, default=64, help="FCC cells per side (64: N = 2^20)")
    ap.add_argument("--coordination", type=float, nargs=2, default=(2.0, 12.0), help="the two mean coordinations aimed at")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default=None, choices=("low", "high"), help="one cut-off, the whole call only: for profiler runs")
    ap.add_argument("--out", default=None, help="write the markdown summary here")
    args = ap.parse_args()

    import torch

    import azplugins_amd as azp
    from azplugins_amd import _lib, compute
    from azplugins_amd import synthetic as syn

    if not torch.cuda.is_available():
        raise SystemExit("cluster_probe: no GPU (the numbers come from a GPU run only)")

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

    def add(what, r_max, t, note=""):
        rows.append(dict(what=what, N=int(n), r_max=r_max, ms=t[0], ms_min=t[1], ms_max=t[2], note=note))
        print(json.dumps(rows[-1]), flush=True)

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

    ratios = {}
    for label, target in zip(("low", "high"), args.coordination):
        if args.only not in (None, label):
            continue
        r_max = find_r_max(target)
        c = compute.Cluster(azp.All(), r_max)
        sim.operations.add(c)
        row = torch.empty((1, c._row_width()), dtype=torch.int64, device="cuda:0")
        times = {}
        for stages in (0,) if args.only else (0, 1, 2):
            c._stages = stages
            times[stages] = windows(lambda: c._launch(row.data_ptr()))
        c._stages = 0
        c._launch(row.data_ptr())
        first, keys = row.cpu().numpy()[0].copy(), c._out[2].clone()
        c._launch(row.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(first, row.cpu().numpy()[0]) and torch.equal(keys, c._out[2]), "two calls differ"
        s = compute.cluster_summary(first, c.size_bins)
        note = "coordination %.2f, %d clusters, the largest of %d, weight average %.1f" % (
            2.0 * s["num_edges"] / n, s["num_clusters"], s["largest_cluster_size"], s["sum_size_squared"] / max(s["num_particles"], 1))
        add("azp_cluster_compute", r_max, times[0], note)
        sim.operations.remove(c)
        if args.only:
            continue
        add("  order only (stages = 1)", r_max, times[1])
        add("  order + union (stages = 2)", r_max, times[2])
        union = times[2][0] - times[1][0]
        rdf = compute.RadialDistributionFunction(azp.All(), azp.All(), r_max, 100)
        sim.operations.add(rdf)
        rrow = torch.empty((1, 104), dtype=torch.int64, device="cuda:0")
        t_rdf = windows(lambda: rdf._launch(rrow.data_ptr()))
        add("azp_rdf_counts (cells), 100 bins", r_max, t_rdf, "%.2f pairs per particle counted" % (rrow.cpu().numpy()[0, :100].sum() / n))
        sim.operations.remove(rdf)
        ratios[label] = (r_max, times[0][0] / t_rdf[0], union, union / times[0][0])

    if args.only is None:
        # the two paths at a size the all-pairs kernel can take
        small = syn.config_north_star(8)
        sim2 = azp.Simulation(device="cuda:0", seed=1)
        sim2.create_state_from_snapshot(azp.Snapshot.from_arrays(small["xyz"], small["L"]))
        got = []
        for path in (_lib.CLUSTER_PATH_ALL_PAIRS, _lib.CLUSTER_PATH_CELLS):
            c = compute.Cluster(azp.All(), 1.15)
            c.path = path
            sim2.operations.add(c)
            got.append((c.cluster_keys, c.cluster_sizes, c._read("summary")))
        assert all(np.array_equal(a, b) for a, b in zip(*got)), "the paths differ"

    lines = ["device: %s; N = %d; ms per call, median [min, max] over %d windows of %d calls" % (
        torch.cuda.get_device_name(0), n, args.repeats, args.calls), "", "| call | r_max | ms per call | note |", "|---|---|---|---|"]
    for r in rows:
        lines.append("| `%s` | %.2f | %.3f [%.3f, %.3f] | %s |" % (r["what"].strip(), r["r_max"], r["ms"], r["ms_min"], r["ms_max"], r["note"]))
    for label, (r_max, ratio, union, share) in ratios.items():
        lines += ["", "r_max = %.2f: Cluster / RDF = %.2f; the union pass alone %.3f ms, %.0f %% of the call" % (r_max, ratio, union, 100.0 * share)]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
