"""Event-timed cost of azp_steinhardt_compute (compute.Steinhardt, compute.SolidLiquid) on the north-star liquid (FCC at
rho* = 0.8, N = 2^20 for --ncell 64), r_max = 1.5, l = (4, 6), all in one process after a run-in:

  the first pass alone            Steinhardt(All(), (4, 6), r_max)
  with the neighbour average      Steinhardt(All(), (4, 6), r_max, average=True)
  with the solid-bond count       SolidLiquid(All(), 6, r_max, 0.7, 6)                 (one l)
  the yardstick                   RadialDistributionFunction(All(), All(), r_max, 100): the same candidates, one square
                                  root and one integer atomic per accepted pair

Every figure is the median over --repeats windows of --calls calls, with the smallest and largest window. Two calls on
one state are compared bit for bit, and the cells path against the all-pairs path at a small size.

  python tools/steinhardt_probe.py [--ncell 64] [--calls 5] [--repeats 5] [--out profiles/steinhardt_probe.md] [--only first|average|solid|rdf]
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
    ap.add_argument("--r-max", type=float, default=1.5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default=None, choices=("first", "average", "solid", "rdf"), help="one case only: for profiler runs")
    ap.add_argument("--out", default=None, help="write the markdown summary here")
    args = ap.parse_args()

    import torch

    import azplugins_amd as azp
    from azplugins_amd import _lib, compute
    from azplugins_amd import synthetic as syn

    if not torch.cuda.is_available():
        raise SystemExit("steinhardt_probe: no GPU (the numbers come from a GPU run only)")

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

    def add(what, t, note=""):
        rows.append(dict(what=what, N=int(n), ms=t[0], ms_min=t[1], ms_max=t[2], note=note))
        print(json.dumps(rows[-1]), flush=True)

    def bond_order(what, c):
        sim.operations.add(c)
        row = torch.empty((1, c._row_width()), dtype=torch.int64, device="cuda:0")
        t = windows(lambda: c._launch(row.data_ptr()))
        first = row.cpu().numpy()[0].copy()
        words = c._out[2]["words"].clone()
        c._launch(row.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(first, row.cpu().numpy()[0]) and torch.equal(words, c._out[2]["words"]), "two calls differ"
        s = compute.steinhardt_summary(first, len(c.l), c._num_bins)
        note = "%.2f neighbours per particle" % (s["sum_neighbors"] / max(s["num_particles"], 1))
        if isinstance(c, compute.Steinhardt):
            note += ", <q_l> = %s" % ", ".join("%.4f" % x for x in s["order"])
        else:
            note += ", %d solid" % s["num_solid"]
        add(what, t, note)
        sim.operations.remove(c)
        return t

    times = {}
    if args.only in (None, "rdf"):
        rdf = compute.RadialDistributionFunction(azp.All(), azp.All(), args.r_max, 100)
        sim.operations.add(rdf)
        row = torch.empty((1, 104), dtype=torch.int64, device="cuda:0")
        times["rdf"] = windows(lambda: rdf._launch(row.data_ptr()))
        add("azp_rdf_counts (cells), 100 bins", times["rdf"], "%.2f pairs per particle counted" % (row.cpu().numpy()[0, :100].sum() / n))
        sim.operations.remove(rdf)
    if args.only in (None, "first"):
        times["first"] = bond_order("azp_steinhardt_compute, l = (4, 6)", compute.Steinhardt(azp.All(), (4, 6), args.r_max))
    if args.only in (None, "average"):
        times["average"] = bond_order("azp_steinhardt_compute, l = (4, 6), AVERAGE", compute.Steinhardt(azp.All(), (4, 6), args.r_max, average=True))
    if args.only in (None, "solid"):
        times["solid"] = bond_order("azp_steinhardt_compute, l = 6, CONNECTIONS", compute.SolidLiquid(azp.All(), 6, args.r_max, 0.7, 6))

    if args.only is None:
        # the two paths at a size the all-pairs kernels can take
        small = syn.config_north_star(8)
        sim2 = azp.Simulation(device="cuda:0", seed=1)
        sim2.create_state_from_snapshot(azp.Snapshot.from_arrays(small["xyz"], small["L"]))
        got = []
        for path in (_lib.STEINHARDT_PATH_ALL_PAIRS, _lib.STEINHARDT_PATH_CELLS):
            c = compute.Steinhardt(azp.All(), (4, 6), args.r_max, average=True)
            c.path = path
            sim2.operations.add(c)
            got.append((c._read("qlm"), c._read("qlm_average")))
        assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]), "the paths differ"

    lines = ["device: %s; N = %d, r_max = %.2f; ms per call, median [min, max] over %d windows of %d calls" % (
        torch.cuda.get_device_name(0), n, args.r_max, args.repeats, args.calls), "", "| call | ms per call | note |", "|---|---|---|"]
    for r in rows:
        lines.append("| `%s` | %.3f [%.3f, %.3f] | %s |" % (r["what"], r["ms"], r["ms_min"], r["ms_max"], r["note"]))
    if "rdf" in times and "first" in times:
        lines += ["", "first pass / RDF = %.2f" % (times["first"][0] / times["rdf"][0])]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
