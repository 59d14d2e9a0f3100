"""Event-timed cost of azp_rdf_counts (compute.RadialDistributionFunction), all in one process, after a run-in:

  (a) N = 2^20 on the north-star liquid (FCC at rho* = 0.8), 300 bins, A = B = All, r_max = 3.0 and 6.0, automatic path
      (the cells); the same with two types (A against B, each half of the particles);
  (b) the yardstick: azp_pair_plan_build_from_cells of the same commit on the same system with a list radius equal to
      r_max (r_cut = r_max - buffer) -- it tests the same candidate set; where the plan compiler refuses the radius
      (rows past its capacity) the table says so;
  (c) all-pairs against cells at N = 4,096, 16,384 and 65,536, r_max = 3.0.

Every figure is the mean over --repeats windows of --calls calls, with the smallest and largest window.

  python tools/rdf_probe.py [--ncell 64] [--calls 10] [--repeats 5] [--out profiles/rdf_probe.md] [--json ...] [--only ns|small]
"""

import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncell", type=int, default=64, help="FCC cells per side of (a) and (b) (64: N = 2^20)")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--num-bins", type=int, default=300)
    ap.add_argument("--only", default=None, choices=("ns", "small"), help="(a) + (b) only, or (c) only: for profiler runs")
    ap.add_argument("--out", default=None, help="write the markdown summary here")
    ap.add_argument("--json", default=None, help="write the raw numbers here")
    args = ap.parse_args()

    import torch

    import azplugins_amd as azp
    from azplugins_amd import _lib, compute
    from azplugins_amd import synthetic as syn

    if not torch.cuda.is_available():
        raise SystemExit("rdf_probe: no GPU (the numbers come from a GPU run only)")

    def windows(fn):
        """ms per call: (mean, min, max) over the windows."""
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
        return float(np.mean(out)), float(min(out)), float(max(out))

    def system(cfg, two_types=False):
        n = cfg["xyz"].shape[0]
        typeid = (syn.hash64(9, np.arange(n, dtype=np.uint64), 0) & np.uint64(1)).astype(np.int64) if two_types else None
        sim = azp.Simulation(device="cuda:0", seed=1)
        sim.create_state_from_snapshot(azp.Snapshot.from_arrays(cfg["xyz"], cfg["L"], typeid=typeid, types=("A", "B")))
        return sim

    def rdf_time(sim, r_max, path, filters=None):
        fa, fb = filters or (azp.All(), azp.All())
        rdf = compute.RadialDistributionFunction(fa, fb, r_max, args.num_bins)
        rdf.path = path
        sim.operations.add(rdf)
        row = torch.empty((1, args.num_bins + 4), dtype=torch.int64, device="cuda:0")
        t = windows(lambda: rdf._launch(row.data_ptr()))
        torch.cuda.synchronize()
        host = row.cpu().numpy()[0]
        sim.operations.remove(rdf)
        return t, host

    def plan_time(cfg, r_list):
        """azp_pair_plan_build_from_cells with list radius r_list (the steps of tools/plan_cells_probe.py)."""
        buffer = 0.4
        sim = azp.Simulation(device="cuda:0", seed=1)
        sim.create_state_from_snapshot(azp.Snapshot.from_arrays(cfg["xyz"], cfg["L"]))
        nl = azp.nlist.Cell(buffer=buffer)
        pot = azp.pair.PerturbedLennardJones(nlist=nl, default_r_cut=r_list - buffer)
        pot.params[("A", "A")] = cfg["params"]
        sim.operations.integrator = azp.Integrator(dt=0.005, forces=[pot], methods=[azp.ConstantVolume()])
        sim.operations.tuners.clear()
        sim.run(0)
        nl.compute(sim.state, force=True)
        a = pot._pair_args()
        stream = torch.cuda.current_stream().cuda_stream
        plan = _lib.PairPlan()
        cells = nl.cells_args(160)
        plan.build_from_cells(cells, a, stream)
        torch.cuda.synchronize()
        info = plan.info()
        return windows(lambda: plan.build_from_cells(cells, a, stream)), info

    res = dict(device=torch.cuda.get_device_name(0), calls=args.calls, repeats=args.repeats, num_bins=args.num_bins, rows=[])
    try:
        res["commit"] = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        res["commit"] = "unknown"

    def add(case, n, r_max, what, t, note=""):
        res["rows"].append(dict(case=case, N=int(n), r_max=r_max, what=what, ms=t[0], ms_min=t[1], ms_max=t[2], note=note))
        print(json.dumps(res["rows"][-1]), flush=True)

    if args.only in (None, "ns"):
        cfg = syn.config_north_star(args.ncell)
        n = cfg["xyz"].shape[0]
        sim = system(cfg)
        two = system(cfg, two_types=True)
        for r_max in (3.0, 6.0):
            t, row = rdf_time(sim, r_max, 0)
            add("north star, All-All", n, r_max, "azp_rdf_counts (cells)", t, "%.1f pairs per particle counted" % (row[:-4].sum() / n))
            t2, row2 = rdf_time(sim, r_max, 0)
            assert np.array_equal(row, row2), "two calls differ"
            t, row = rdf_time(two, r_max, 0, (azp.Type(["A"]), azp.Type(["B"])))
            add("north star, A-B (half each)", n, r_max, "azp_rdf_counts (cells)", t, "N_A = %d, N_B = %d" % (row[-4], row[-3]))
            try:
                t, info = plan_time(cfg, r_max)
                add("north star, yardstick", n, r_max, "azp_pair_plan_build_from_cells", t,
                    "plan valid, max_row %d of row_capacity %d" % (info["max_row"], info["row_capacity"]) if info["valid"]
                    else "PLAN INVALID (reason %d, max_row %d of row_capacity %d): the time is of a refused build" % (
                        info["invalid_reason"], info["max_row"], info["row_capacity"]))
            except _lib.AzpError as e:
                add("north star, yardstick", n, r_max, "azp_pair_plan_build_from_cells", (float("nan"),) * 3, "refused: %s" % e)

    if args.only in (None, "small"):
        for shape in ((8, 8, 16), (16, 16, 16), (32, 32, 16)):
            cfg = syn.config_north_star(shape)
            n = cfg["xyz"].shape[0]
            sim = system(cfg)
            rows = {}
            for path, name in ((_lib.RDF_PATH_ALL_PAIRS, "all-pairs"), (_lib.RDF_PATH_CELLS, "cells")):
                t, rows[path] = rdf_time(sim, 3.0, path)
                add("FCC %dx%dx%d" % shape, n, 3.0, "azp_rdf_counts (%s)" % name, t)
            assert np.array_equal(rows[_lib.RDF_PATH_ALL_PAIRS], rows[_lib.RDF_PATH_CELLS]), "the paths differ"

    lines = ["device: %s, commit %s; ms per call, mean [min, max] over %d windows of %d calls, %d bins" % (
        res["device"], res["commit"], args.repeats, args.calls, args.num_bins), "",
        "| case | N | r_max | call | ms per call | note |", "|---|---|---|---|---|---|"]
    for r in res["rows"]:
        lines.append("| %s | %d | %.1f | `%s` | %.3f [%.3f, %.3f] | %s |" % (r["case"], r["N"], r["r_max"], r["what"], r["ms"], r["ms_min"], r["ms_max"], r["note"]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
