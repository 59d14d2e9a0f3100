"""Event-timed cost of the topology exclusions on the C3 chains (32,768 chains of 32 beads, N = 2^20), all
in one process, after a run-in:

  (a) azp_pair_plan_build_from_cells, the rebuild of the fused neighbor list, with exclusions=("bond",) (two entries per
      interior bead, all in the compiler's four registers) against ("bond", "1-3", "1-4") (six: two of them walked from
      global memory); and, once each, the torch build of the merged exclusion table that the second needs;
  (b) azp_special_pair_forces_lj over the chains' 1-4 pairs against azp_bond_forces_double_well over their bonds (both
      with the virial);
  (c) azp_rdf_counts alone against azp_rdf_counts + azp_rdf_subtract_excluded with ("bond", "1-3", "1-4"), 300 bins,
      r_max = 3.5 (the chains' 1-4 pairs are 3.2 apart), automatic path.

Every figure is the mean over --repeats windows of --calls calls, with the smallest and largest window.

  python tools/exclusion_probe.py [--shape 128 128 64 32] [--calls 10] [--repeats 5] [--out profiles/exclusions.md] [--json ...]
"""

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALL = ("bond", "1-3", "1-4")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=4, default=(128, 128, 64, 32), metavar=("NX", "NY", "NZ", "LEN"),
                    help="lattice and chain length of synthetic.config_chains (default: C3, N = 2^20)")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--num-bins", type=int, default=300)
    ap.add_argument("--out", default=None, help="write the markdown summary here")
    ap.add_argument("--json", default=None, help="write the raw numbers here")
    args = ap.parse_args()

    import torch

    import azplugins_amd as azp
    from azplugins_amd import _lib, compute
    from azplugins_amd import synthetic as syn
    from azplugins_amd.state import excluded_pairs

    if not torch.cuda.is_available():
        raise SystemExit("exclusion_probe: no GPU (the numbers come from a GPU run only)")

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

    cfg = syn.config_chains(*args.shape)
    n = cfg["xyz"].shape[0]
    bonds = np.asarray(cfg["bonds"], dtype=np.int64)
    p14 = excluded_pairs(("1-4",), {"bond": torch.from_numpy(bonds)}).numpy()
    p14 = p14[p14[:, 0] < p14[:, 1]]

    res = dict(device=torch.cuda.get_device_name(0), calls=args.calls, repeats=args.repeats, num_bins=args.num_bins, N=int(n),
               bonds=int(len(bonds)), pairs_1_4=int(len(p14)), rows=[])
    try:
        res["commit"] = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        res["commit"] = "unknown"

    def add(what, t, note=""):
        res["rows"].append(dict(what=what, ms=t[0], ms_min=t[1], ms_max=t[2], note=note))
        print(json.dumps(res["rows"][-1]), flush=True)

    def simulation(**topology):
        sim = azp.Simulation(device="cuda:0", seed=1)
        sim.create_state_from_snapshot(azp.Snapshot.from_arrays(cfg["xyz"], cfg["L"], bonds=bonds, **topology))
        sim.operations.tuners.clear()
        return sim

    # (a) the fused rebuild (the steps of tools/plan_cells_probe.py)
    for kinds in (("bond",), ALL):
        sim = simulation()
        nl = azp.nlist.Cell(buffer=cfg["r_buff"], exclusions=kinds)
        pot = azp.pair.PerturbedLennardJones(nlist=nl, default_r_cut=cfg["r_cut"], mode="shift")
        pot.params[("A", "A")] = cfg["params"]
        sim.operations.integrator = azp.Integrator(dt=0.005, forces=[pot], methods=[azp.ConstantVolume()])
        if kinds != ("bond",):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            table = sim.state.exclusion_table(kinds)
            torch.cuda.synchronize()
            first = 1e3 * (time.perf_counter() - t0)
            sim.state.drop_exclusion_table()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            table = sim.state.exclusion_table(kinds)
            torch.cuda.synchronize()
            again = 1e3 * (time.perf_counter() - t0)
            add("State.exclusion_table%r, torch, wall clock" % (kinds,), (again, again, first),
                "width %d; min: a second build, max: the first (lazy kernel loading); kept until the topology or the order changes"
                % table[1].shape[0])
        sim.run(0)
        nl.compute(sim.state, force=True)
        a = pot._pair_args()
        stream = torch.cuda.current_stream().cuda_stream
        plan = _lib.PairPlan()
        cells = nl.cells_args(160)
        plan.build_from_cells(cells, a, stream)
        torch.cuda.synchronize()
        info = plan.info()
        t = windows(lambda: plan.build_from_cells(cells, a, stream))
        add("azp_pair_plan_build_from_cells, exclusions=%r" % (kinds,), t,
            ("plan valid, max_row %d" % info["max_row"]) if info["valid"] else "PLAN INVALID (reason %d)" % info["invalid_reason"])

    # (b) the special-pair kernel against the bond kernel
    sim = simulation(pairs=p14)
    dw = azp.bond.DoubleWell()
    dw.params["A-A"] = cfg["bond_params"]
    lj = azp.special_pair.LJ()
    lj.params["A-A"] = dict(epsilon=0.5, sigma=1.0)
    lj.r_cut["A-A"] = 4.0  # (the 1-4 pairs of the lattice chains are 3.2 apart: inside, the arithmetic runs)
    dw.compute_virial = lj.compute_virial = True
    sim.operations.integrator = azp.Integrator(dt=0.005, forces=[dw, lj], methods=[azp.ConstantVolume()])
    sim.run(0)
    dw.defer_flag_check = True
    add("azp_bond_forces_double_well, %d bonds" % len(bonds), windows(dw.compute), "with its flag word's copy on a side stream")
    dw.check_flags(wait=True)
    add("azp_special_pair_forces_lj, %d 1-4 pairs" % len(p14), windows(lj.compute))

    # (c) the RDF with and without the subtraction
    rows = {}
    for kinds in ((), ALL):
        rdf = compute.RadialDistributionFunction(azp.All(), azp.All(), 3.5, args.num_bins, exclusions=kinds)
        sim.operations.add(rdf)
        row = torch.empty((1, args.num_bins + 4), dtype=torch.int64, device="cuda:0")
        rdf._launch(row.data_ptr())  # (builds and keeps the exclusion table)
        t = windows(lambda: rdf._launch(row.data_ptr()))
        torch.cuda.synchronize()
        rows[kinds] = row.cpu().numpy()[0]
        add("azp_rdf_counts%s, r_max = 3.5" % (" + azp_rdf_subtract_excluded%r" % (kinds,) if kinds else ""), t,
            "%.2f pairs per particle counted, %d ordered pairs taken out" % (rows[kinds][:-4].sum() / n, rows[kinds][-1]))
        sim.operations.remove(rdf)
    assert rows[()][:-4].sum() - rows[ALL][:-4].sum() == rows[ALL][-1] and rows[()][-1] == 0

    lines = ["device: %s, commit %s; N = %d (%d bonds, %d 1-4 pairs); ms per call, mean [min, max] over %d windows of %d calls" % (
        res["device"], res["commit"], n, len(bonds), len(p14), args.repeats, args.calls), "",
        "| call | ms per call | note |", "|---|---|---|"]
    for r in res["rows"]:
        lines.append("| `%s` | %.3f [%.3f, %.3f] | %s |" % (r["what"], r["ms"], r["ms_min"], r["ms_max"], r["note"]))
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
