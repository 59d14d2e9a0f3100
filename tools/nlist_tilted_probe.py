"""Cost of the cell list in a tilted box (fractional cells) next to the orthorhombic one, all in one process, after a
run-in. The system is the north-star liquid's lattice (FCC at rho* = 0.8, jittered) laid out along the lattice vectors
of three boxes of the same edge lengths, and so the same volume: untilted, tilt (0.5, 0.3, -0.4), tilt (1, 0, 0).

  (a) the row build of nlist.Cell -- binning and the single-pass fill, r_list = 3.4 -- at every --ncell (32: N = 2^17,
      64: N = 2^20), event-timed, ms per build;
  (b) what a list rebuild costs the one consumer of a run: tilted, rows + the tile plan compiled from them
      (azp_pair_plan_build); untilted, binning + the plan compiled from the cells (azp_pair_plan_build_from_cells);
  (c) the NVE step rate of tools/md_bench.py's north-star run (PerturbedLennardJones, r_cut 3.0, buffer 0.4, dt 0.005,
      a particle sort every 200 steps) in the first two boxes, at --md-ncell, both brought to --kT first.

Every figure is the mean over --repeats windows with the smallest and largest window. A commit whose list refuses
tilted boxes reports those rows as refused. --package: directory holding another build of azplugins_amd (a parent commit).

  python tools/nlist_tilted_probe.py [--ncell 32 64] [--md-ncell 64] [--steps 300] [--repeats 3] [--out ...] [--json ...]
"""

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BOXES = (("untilted", (0.0, 0.0, 0.0)), ("tilt (0.5, 0.3, -0.4)", (0.5, 0.3, -0.4)), ("tilt (1, 0, 0)", (1.0, 0.0, 0.0)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncell", type=int, nargs="*", default=[32, 64], help="FCC cells per side of (a) and (b)")
    ap.add_argument("--md-ncell", type=int, default=64, help="FCC cells per side of (c); 0: skip (c)")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--kT", type=float, default=0.7, help="temperature both boxes of (c) are brought to before the NVE windows")
    ap.add_argument("--equilibrate", type=int, default=400, help="thermostatted steps before the NVE windows of (c)")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only-untilted", action="store_true", help="the untilted box alone (the comparison with a parent commit)")
    ap.add_argument("--package", default=ROOT, help="directory that holds the azplugins_amd package to measure")
    ap.add_argument("--label", default=None, help="name of the measured build in the output (default: the commit)")
    ap.add_argument("--out", default=None, help="write the markdown summary here")
    ap.add_argument("--json", default=None, help="write the raw numbers here")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package))

    import torch

    import azplugins_amd as azp
    from azplugins_amd import _lib
    from azplugins_amd import synthetic as syn

    if not torch.cuda.is_available():
        raise SystemExit("nlist_tilted_probe: no GPU (the numbers come from a GPU run only)")

    def windows(fn, calls=args.calls):
        """ms per call: (mean, min, max) over the windows."""
        for _ in range(args.warmup):
            fn()
        out = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) / calls)
        return float(np.mean(out)), float(min(out)), float(max(out))

    def system(ncell, tilt, fused):
        """The liquid's lattice along the lattice vectors of the box, one PerturbedLennardJones consumer."""
        cfg = syn.config_north_star(ncell)
        L = np.asarray(cfg["L"], dtype=np.float64)
        xy, xz, yz = tilt
        h = np.array([[L[0], 0.0, 0.0], [xy * L[1], L[1], 0.0], [xz * L[2], yz * L[2], L[2]]])
        xyz = (cfg["xyz"] / L) @ h
        sim = azp.Simulation(device="cuda:0", seed=1)
        sim.create_state_from_snapshot(azp.Snapshot.from_arrays(xyz, azp.Box(*L, xy=xy, xz=xz, yz=yz)))
        nl = azp.nlist.Cell(buffer=cfg["r_buff"])
        nl.fused = fused
        pot = azp.pair.PerturbedLennardJones(nlist=nl, default_r_cut=cfg["r_cut"])
        pot.params[("A", "A")] = cfg["params"]
        sim.operations.integrator = azp.Integrator(dt=0.005, forces=[pot], methods=[azp.ConstantVolume()])
        sim.operations.tuners.clear()
        return sim, nl, pot

    res = dict(device=torch.cuda.get_device_name(0), calls=args.calls, repeats=args.repeats, rows=[])
    try:
        res["commit"] = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        res["commit"] = "unknown"
    res["label"] = args.label or res["commit"]

    def add(part, box, n, what, t, note=""):
        res["rows"].append(dict(part=part, box=box, N=int(n), what=what, ms=t[0], ms_min=t[1], ms_max=t[2], note=note))
        print(json.dumps(res["rows"][-1]), flush=True)

    nan3 = (float("nan"),) * 3
    stream = torch.cuda.current_stream().cuda_stream
    for ncell in args.ncell:
        for name, tilt in (BOXES[:1] if args.only_untilted else BOXES):
            sim, nl, pot = system(ncell, tilt, fused=False)
            n = sim.state.N
            try:
                sim.run(0)
            except _lib.AzpError as e:
                add("a", name, n, "nlist.Cell row build", nan3, "refused: %s" % e)
                continue
            g = nl._cells.grid
            dims = tuple(int(d) for d in g.dim)
            note = "%d x %d x %d cells, %.1f particles per cell, %s binning, %.1f neighbors per particle" % (
                dims + (n / float(np.prod(dims)), nl.binning_path, nl.n_pairs / n))
            builds = nl.num_builds
            t = windows(lambda: nl.compute(sim.state, force=True))
            assert nl.num_builds == builds + (args.warmup + args.repeats * args.calls) and nl.size == n * nl._row_capacity
            add("a", name, n, "nlist.Cell row build (binning + single-pass fill)", t, note)
            # (b) the consumer's plan from these rows
            a = pot._pair_args()
            plan = _lib.PairPlan()
            plan.build(a, stream)
            info = plan.info()
            add("b", name, n, "azp_pair_plan_build (from the rows)", windows(lambda: plan.build(a, stream)),
                "plan valid" if info["valid"] else "PLAN INVALID (reason %d)" % info["invalid_reason"])
            if not any(tilt):
                cells = nl.cells_args(160)
                plan2 = _lib.PairPlan()
                plan2.build_from_cells(cells, a, stream)
                info = plan2.info()
                if not info["valid"] and info["invalid_reason"] == 3:
                    cells = nl.cells_args((int(info["max_row"] * 1.06) + 11) // 8 * 8)
                    plan2.build_from_cells(cells, a, stream)
                    info = plan2.info()
                add("b", name, n, "azp_pair_plan_build_from_cells", windows(lambda: plan2.build_from_cells(cells, a, stream)),
                    "plan valid" if info["valid"] else "PLAN INVALID (reason %d)" % info["invalid_reason"])
                keep = [None]  # (the tensors the args point to)
                bins = windows(lambda: keep.__setitem__(0, nl._bin(nl._cells, nl._box_at_build, nl._rl_max, n, 1, sim.state.pos.device, stream)))
                add("b", name, n, "binning alone", bins)
            del sim, nl, pot, plan
            torch.cuda.empty_cache()

    if args.md_ncell:
        for name, tilt in (BOXES[:1] if args.only_untilted else BOXES[:2]):
            sim, nl, pot = system(args.md_ncell, tilt, fused=True)
            n = sim.state.N
            sim.operations.tuners.append(azp.ParticleSorter(trigger_period=200, curve="hilbert"))
            try:
                sim.run(0)
            except _lib.AzpError as e:
                add("c", name, n, "NVE step", nan3, "refused: %s" % e)
                continue
            # the lattice laid out along tilted vectors is strained and heats up as it melts: bring both boxes to the same
            # temperature with a Berendsen thermostat before the NVE windows
            sim.thermalize_particle_momenta(args.kT, seed=7)
            method = sim.operations.integrator.methods[0]
            method.thermostat = azp.thermostats.Berendsen(kT=args.kT, tau=0.05)
            sim.run(50)
            sim.operations.tuners[0].sort(sim)
            sim.run(args.equilibrate)
            method.thermostat = None
            _ = nl.size
            sim.run(20)
            out, b0 = [], nl.num_builds
            for _ in range(args.repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                sim.run(args.steps)
                torch.cuda.synchronize()
                out.append(1e3 * (time.perf_counter() - t0) / args.steps)
            builds = nl.num_builds - b0
            add("c", name, n, "NVE step (%d steps per window)" % args.steps, (float(np.mean(out)), min(out), max(out)),
                "%d list rebuilds = one per %.1f steps; plan %s; kT = %.3f" % (
                    builds, args.repeats * args.steps / max(builds, 1),
                    "from the cells" if pot.plan_info["from_cells"] else "from the rows", sim.kinetic_temperature()))
            del sim, nl, pot
            torch.cuda.empty_cache()

    lines = ["build: %s; device: %s; ms, mean [min, max] over %d windows (of %d calls in (a) and (b))" % (
        res["label"], res["device"], args.repeats, args.calls), "",
        "| part | box | N | what | ms | note |", "|---|---|---|---|---|---|"]
    for r in res["rows"]:
        lines.append("| %s | %s | %d | %s | %.3f [%.3f, %.3f] | %s |" % (r["part"], r["box"], r["N"], r["what"], r["ms"], r["ms_min"], r["ms_max"], r["note"]))
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
