"""What the host side of the integration methods computes and costs, for one checkout or for two side by side (the
method of profiles/step_loop.md, sections 2 and 3). Every side runs in a fresh child process that imports the package from
its checkout (which must hold a built libazp.so) and the scenarios from this checkout's tests/.

  digests: on the GPU. SHA-256 of pos, vel and image ordered by tag after run(12), for the four paths of
           tests/test_gpu_step_loop.py and for an NPT run of the liquid of tests/test_gpu_barostat.py (ConstantPressure with
           Bussi, couple="xyz"), whose box lengths and barostat_dof are digested too.
  host:    no GPU. Host time per step with the launches intercepted by the harness of tests/test_step_loop.py (the figures
           contain the harness's recording): 100 steps of run-in, then run(10000) six times per process, the smallest kept;
           thread CPU time; --processes children per checkout, the checkouts alternating. The stand-in's barostat scales the
           box by 1 +- 1e-7 every step, so that it changes every step and survives 60 000 of them.

  python tools/methods_probe.py digests --checkout . [--checkout ../parent] [--json out.json]
  python tools/methods_probe.py host --checkout ../parent --checkout . [--processes 5] [--steps 10000] [--json out.json]
"""

import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_PATHS = ["nve", "nve_rot", "nve_domain", "bussi", "fire", "langevin", "langevin_brownian", "nph", "npt_bussi"]


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def child_digests():
    import torch

    import azplugins_amd as azp
    import test_gpu_barostat as tb
    import test_gpu_step_loop as ts
    from azplugins_amd import thermostats

    out = {}
    for path in ts.PATHS:
        sim, _ = ts._sim(path)
        sim.run(12)
        end = ts._by_tag(sim)
        out[path] = _sha(end["pos"], end["vel"], end["image"])
    method = azp.ConstantPressure(azp.All(), S=2.0, tauS=tb.LIQ_TAUS_NPT, couple="xyz", thermostat=thermostats.Bussi(kT=1.0, tau=0.5))
    sim = tb._liquid(method)[0]
    sim.run(12)
    end = ts._by_tag(sim)
    box = sim.state.box
    out["npt"] = _sha(end["pos"], end["vel"], end["image"])
    out["npt box, barostat_dof"] = _sha(torch.tensor([box.Lx, box.Ly, box.Lz], dtype=torch.float64),
                                         torch.tensor(method.barostat_dof, dtype=torch.float64))
    return out


def child_host(steps):
    import pytest

    import test_step_loop as t

    t.LAMBDA = (1.0 + 1e-7, 1.0, 1.0 - 1e-7)
    out = {}
    for path in HOST_PATHS:
        mp = pytest.MonkeyPatch()
        try:
            sim, log = t.make_sim(path, mp, writer=0, updater=0, tuner=0)
            sim.run(100)
            best = None
            for _ in range(6):
                del log[:]
                t0 = time.thread_time()
                sim.run(steps)
                dt = time.thread_time() - t0
                best = dt if best is None else min(best, dt)
            out[path] = 1e6 * best / steps
        finally:
            mp.undo()
    return out


def run_child(mode, checkout, steps):
    cmd = [sys.executable, os.path.abspath(__file__), mode, "--child", "--checkout", os.path.abspath(checkout), "--steps", str(steps)]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, check=True, timeout=1100)
    return json.loads(res.stdout.decode().strip().split("\n")[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["digests", "host"])
    ap.add_argument("--checkout", action="append", required=True, help="a checkout with a built libazp.so; repeat to compare")
    ap.add_argument("--processes", type=int, default=5, help="host: child processes per checkout")
    ap.add_argument("--steps", type=int, default=10000, help="host: steps per timed run")
    ap.add_argument("--json", default=None, help="write the raw numbers here")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        sys.path[:0] = [args.checkout[0], os.path.join(ROOT, "tests")]
        print(json.dumps(child_digests() if args.mode == "digests" else child_host(args.steps)), flush=True)
        return
    if args.mode == "digests":
        res = {c: run_child("digests", c, args.steps) for c in args.checkout}
        print("| run | " + " | ".join(args.checkout) + " |\n|---|" + "---|" * len(args.checkout))
        for k in res[args.checkout[0]]:
            print("| %s | " % k + " | ".join("`%s`" % res[c][k] for c in args.checkout) + " |")
        if len(args.checkout) > 1:
            print("equal" if all(res[c] == res[args.checkout[0]] for c in args.checkout) else "DIFFERENT")
    else:
        runs = {c: [] for c in args.checkout}
        for _ in range(args.processes):
            for c in args.checkout:
                runs[c].append(run_child("host", c, args.steps))
        res = runs
        print("us per step, smallest - largest of %d processes (median)\n" % args.processes)
        print("| path | " + " | ".join(args.checkout) + " |\n|---|" + "---|" * len(args.checkout))
        for p in HOST_PATHS:
            cells = []
            for c in args.checkout:
                v = sorted(r[p] for r in runs[c])
                cells.append("%.2f - %.2f (%.2f)" % (v[0], v[-1], v[len(v) // 2]))
            print("| %s | " % p + " | ".join(cells) + " |")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
