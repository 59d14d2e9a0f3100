"""Event-timed cost of the type-update calls at N = 2^20 (the north-star liquid's positions, two types), each call
between its own pair of device events, the type words restored before every call (outside the timed window):

  azp_evaporate, thin slab   about 1 % of the particles are candidates, Nmax = 64
  azp_evaporate, worst case  every particle a candidate, Nmax = N / 2
  azp_evaporate, no limit    every candidate goes (one kernel)
  azp_type_update_region     half the box inside
  azp_integrate_nve_step_one the yardstick: one streaming pass over the particle arrays, same state, same process

and the step time of an MD run (PerturbedLJ, NVE) with an evaporator every 10 steps, with a do-nothing updater every 10
steps (the forced neighbor-list rebuild alone) and with neither.

  python tools/evaporate_probe.py [--reps 200] [--md-steps 300] [--out profiles/evaporate_table.md] [--json out.json]
  python tools/evaporate_probe.py --rocprof DIR   # afterwards a few updating calls once more, in a child process under
                                                  # rocprofv3 --kernel-trace --stats (no counters), output under DIR
"""

import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(us):
    us = np.sort(np.asarray(us))
    return dict(median_us=float(np.median(us)), min_us=float(us[0]), p10_us=float(us[len(us) // 10]),
                p90_us=float(us[(9 * len(us)) // 10]), max_us=float(us[-1]), reps=int(us.size))


def kernel_cases(reps, warmup):
    import torch

    import azplugins_amd as azp
    from azplugins_amd import _lib
    from azplugins_amd import synthetic as syn

    dev = torch.device("cuda:0")
    cfg = syn.config_north_star()
    N = cfg["xyz"].shape[0]
    L = [float(v) for v in cfg["L"]]
    tag = np.arange(N, dtype=np.uint64)
    pos0 = torch.from_numpy(syn.pos4(cfg["xyz"], np.zeros(N, dtype=np.int64))).to(dev)
    vel = torch.from_numpy(np.stack([syn.normal(21, tag, c) for c in range(3)] + [np.ones(N)], axis=1)).to(dev)
    force = torch.from_numpy(np.stack([syn.normal(23, tag, c) for c in range(3)] + [np.zeros(N)], axis=1)).to(dev)
    image = torch.zeros((N, 3), dtype=torch.int32, device=dev)
    d_tag = torch.from_numpy(np.arange(N, dtype=np.int32)).to(dev)
    d_pos = pos0.clone()
    lib = _lib.lib()
    stream = _lib.raw_stream(dev)
    scratch = torch.empty(int(lib.azp_evaporate_scratch_size(N)), dtype=torch.uint8, device=dev)
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    z = cfg["xyz"][:, 2]
    thin_hi = float(np.quantile(z, 0.01))  # about 1 % of the particles lie under it

    def evaporate(lo, hi, Nmax):
        a = _lib.EvaporateArgs()
        a.d_pos, a.d_tag, a.N = d_pos.data_ptr(), d_tag.data_ptr(), N
        a.solvent_type, a.evaporated_type, a.Nmax = 0, 1, _lib.EVAPORATE_NO_LIMIT if Nmax is None else Nmax
        a.z_lo, a.z_hi, a.seed = lo, hi, 7
        a.d_scratch, a.scratch_bytes, a.d_counts = scratch.data_ptr(), scratch.numel(), counts.data_ptr()

        def call(k):
            a.timestep = k
            _lib.check(lib.azp_evaporate(C.byref(a), stream), "azp_evaporate")
        return call

    def region():
        a = _lib.TypeUpdateArgs()
        a.d_pos, a.N, a.inside_type, a.outside_type, a.z_lo, a.z_hi = d_pos.data_ptr(), N, 1, 0, -0.25 * L[2], 0.25 * L[2]
        return lambda k: _lib.check(lib.azp_type_update_region(C.byref(a), stream), "azp_type_update_region")

    def nve():
        a = _lib.NVEArgs()
        a.d_pos, a.d_vel, a.d_net_force, a.d_image = d_pos.data_ptr(), vel.data_ptr(), force.data_ptr(), image.data_ptr()
        a.box, a.dt, a.N = azp.Box(*L).to_c(), 1e-6, N
        return lambda k: _lib.check(lib.azp_integrate_nve_step_one(C.byref(a), stream), "azp_integrate_nve_step_one")

    cases = [("azp_evaporate thin slab (1 %, Nmax 64)", evaporate(-0.5 * L[2], thin_hi, 64)),
             ("azp_evaporate worst case (all, Nmax N/2)", evaporate(-0.5 * L[2], 0.5 * L[2], N // 2)),
             ("azp_evaporate no limit (all)", evaporate(-0.5 * L[2], 0.5 * L[2], None)),
             ("azp_type_update_region", region()),
             ("azp_integrate_nve_step_one", nve())]
    times = {name: [] for name, _ in cases}
    seen = {}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for k in range(warmup + reps):  # the cases interleaved: a drift of the clock touches all alike
        for name, call in cases:
            d_pos.copy_(pos0)
            e0.record()
            call(k)
            e1.record()
            e1.synchronize()
            if k >= warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)
            if name.startswith("azp_evaporate"):
                seen[name] = counts.cpu().numpy().view(np.uint32).tolist()
    rows = []
    nve_us = float(np.median(times["azp_integrate_nve_step_one"]))
    for name, _ in cases:
        r = dict(case=name, **_stats(times[name]))
        r["vs_nve_step_one"] = r["median_us"] / nve_us
        if name in seen:
            r["candidates"], r["picked"] = seen[name]
        rows.append(r)
        print(json.dumps(r), flush=True)
    return N, rows


def md_cases(steps):
    """ms per step of the north-star NVE run: plain, with a do-nothing updater every 10 steps (the forced rebuild of the
    list and the tile plan alone), with the evaporator every 10 steps."""
    import torch

    import azplugins_amd as azp
    from azplugins_amd import synthetic as syn
    from azplugins_amd.evaporate import ParticleEvaporator
    from azplugins_amd.update import _Updater

    class RebuildOnly(_Updater):
        def _update(self, sim, timestep):
            pass

    cfg = syn.config_north_star()
    N = cfg["xyz"].shape[0]
    tag = np.arange(N, dtype=np.uint64)
    vel = np.stack([syn.normal(31, tag, c) for c in range(3)], axis=1)
    thin_hi = float(np.quantile(cfg["xyz"][:, 2], 0.01))
    rows = []
    for name in ("no updater", "forced rebuild every 10 steps", "evaporator every 10 steps (Nmax 64)"):
        snap = azp.Snapshot.from_arrays(cfg["xyz"], cfg["L"], types=("S", "E"), velocity=vel - vel.mean(axis=0))
        sim = azp.Simulation(device="cuda:0", seed=3)
        sim.create_state_from_snapshot(snap)
        nl = azp.nlist.Cell(buffer=cfg["r_buff"])
        plj = azp.pair.PerturbedLennardJones(nlist=nl, default_r_cut=cfg["r_cut"], mode="shift")
        for pair in (("S", "S"), ("S", "E"), ("E", "E")):
            plj.params[pair] = dict(cfg["params"], epsilon=0.0 if "E" in pair else cfg["params"]["epsilon"])
        sim.operations.integrator = azp.Integrator(dt=0.002, forces=[plj], methods=[azp.ConstantVolume()])
        if name.startswith("forced"):
            sim.operations.add(RebuildOnly(10))
        elif name.startswith("evaporator"):
            sim.operations.add(ParticleEvaporator(10, "S", "E", lo=-0.5 * float(cfg["L"][2]), hi=thin_hi, Nmax=64))
        sim.run(50)  # warm-up: first builds, plan, code objects
        torch.cuda.synchronize()
        b0 = nl.num_builds
        t0 = time.perf_counter()
        sim.run(steps)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / steps
        rows.append(dict(case=name, ms_per_step=ms, steps=steps, list_builds=nl.num_builds - b0,
                         evaporated=int((sim.state.typeid_host == 1).sum())))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--md-steps", type=int, default=300)
    ap.add_argument("--out", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--rocprof", default=None, help="after timing, rerun a few calls under rocprofv3 --kernel-trace --stats into DIR")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("evaporate_probe: no GPU (the numbers come from a GPU run only)")
    N, rows = kernel_cases(args.reps, args.warmup)
    md = md_cases(args.md_steps) if args.md_steps > 0 else []
    head = "device: %s, N = %d, %d timed calls per case after %d warm-up calls, cases interleaved" % (
        torch.cuda.get_device_name(0), N, args.reps, args.warmup)
    lines = ["| call | median us | min | p10 | p90 | max | x nve_step_one | candidates | picked |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %s | %.1f | %.1f | %.1f | %.1f | %.1f | %.2f | %s | %s |" % (
            r["case"], r["median_us"], r["min_us"], r["p10_us"], r["p90_us"], r["max_us"], r["vs_nve_step_one"],
            r.get("candidates", ""), r.get("picked", "")))
    if md:
        lines += ["", "| MD run, %d steps | ms / step | list builds | evaporated |" % md[0]["steps"], "|---|---|---|---|"]
        lines += ["| %s | %.4f | %d | %d |" % (r["case"], r["ms_per_step"], r["list_builds"], r["evaporated"]) for r in md]
    table = "\n".join(lines)
    print(head)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(head + "\n\n" + table + "\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(kernels=rows, md=md), f, indent=1)
    if args.rocprof:
        os.makedirs(args.rocprof, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", args.rocprof, "-o", "evaporate", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--reps", "10", "--warmup", "2", "--md-steps", "0"]
        print(" ".join(cmd), flush=True)
        rc = subprocess.call(cmd)
        print("rocprofv3 exit status %d; output under %s" % (rc, args.rocprof))
        if rc != 0:
            raise SystemExit(rc)


if __name__ == "__main__":
    main()
