"""Event-timed cost of the wall kernels at N = 2^20 on the north-star liquid's positions, for both potentials, against
the planar harmonic barrier in the same process (the barrier kernel moves the same 64 B per particle as a one-plane
wall: it is the yardstick):

  one plane      a substrate on the lower z face of the box
  slit           the substrate and a facing plane on the upper z face
  16 walls       the slit and 14 more planes, spheres and cylinders
  net forces     azp_wall_net_forces_* (the force on each wall) for the slit and for the 16 walls
  barrier        azp_external_planar_harmonic_barrier, d_virial NULL as for the walls

Every call sits between its own pair of device events; the cases are interleaved, so a drift of the clock touches all
alike. The table and the comparison go to --out (profiles/wall.md).

  python tools/wall_probe.py [--reps 200] [--warmup 20] [--out profiles/wall.md] [--json out.json]
  python tools/wall_probe.py --rocprof DIR   # afterwards a few calls once more, in a child process under
                                             # rocprofv3 --kernel-trace --stats (no counters), output under DIR
"""

import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(us):
    us = np.sort(np.asarray(us))
    return dict(median_us=float(np.median(us)), min_us=float(us[0]), p10_us=float(us[len(us) // 10]),
                p90_us=float(us[(9 * len(us)) // 10]), max_us=float(us[-1]), reps=int(us.size))


def wall_sets(azp, L):
    h = [0.5 * v for v in L]
    W = azp.wall
    slit = [W.Plane(origin=(0, 0, -h[2]), normal=(0, 0, 1)), W.Plane(origin=(0, 0, h[2]), normal=(0, 0, -1))]
    more = [W.Plane(origin=(-h[0], 0, 0), normal=(1, 0, 0)), W.Plane(origin=(h[0], 0, 0), normal=(-1, 0, 0)),
            W.Plane(origin=(0, -h[1], 0), normal=(0, 1, 0)), W.Plane(origin=(0, h[1], 0), normal=(0, -1, 0)),
            W.Plane(origin=(0, 0, 0), normal=(1, 1, 0)), W.Plane(origin=(0, 0, 0), normal=(1, 2, 2)),
            W.Sphere(0.8 * h[0], inside=True), W.Sphere(0.3 * h[0], inside=False),
            W.Sphere(0.5 * h[0], origin=(0.2 * h[0], 0, 0), inside=True), W.Sphere(0.1 * h[0], origin=(0, 0.5 * h[1], 0), inside=False),
            W.Cylinder(0.7 * h[0], inside=True), W.Cylinder(0.2 * h[0], axis=(1, 1, 0), inside=False),
            W.Cylinder(0.6 * h[0], origin=(0, 0.1 * h[1], 0), axis=(1, 0, 0), inside=True),
            W.Cylinder(0.15 * h[0], origin=(0.3 * h[0], 0, 0), axis=(0, 1, 1), inside=False)]
    return {"one plane": slit[:1], "slit": slit, "16 walls": slit + more}


def kernel_cases(reps, warmup):
    import torch

    import azplugins_amd as azp
    from azplugins_amd import _lib
    from azplugins_amd import synthetic as syn

    dev = torch.device("cuda:0")
    cfg = syn.config_north_star()
    N = cfg["xyz"].shape[0]
    L = [float(v) for v in cfg["L"]]
    pos = torch.from_numpy(syn.pos4(cfg["xyz"], np.zeros(N, dtype=np.int64))).to(dev)
    force = torch.empty((N, 4), dtype=torch.float64, device=dev)
    lib = _lib.lib()
    stream = _lib.raw_stream(dev)
    box = azp.Box(*L).to_c()
    sets = wall_sets(azp, L)
    potentials = {"LJ93": (azp.wall.LJ93, dict(epsilon=1.0, sigma=1.0, r_cut=3.0)),
                  "Colloid": (azp.wall.Colloid, dict(A=100.0, sigma=1.0, a=0.5, r_cut=3.0, r_extrap=0.8))}
    keep = []  # tensors the calls point at
    cases = []
    in_range = {}

    def wall_args(cls, params, walls):
        f = cls(walls, mode="shift")
        f.params["A"] = params
        table = torch.tensor([f._row(f.params.get_raw("A"))], dtype=torch.float64, device=dev)
        keep.append(table)
        a = _lib.WallArgs()
        a.d_force, a.N, a.ntypes, a.d_pos, a.box, a.d_params = force.data_ptr(), N, 1, pos.data_ptr(), box, table.data_ptr()
        a.n_walls = len(walls)
        for k, w in enumerate(walls):
            a.walls[k] = w._c()
        return f, a

    for pname, (cls, params) in potentials.items():
        for sname, walls in sets.items():
            f, a = wall_args(cls, params, walls)
            entry = getattr(lib, f._entry)
            name = "%s, %s" % (pname, sname)
            cases.append((name, lambda a=a, entry=entry, name=name: _lib.check(entry(C.byref(a), stream), name)))
            if sname != "one plane":
                need = C.c_uint64(0)
                _lib.check(lib.azp_wall_net_forces_scratch_size(C.byref(a), C.byref(need)), "scratch size")
                out = torch.empty((len(walls), 4), dtype=torch.float64, device=dev)
                scratch = torch.empty(int(need.value), dtype=torch.uint8, device=dev)
                keep.extend([out, scratch])
                net = getattr(lib, f._net_entry)
                nname = "%s, net forces, %s" % (pname, sname)
                cases.append((nname, lambda a=a, net=net, out=out, scratch=scratch, nname=nname: _lib.check(
                    net(C.byref(a), out.data_ptr(), scratch.data_ptr(), scratch.numel(), stream), nname)))
            # share of the particles inside the cutoff of at least one wall (what the evaluator runs for)
            entry(C.byref(a), stream)
            torch.cuda.synchronize()
            in_range[name] = float((force[:, 3] != 0.0).double().mean().item())

    b = _lib.BarrierArgs()
    btable = torch.tensor([[100.0, 0.0]], dtype=torch.float64, device=dev)
    b.d_force, b.N, b.ntypes, b.d_pos, b.box, b.d_params = force.data_ptr(), N, 1, pos.data_ptr(), box, btable.data_ptr()
    b.location = 0.5 * L[1] - 3.0  # the same share of the box in range as a wall with r_cut = 3
    barrier = "azp_external_planar_harmonic_barrier"
    cases.append((barrier, lambda: _lib.check(lib.azp_external_planar_harmonic_barrier(C.byref(b), stream), barrier)))
    lib.azp_external_planar_harmonic_barrier(C.byref(b), stream)
    torch.cuda.synchronize()
    in_range[barrier] = float((force[:, 3] != 0.0).double().mean().item())

    times = {name: [] for name, _ in cases}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for k in range(warmup + reps):
        for name, call in cases:
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            if k >= warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    rows = []
    ref_us = float(np.median(times[barrier]))
    for name, _ in cases:
        r = dict(case=name, **_stats(times[name]))
        r["vs_barrier"] = r["median_us"] / ref_us
        if "net forces" not in name:
            r["TB_per_s"] = 64.0 * N / (r["median_us"] * 1e-6) / 1e12
            r["in_range"] = in_range[name]
        rows.append(r)
        print(json.dumps(r), flush=True)
    return N, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wall.md"))
    ap.add_argument("--json", default=None)
    ap.add_argument("--rocprof", default=None, help="after timing, rerun a few calls under rocprofv3 --kernel-trace --stats into DIR")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("wall_probe: no GPU (the numbers come from a GPU run only)")
    N, rows = kernel_cases(args.reps, args.warmup)
    by = {r["case"]: r for r in rows}
    bar = by["azp_external_planar_harmonic_barrier"]
    one = by["LJ93, one plane"]
    inside = bar["p10_us"] <= one["median_us"] <= bar["p90_us"]
    lines = ["# Wall kernels at N = 2^20 against the planar harmonic barrier", "",
             "Written by `python tools/wall_probe.py --reps %d --warmup %d`." % (args.reps, args.warmup), "",
             "device: %s, N = %d (north-star liquid, FCC 64^3 x 4 at rho* = 0.8, one type), %d timed calls per case after %d "
             "warm-up calls, every call between its own pair of device events, the cases interleaved. A force call reads "
             "32 B and writes 32 B per particle (no virial buffer given, for the walls and for the barrier); TB/s is 64 B x "
             "N over the median. `in range` is the share of the particles with a non-zero result."
             % (torch.cuda.get_device_name(0), N, args.reps, args.warmup), "",
             "| call | median us | min | p10 | p90 | max | x barrier | TB/s | in range |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %s | %.1f | %.1f | %.1f | %.1f | %.1f | %.2f | %s | %s |" % (
            r["case"], r["median_us"], r["min_us"], r["p10_us"], r["p90_us"], r["max_us"], r["vs_barrier"],
            "%.2f" % r["TB_per_s"] if "TB_per_s" in r else "", "%.3f" % r["in_range"] if "in_range" in r else ""))
    lines += ["", "The one-plane LJ93 kernel's median, %.1f us, lies %s the barrier kernel's own p10 - p90 spread, %.1f - %.1f us "
              "(median %.1f us)." % (one["median_us"], "inside" if inside else "OUTSIDE", bar["p10_us"], bar["p90_us"], bar["median_us"])]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(N=N, rows=rows), f, indent=1)
    if args.rocprof:
        os.makedirs(args.rocprof, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", args.rocprof, "-o", "wall", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--reps", "20", "--warmup", "5", "--out", ""]
        print(" ".join(cmd), flush=True)
        rc = subprocess.call(cmd)
        print("rocprofv3 exit status %d; output under %s" % (rc, args.rocprof))
        if rc != 0:
            raise SystemExit(rc)


if __name__ == "__main__":
    main()
