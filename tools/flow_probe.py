"""Event-timed cost of the fused Langevin-in-flow kernel (azp_integrate_langevin_flow_step_two_one, constant and
parabolic flow) against the fused NVE kernel (azp_integrate_nve_step_two_one) at N = 2^20, in one process: the
north-star FCC positions, Gaussian velocities, masses in [1, 2), a random net force, all particles integrated.
Per kernel: microseconds per call (device events around `--calls` back-to-back calls after a warm-up), the bytes it
moves per particle and the share of the 6.29 TB/s measured copy bandwidth that makes.

  python tools/flow_probe.py [--calls 200] [--out profiles/flow_methods_table.md] [--json out.json]
  python tools/flow_probe.py --rocprof DIR   # then the same calls once more under rocprofv3 --kernel-trace --stats
                                             # (a separate child process; output under DIR)
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

COPY_BW = 6.29e12  # B/s, measured device-to-device copy bandwidth of one MI355X
# bytes per particle of one fused call: reads + writes of the rows it touches
BYTES = {
    "nve_step_two_one": 32 + 32 + 32 + 32 + 32 + 12 + 12,              # vel r/w, net_force r, pos r/w, image r/w = 184
    "langevin_step_two_one": 32 + 32 + 32 + 32 + 32 + 4 + 32 + 12 + 12,  # + tag r, accel w = 220
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--rocprof", default=None, help="after timing, rerun under rocprofv3 --kernel-trace --stats into DIR")
    args = ap.parse_args()

    import torch

    import azplugins_amd as azp
    from azplugins_amd import _lib, flow
    from azplugins_amd import synthetic as syn

    if not torch.cuda.is_available():
        raise SystemExit("flow_probe: no GPU (the numbers come from a GPU run only)")
    dev = torch.device("cuda:0")
    cfg = syn.config_north_star()
    N = cfg["xyz"].shape[0]
    L = [float(v) for v in cfg["L"]]
    tag = np.arange(N, dtype=np.uint64)
    vel = np.stack([syn.normal(21, tag, c) for c in range(3)] + [1.0 + syn.u01(22, tag, 0)], axis=1)
    force = np.stack([syn.normal(23, tag, c) for c in range(3)] + [np.zeros(N)], axis=1)
    pos = syn.pos4(cfg["xyz"])
    lib = _lib.lib()
    stream = _lib.raw_stream(dev)
    box = azp.Box(*L).to_c()

    def up(a, dtype=None):
        return torch.from_numpy(np.ascontiguousarray(a if dtype is None else a.astype(dtype))).to(dev)

    d_tag = up(np.arange(N, dtype=np.int32))
    d_gamma = up(np.array([1.0]))
    d_force = up(force)

    def nve_case():
        d_pos, d_vel, d_img = up(pos), up(vel), torch.zeros((N, 3), dtype=torch.int32, device=dev)
        a = _lib.NVEArgs()
        a.d_pos, a.d_vel, a.d_net_force, a.d_image = d_pos.data_ptr(), d_vel.data_ptr(), d_force.data_ptr(), d_img.data_ptr()
        a.box, a.dt, a.N = box, 0.005, N

        def call(k):
            _lib.check(lib.azp_integrate_nve_step_two_one(C.byref(a), stream))
        return call, (d_pos, d_vel, d_img)

    def langevin_case(field):
        d_pos, d_vel, d_img = up(pos), up(vel), torch.zeros((N, 3), dtype=torch.int32, device=dev)
        d_acc = torch.zeros((N, 4), dtype=torch.float64, device=dev)
        a = _lib.FlowMethodArgs()
        a.d_pos, a.d_vel, a.d_accel, a.d_net_force = d_pos.data_ptr(), d_vel.data_ptr(), d_acc.data_ptr(), d_force.data_ptr()
        a.d_image, a.d_tag, a.d_gamma, a.d_type_mask = d_img.data_ptr(), d_tag.data_ptr(), d_gamma.data_ptr(), None
        a.box, a.dt, a.kT, a.seed, a.N, a.ntypes = box, 0.005, 1.0, 7, N, 1
        a.flow = field._c()

        def call(k):
            a.timestep = k
            _lib.check(lib.azp_integrate_langevin_flow_step_two_one(C.byref(a), stream))
        return call, (d_pos, d_vel, d_img, d_acc)

    cases = [
        ("nve_step_two_one", "nve_step_two_one", nve_case()),
        ("langevin_step_two_one constant", "langevin_step_two_one", langevin_case(flow.ConstantFlow(velocity=(1.0, 0.0, 0.0)))),
        ("langevin_step_two_one parabolic", "langevin_step_two_one", langevin_case(flow.ParabolicFlow(mean_velocity=1.0, separation=L[1]))),
    ]
    rows = []
    for rnd in range(2):  # two interleaved rounds: drift of the clock shows up as a difference between them
        for name, kind, (call, keep) in cases:
            for k in range(args.warmup):
                call(k)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(args.calls):
                call(args.warmup + k)
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / args.calls
            bw = BYTES[kind] * N / (us * 1e-6)
            rows.append(dict(round=rnd, case=name, us=us, bytes_per_particle=BYTES[kind], bandwidth_TBps=bw / 1e12,
                             share_of_copy_bw=bw / COPY_BW))
            print(json.dumps(rows[-1]), flush=True)
    for name, _, (call, keep) in cases:
        assert all(bool(torch.isfinite(t.double()).all()) for t in keep), name
    nve = min(r["us"] for r in rows if r["case"] == "nve_step_two_one")
    lines = ["| kernel | round | us / call | B / particle | TB/s | share of 6.29 TB/s | vs NVE (best) |", "|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %s | %d | %.1f | %d | %.2f | %.2f | %.2fx |" % (r["case"], r["round"], r["us"], r["bytes_per_particle"],
                                                                     r["bandwidth_TBps"], r["share_of_copy_bw"], r["us"] / nve))
    head = "device: %s, N = %d, %d calls after %d warm-up calls per round" % (torch.cuda.get_device_name(0), N, args.calls, args.warmup)
    table = "\n".join(lines)
    print(head)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(head + "\n\n" + table + "\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    if args.rocprof:
        # a separate run: the profiler's own process tree, with the kernels of the same calls
        os.makedirs(args.rocprof, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", args.rocprof, "-o", "flow", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--calls", "50", "--warmup", "5"]
        print(" ".join(cmd), flush=True)
        rc = subprocess.call(cmd)
        print("rocprofv3 exit status %d; output under %s" % (rc, args.rocprof))
        if rc != 0:
            raise SystemExit(rc)


if __name__ == "__main__":
    main()
