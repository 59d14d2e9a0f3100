"""Event-timed cost of the thermostatted NVE step at N = 2^20 (csrc/thermostat.hip) against the parent's kernels, through
the C ABI on one set of arrays (random positions in a cubic box at rho* = 0.8, thermal velocities, random forces), all in
one process, the cases interleaved:

  (a) thermostatted: azp_thermostat_advance + azp_thermostat_step_one + azp_thermostat_step_two  (per step)
  (b) un-fused NVE:  azp_integrate_nve_step_two + azp_integrate_nve_step_one
  (c) fused NVE:     azp_integrate_nve_step_two_one
  and each thermostat kernel on its own, the kinetic pass included.

  python tools/thermostat_probe.py [--n 1048576] [--calls 200] [--repeats 5] [--out profiles/thermostat_probe.md] [--json ...]
"""

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # B/s, MI355X spec
# bytes per particle: step one 184 (vel 32 read + 32 written, force 32, pos 32 + 32, image 12 + 12), step two 96 (vel
# 32 + 32, force 32), the kinetic pass 32; the fused NVE kernel 184


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2**20)
    ap.add_argument("--calls", type=int, default=200, help="timed calls per case and repeat")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None, help="write the markdown summary here")
    ap.add_argument("--json", default=None, help="write the raw numbers here")
    args = ap.parse_args()

    import torch

    from azplugins_amd import _lib

    if not torch.cuda.is_available():
        raise SystemExit("thermostat_probe: no GPU (the numbers come from a GPU run only)")
    N = args.n
    L = (N / 0.8) ** (1.0 / 3.0)
    rng = np.random.default_rng(1)
    dev = "cuda:0"
    pos = torch.from_numpy(np.c_[rng.uniform(-0.5 * L, 0.5 * L, (N, 3)), np.zeros(N)]).to(dev)
    vel0 = torch.from_numpy(np.c_[rng.normal(size=(N, 3)), np.ones(N)]).to(dev)
    vel = vel0.clone()
    force = torch.from_numpy(np.c_[rng.normal(0.0, 10.0, (N, 3)), np.zeros(N)]).to(dev)
    image = torch.zeros((N, 3), dtype=torch.int32, device=dev)
    lib = _lib.lib()
    stream = _lib.raw_stream(dev)
    need = C.c_uint64(0)
    _lib.check(lib.azp_thermostat_partials_size(N, C.byref(need)))
    partials = torch.zeros(need.value // 8, dtype=torch.float64, device=dev)
    state = torch.zeros(_lib.THERMOSTAT_NSTATE, dtype=torch.float64, device=dev)

    t = _lib.ThermostatArgs()
    t.d_pos, t.d_vel, t.d_net_force, t.d_image = pos.data_ptr(), vel.data_ptr(), force.data_ptr(), image.data_ptr()
    t.d_partials, t.partials_bytes, t.d_state = partials.data_ptr(), need.value, state.data_ptr()
    t.box = _lib.make_box(L)
    t.dt, t.kT, t.tau, t.ndof, t.seed, t.N = 0.005, 1.0, 0.5, float(3 * N - 3), 1, N
    n = _lib.NVEArgs()
    n.d_pos, n.d_vel, n.d_net_force, n.d_image = pos.data_ptr(), vel.data_ptr(), force.data_ptr(), image.data_ptr()
    n.box, n.dt, n.N = t.box, t.dt, N

    def call(fn, a):
        _lib.check(fn(C.byref(a), stream))

    step = [0]

    def thermostatted(kind):
        def fn():
            t.kind, t.timestep = kind, step[0]
            step[0] += 1
            call(lib.azp_thermostat_advance, t)
            call(lib.azp_thermostat_step_one, t)
            call(lib.azp_thermostat_step_two, t)
        return fn

    def only(kind, name):
        def fn():
            t.kind, t.timestep = kind, step[0]
            step[0] += 1
            call(getattr(lib, name), t)
        return fn

    cases = {
        "thermostatted step, Bussi (advance + step one + step two)": thermostatted(_lib.THERMOSTAT_BUSSI),
        "thermostatted step, MTTK": thermostatted(_lib.THERMOSTAT_MTTK),
        "thermostatted step, Berendsen": thermostatted(_lib.THERMOSTAT_BERENDSEN),
        "NVE un-fused (step two + step one)": lambda: (call(lib.azp_integrate_nve_step_two, n), call(lib.azp_integrate_nve_step_one, n)),
        "NVE fused (step two + one in one kernel)": lambda: call(lib.azp_integrate_nve_step_two_one, n),
        "azp_thermostat_advance alone (Bussi)": only(_lib.THERMOSTAT_BUSSI, "azp_thermostat_advance"),
        "azp_thermostat_step_one alone": only(_lib.THERMOSTAT_BUSSI, "azp_thermostat_step_one"),
        "azp_thermostat_step_two alone": only(_lib.THERMOSTAT_BUSSI, "azp_thermostat_step_two"),
        "azp_thermostat_kinetic alone": only(_lib.THERMOSTAT_BUSSI, "azp_thermostat_kinetic"),
        "azp_integrate_nve_step_one alone": lambda: call(lib.azp_integrate_nve_step_one, n),
        "azp_integrate_nve_step_two alone": lambda: call(lib.azp_integrate_nve_step_two, n),
    }
    bytes_per_particle = {
        "thermostatted step, Bussi (advance + step one + step two)": 280, "thermostatted step, MTTK": 280,
        "thermostatted step, Berendsen": 280, "NVE un-fused (step two + step one)": 280,
        "NVE fused (step two + one in one kernel)": 184, "azp_thermostat_advance alone (Bussi)": 0,
        "azp_thermostat_step_one alone": 184, "azp_thermostat_step_two alone": 96, "azp_thermostat_kinetic alone": 32,
        "azp_integrate_nve_step_one alone": 184, "azp_integrate_nve_step_two alone": 96,
    }

    def events(fn):
        # (the forces are random, not those of the positions: the velocities are reset so that nothing runs away)
        vel.copy_(vel0)
        call(lib.azp_thermostat_kinetic, t)
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.calls  # us

    times = {k: [] for k in cases}
    for r in range(args.repeats):
        order = list(cases) if r % 2 == 0 else list(cases)[::-1]
        for k in order:
            times[k].append(events(cases[k]))
    res = dict(N=N, device=torch.cuda.get_device_name(0), calls=args.calls, repeats=args.repeats,
               us={k: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v))) for k, v in times.items()})
    torch.cuda.synchronize()
    assert bool(torch.isfinite(vel).all()) and bool(torch.isfinite(state).all())
    print(json.dumps(res), flush=True)

    lines = ["device: %s, N = %d; device events around %d back-to-back calls after %d warm-up calls, %d repeats in alternating "
             "order, median (min - max)" % (res["device"], N, args.calls, args.warmup, args.repeats), "",
             "| case | us per step or call | bytes per particle | share of the 8 TB/s HBM peak |", "|---|---|---|---|"]
    for k in cases:
        u = res["us"][k]
        b = bytes_per_particle[k]
        share = "%.2f" % (b * N / (u["median"] * 1e-6) / HBM_PEAK) if b else "-"
        lines.append("| %s | %.1f (%.1f - %.1f) | %s | %s |" % (k, u["median"], u["min"], u["max"], b if b else "-", share))
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
