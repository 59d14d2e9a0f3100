"""Event-timed cost of the two FIRE passes at N = 2^20 (csrc/fire.hip) against their thermostat counterparts
(csrc/thermostat.hip), through the C ABI on one set of arrays (random positions in a cubic box at rho* = 0.8, thermal
velocities, random forces), all in one process, the cases interleaved:

  azp_fire_step_two        against  azp_thermostat_step_two   (96 B per particle; 4 x n_blocks partials against 1 x)
  azp_fire_step_one        against  azp_thermostat_step_one   (184 B per particle)
  and the measure pass, the advance and the passes of a converged state (which return at once) on their own.

Each FIRE pass is expected to take no longer than its counterpart plus the run-to-run spread (max - min over the
repeats) measured for that counterpart in the same process; the summary says whether it does.

  python tools/fire_probe.py [--n 1048576] [--calls 200] [--repeats 5] [--out profiles/fire.md] [--json ...]
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
        raise SystemExit("fire_probe: no GPU (the numbers come from a GPU run only)")
    N = args.n
    L = (N / 0.8) ** (1.0 / 3.0)
    rng = np.random.default_rng(1)
    dev = "cuda:0"
    pos = torch.from_numpy(np.c_[rng.uniform(-0.5 * L, 0.5 * L, (N, 3)), np.zeros(N)]).to(dev)
    vel0 = torch.from_numpy(np.c_[rng.normal(size=(N, 3)), np.ones(N)]).to(dev)
    vel = vel0.clone()
    force = torch.from_numpy(np.c_[rng.normal(0.0, 10.0, (N, 3)), rng.normal(size=N)]).to(dev)
    image = torch.zeros((N, 3), dtype=torch.int32, device=dev)
    lib = _lib.lib()
    stream = _lib.raw_stream(dev)
    need = C.c_uint64(0)
    _lib.check(lib.azp_fire_partials_size(N, C.byref(need)))
    partials = torch.zeros(need.value // 8, dtype=torch.float64, device=dev)  # (the thermostat uses its first quarter)
    t_state = torch.zeros(_lib.THERMOSTAT_NSTATE, dtype=torch.float64, device=dev)
    t_state[_lib.THERMOSTAT_ALPHA] = 1.0

    def fire_state(**slots):
        s = [0.0] * _lib.FIRE_NSTATE
        # (the coefficients of a step under way; KEEP + MIX |f| / |v| stays near one, so nothing runs away)
        s[_lib.FIRE_DT], s[_lib.FIRE_ALPHA], s[_lib.FIRE_KEEP], s[_lib.FIRE_MIX] = 0.005, 0.1, 0.9, 0.005
        for k, v in slots.items():
            s[getattr(_lib, "FIRE_" + k)] = v
        return torch.tensor(s, dtype=torch.float64, device=dev)

    f_state, f_done = fire_state(), fire_state(CONVERGED=1.0)

    f = _lib.FireArgs()
    f.d_pos, f.d_vel, f.d_net_force, f.d_image = pos.data_ptr(), vel.data_ptr(), force.data_ptr(), image.data_ptr()
    f.d_partials, f.partials_bytes, f.d_state = partials.data_ptr(), need.value, f_state.data_ptr()
    f.box = _lib.make_box(L)
    f.dt_max, f.force_tol, f.energy_tol, f.N = 0.005, 1e-3, 1e-7, N
    f.finc_dt, f.fdec_dt, f.alpha_start, f.fdec_alpha, f.min_steps_adapt, f.min_steps_conv = 1.1, 0.5, 0.1, 0.99, 5, 10
    t = _lib.ThermostatArgs()
    t.d_pos, t.d_vel, t.d_net_force, t.d_image = pos.data_ptr(), vel.data_ptr(), force.data_ptr(), image.data_ptr()
    t.d_partials, t.partials_bytes, t.d_state = partials.data_ptr(), need.value, t_state.data_ptr()
    t.box = f.box
    t.dt, t.kT, t.tau, t.ndof, t.seed, t.N, t.kind = 0.005, 1.0, 0.5, float(3 * N - 3), 1, N, _lib.THERMOSTAT_BERENDSEN

    def call(fn, a):
        _lib.check(fn(C.byref(a), stream))

    def fire(name, state=f_state):
        def fn():
            f.d_state = state.data_ptr()
            call(getattr(lib, name), f)
        return fn

    cases = {
        "azp_fire_step_two": fire("azp_fire_step_two"),
        "azp_thermostat_step_two": lambda: call(lib.azp_thermostat_step_two, t),
        "azp_fire_step_one": fire("azp_fire_step_one"),
        "azp_thermostat_step_one": lambda: call(lib.azp_thermostat_step_one, t),
        "azp_fire_measure": fire("azp_fire_measure"),
        "azp_thermostat_kinetic": lambda: call(lib.azp_thermostat_kinetic, t),
        "azp_fire_advance": fire("azp_fire_advance", f_done),  # (the fold of 4 x n_blocks partials; the state is left alone)
        "azp_fire_step_two, converged state": fire("azp_fire_step_two", f_done),
        "azp_fire_step_one, converged state": fire("azp_fire_step_one", f_done),
    }
    bytes_per_particle = {"azp_fire_step_two": 96, "azp_thermostat_step_two": 96, "azp_fire_step_one": 184,
                          "azp_thermostat_step_one": 184, "azp_fire_measure": 64, "azp_thermostat_kinetic": 32}
    pairs = [("azp_fire_step_two", "azp_thermostat_step_two"), ("azp_fire_step_one", "azp_thermostat_step_one")]

    def events(fn):
        # (the forces are random, not those of the positions: the velocities are reset so that nothing runs away)
        vel.copy_(vel0)
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
    res["pairs"] = []
    for mine, theirs in pairs:
        a, b = res["us"][mine], res["us"][theirs]
        spread = b["max"] - b["min"]
        res["pairs"].append(dict(fire=mine, thermostat=theirs, fire_us=a["median"], thermostat_us=b["median"], spread_us=spread,
                                 ratio=a["median"] / b["median"], within=bool(a["median"] <= b["median"] + spread)))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(vel).all()) and bool(torch.isfinite(f_state).all())
    print(json.dumps(res), flush=True)

    lines = ["device: %s, N = %d; device events around %d back-to-back calls after %d warm-up calls, %d repeats in alternating "
             "order, median (min - max)" % (res["device"], N, args.calls, args.warmup, args.repeats), "",
             "| case | us per call | bytes per particle | share of the 8 TB/s HBM peak |", "|---|---|---|---|"]
    for k in cases:
        u = res["us"][k]
        b = bytes_per_particle.get(k, 0)
        share = "%.2f" % (b * N / (u["median"] * 1e-6) / HBM_PEAK) if b else "-"
        lines.append("| %s | %.1f (%.1f - %.1f) | %s | %s |" % (k, u["median"], u["min"], u["max"], b if b else "-", share))
    lines += ["", "Each FIRE pass against its thermostat counterpart; expected: no longer than the counterpart plus the counterpart's "
              "run-to-run spread (max - min over the repeats) in this process.", "",
              "| FIRE pass | us | thermostat pass | us | spread of the thermostat pass (us) | ratio | within the expectation |",
              "|---|---|---|---|---|---|---|"]
    for p in res["pairs"]:
        lines.append("| %s | %.1f | %s | %.1f | %.1f | %.3f | %s |" % (p["fire"], p["fire_us"], p["thermostat"], p["thermostat_us"],
                                                                    p["spread_us"], p["ratio"], "yes" if p["within"] else "NO"))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
