"""What ConstantPressure costs at N = 2^20 (csrc/barostat.hip), in one process:

  kernels: device events around back-to-back calls through the C ABI on one set of arrays (random positions in a cubic box
           at rho* = 0.8, thermal velocities, random forces, the cases interleaved): azp_barostat_step_one and
           azp_barostat_step_two next to azp_thermostat_step_one and azp_thermostat_step_two, which move the same bytes
           (184 and 96 per particle); azp_thermo_sums with one force and its virial (112 B); azp_barostat_advance; and, on
           the host clock, the advance followed by the readback of the state that the driver does every step.
  steps:   the north-star liquid of tools/md_bench.py (PerturbedLJ, dt 0.005, particle sorter every 200 steps), time per MD
           step under ConstantVolume + MTTK, under NVE with update.BoxResize every step, and under ConstantPressure without
           and with MTTK at S = the liquid's own pressure.

  python tools/barostat_probe.py [--ncell 64] [--calls 200] [--repeats 5] [--steps 200] [--out profiles/...md] [--json ...]
"""

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # B/s, MI355X spec
BYTES = {"azp_barostat_step_one": 184, "azp_thermostat_step_one": 184, "azp_barostat_step_two": 96, "azp_thermostat_step_two": 96,
         "azp_thermo_sums (one force, virial)": 112, "azp_barostat_advance (open)": 0, "azp_barostat_advance (close|open, MTTK)": 0}


def kernels(args, N):
    import torch

    from azplugins_amd import _lib

    L = (N / 0.8) ** (1.0 / 3.0)
    rng = np.random.default_rng(1)
    dev = "cuda:0"
    pos = torch.from_numpy(np.c_[rng.uniform(-0.5 * L, 0.5 * L, (N, 3)), np.zeros(N)]).to(dev)
    vel0 = torch.from_numpy(np.c_[rng.normal(size=(N, 3)), np.ones(N)]).to(dev)
    vel = vel0.clone()
    force = torch.from_numpy(np.c_[rng.normal(0.0, 10.0, (N, 3)), np.zeros(N)]).to(dev)
    virial = torch.from_numpy(rng.normal(size=(6, N))).to(dev)
    image = torch.zeros((N, 3), dtype=torch.int32, device=dev)
    lib, stream = _lib.lib(), _lib.raw_stream(dev)
    need = C.c_uint64(0)
    _lib.check(lib.azp_thermostat_partials_size(N, C.byref(need)))
    partials = torch.zeros(need.value // 8, dtype=torch.float64, device=dev)
    ts_state = torch.zeros(_lib.THERMOSTAT_NSTATE, dtype=torch.float64, device=dev)
    state0 = torch.zeros(_lib.BAROSTAT_NSTATE, dtype=torch.float64, device=dev)
    state0[_lib.BAROSTAT_REF_KT] = 1.0
    state = state0.clone()
    row = torch.zeros(_lib.THERMO_NSUMS, dtype=torch.float64, device=dev)

    t = _lib.ThermostatArgs()
    t.d_pos, t.d_vel, t.d_net_force, t.d_image = pos.data_ptr(), vel.data_ptr(), force.data_ptr(), image.data_ptr()
    t.d_partials, t.partials_bytes, t.d_state = partials.data_ptr(), need.value, ts_state.data_ptr()
    t.box = _lib.make_box(L)
    t.dt, t.kT, t.tau, t.ndof, t.seed, t.N, t.kind = 0.005, 1.0, 0.5, float(3 * N - 3), 1, N, _lib.THERMOSTAT_MTTK
    b = _lib.BarostatArgs()
    b.d_pos, b.d_vel, b.d_net_force, b.d_image = pos.data_ptr(), vel.data_ptr(), force.data_ptr(), image.data_ptr()
    b.d_state, b.d_sums = state.data_ptr(), row.data_ptr()
    b.box = t.box
    b.dt, b.tauS, b.ndof, b.box_dof, b.N, b.couple = 0.005, 1.0, float(3 * N - 3), 7, N, _lib.BAROSTAT_COUPLE["xyz"]
    b.thermostat_kind, b.thermostat_kT, b.thermostat_tau = _lib.THERMOSTAT_MTTK, 1.0, 0.5
    th = _lib.ThermoArgs()
    th.d_vel, th.N, th.n_forces = vel.data_ptr(), N, 1
    th.d_force[0], th.d_virial[0] = force.data_ptr(), virial.data_ptr()
    _lib.check(lib.azp_thermo_scratch_size(C.byref(th), C.byref(need)))
    scratch = torch.empty(int(need.value), dtype=torch.uint8, device=dev)
    th.d_scratch, th.scratch_bytes, th.d_out = scratch.data_ptr(), scratch.numel(), row.data_ptr()

    def call(name, a):
        _lib.check(getattr(lib, name)(C.byref(a), stream))

    def advance(phase, thermostat):
        def fn():
            b.phase = phase
            b.d_thermostat_state = ts_state.data_ptr() if thermostat else None
            call("azp_barostat_advance", b)
        return fn

    cases = {
        "azp_barostat_step_one": lambda: call("azp_barostat_step_one", b),
        "azp_thermostat_step_one": lambda: call("azp_thermostat_step_one", t),
        "azp_barostat_step_two": lambda: call("azp_barostat_step_two", b),
        "azp_thermostat_step_two": lambda: call("azp_thermostat_step_two", t),
        "azp_thermo_sums (one force, virial)": lambda: call("azp_thermo_sums", th),
        "azp_barostat_advance (open)": advance(_lib.BAROSTAT_OPEN, False),
        "azp_barostat_advance (close|open, MTTK)": advance(_lib.BAROSTAT_CLOSE | _lib.BAROSTAT_OPEN, True),
    }

    def reset():
        # (the forces are random, not those of the positions: everything is reset so that nothing runs away. S = 0 and
        # sums of zero leave nu = 0, alpha = lambda = 1 and b = dt in the state; alpha of the thermostat is 1)
        vel.copy_(vel0)
        state.copy_(state0)
        ts_state.zero_()
        row.zero_()
        b.d_thermostat_state = None
        b.phase = _lib.BAROSTAT_OPEN
        call("azp_barostat_advance", b)
        call("azp_thermostat_kinetic", t)
        call("azp_thermostat_advance", t)

    def events(fn):
        reset()
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
    wait = []
    for r in range(args.repeats):
        for k in (list(cases) if r % 2 == 0 else list(cases)[::-1]):
            times[k].append(events(cases[k]))
        # the host's wait of every step: the advance queued on an idle stream, then the state read back
        reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            call("azp_barostat_advance", b)
            state.tolist()
        wait.append((time.perf_counter() - t0) * 1e6 / args.calls)
    assert bool(torch.isfinite(vel).all()) and bool(torch.isfinite(state).all())
    out = {k: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v))) for k, v in times.items()}
    return out, dict(median=float(np.median(wait)), min=float(np.min(wait)), max=float(np.max(wait)))


def steps(args, cfg, kind):
    import torch

    import azplugins_amd as azp
    from azplugins_amd import compute, thermostats, update, variant

    N = cfg["xyz"].shape[0]
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(azp.Snapshot.from_arrays(cfg["xyz"], cfg["L"]))
    nl = azp.nlist.Cell(buffer=cfg["r_buff"])
    pot = azp.pair.PerturbedLennardJones(nlist=nl, default_r_cut=cfg["r_cut"])
    pot.params[("A", "A")] = cfg["params"]
    integ = sim.operations.integrator = azp.Integrator(dt=0.005, forces=[pot], methods=[azp.ConstantVolume()])
    sim.operations.tuners.clear()
    sim.operations.tuners.append(azp.ParticleSorter(trigger_period=200))
    barostat = kind.startswith("ConstantPressure")
    thermo = compute.ThermodynamicQuantities(azp.All())
    if barostat:
        sim.operations.add(thermo)  # (to read the liquid's pressure; the other runs keep their virial pass off)
    sim.run(0)
    sim.thermalize_particle_momenta(1.0, seed=7)
    sim.run(50)
    sim.operations.tuners[0].sort(sim)
    sim.run(10)
    _ = nl.size
    sim.run(10)
    mttk = thermostats.MTTK(kT=1.0, tau=0.5)
    pressure = None
    if barostat:
        pressure = thermo.pressure
        sim.operations.remove(thermo)
        integ.methods[0] = azp.ConstantPressure(azp.All(), S=pressure, tauS=1.0, couple="xyz", thermostat=mttk if "MTTK" in kind else None)
    elif "MTTK" in kind:
        integ.methods[0] = azp.ConstantVolume(thermostat=mttk)
    elif "BoxResize" in kind:
        box0 = sim.state.box
        small = azp.Box(0.999 * box0.Lx, 0.999 * box0.Ly, 0.999 * box0.Lz)
        sim.operations.add(update.BoxResize(1, variant.box.Interpolate(box0, small, variant.Cycle(0.0, 1.0, sim.timestep, 0, 200, 0, 200))))
    sim.run(10)  # (the first step loads the kernels)
    torch.cuda.synchronize()
    b0, g0, V0 = nl.num_builds, sim.state.box_generation, sim.state.box.volume
    t0 = time.perf_counter()
    sim.run(args.steps)
    torch.cuda.synchronize()
    t = time.perf_counter() - t0
    assert bool(torch.isfinite(sim.state.pos[:N]).all())
    return dict(ms_per_step=1e3 * t / args.steps, builds=nl.num_builds - b0, box_changes=sim.state.box_generation - g0, steps=args.steps,
                S=pressure, volume_ratio=sim.state.box.volume / V0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncell", type=int, default=64, help="FCC cells per edge of the north-star box (64: N = 2^20)")
    ap.add_argument("--calls", type=int, default=200, help="timed kernel calls per case and repeat")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=200, help="timed MD steps per run")
    ap.add_argument("--out", default=None, help="write the markdown summary here")
    ap.add_argument("--json", default=None, help="write the raw numbers here")
    args = ap.parse_args()

    import torch

    from azplugins_amd import synthetic as syn

    if not torch.cuda.is_available():
        raise SystemExit("barostat_probe: no GPU (the numbers come from a GPU run only)")
    cfg = syn.config_north_star(args.ncell)
    N = cfg["xyz"].shape[0]
    us, wait = kernels(args, N)
    runs = ("ConstantVolume + MTTK", "ConstantVolume (NVE) + BoxResize(Periodic(1))", "ConstantPressure (NPH)", "ConstantPressure + MTTK")
    res = dict(N=N, device=torch.cuda.get_device_name(0), calls=args.calls, repeats=args.repeats, us=us, host_wait_us=wait,
               steps={name: steps(args, cfg, name) for name in runs})
    print(json.dumps(res), flush=True)
    lines = ["device: %s, N = %d" % (res["device"], N), "",
             "Kernels: device events around %d back-to-back calls after %d warm-up calls, %d repeats in alternating order, median "
             "(min - max)." % (args.calls, args.warmup, args.repeats), "",
             "| kernel | us per call | bytes per particle | share of the 8 TB/s HBM peak |", "|---|---|---|---|"]
    for k, u in res["us"].items():
        share = "%.2f" % (BYTES[k] * N / (u["median"] * 1e-6) / HBM_PEAK) if BYTES[k] else "-"
        lines.append("| %s | %.1f (%.1f - %.1f) | %s | %s |" % (k, u["median"], u["min"], u["max"], BYTES[k] or "-", share))
    for one in ("one", "two"):
        lines.append("| ratio azp_barostat_step_%s / azp_thermostat_step_%s | %.3f | | |"
                     % (one, one, res["us"]["azp_barostat_step_" + one]["median"] / res["us"]["azp_thermostat_step_" + one]["median"]))
    lines += ["", "Host wait: host clock around %d times (azp_barostat_advance on an idle stream, then the %d doubles of the state "
              "read back): %.1f us each (%.1f - %.1f)." % (args.calls, 24, wait["median"], wait["min"], wait["max"]), "",
              "MD steps: host clock around run(%d) ending in a device synchronise, after the warm-up of tools/md_bench.py." % args.steps, "",
              "| run | ms per step | box changes | neighbor-list builds | S | V / V0 at the end |", "|---|---|---|---|---|---|"]
    for name, s in res["steps"].items():
        lines.append("| %s | %.3f | %d | %d | %s | %.5f |" % (name, s["ms_per_step"], s["box_changes"], s["builds"],
                                                             "%.4f" % s["S"] if s["S"] is not None else "-", s["volume_ratio"]))
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
