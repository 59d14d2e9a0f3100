"""What a box resize costs at N = 2^20 in the north-star box (csrc/box_resize.hip), in one process:

  kernels: device events around back-to-back calls of azp_box_resize with every row selected and with a Type mask that
           selects one type of three, next to azp_integrate_nve_step_one on the same arrays, the cases interleaved. The
           box breathes by 0.1 % (M and its inverse alternate), so the positions stay where they were. Traffic by the
           argument structs: the resize kernel 44 B in (pos 32, image 12) and 44 B out per particle; NVE step one 108 B in
           (pos 32, vel 32, force 32, image 12) and 76 B out (pos 32, vel 32, image 12).
  steps:   tools/md_bench.py's run (north-star liquid, PerturbedLJ, NVE, particle sorter every 200 steps), time per MD
           step without an updater and with update.BoxResize every 10 steps and every step -- each resize forces a
           neighbor-list rebuild, which is what this measures. The box breathes by 0.1 % with a period of 400 steps.

  python tools/box_resize_probe.py [--ncell 64] [--calls 200] [--repeats 5] [--steps 300] [--out profiles/...md] [--json ...]
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
BYTES = {"azp_box_resize, All": 88, "azp_box_resize, Type mask (1 of 3 types)": 88, "azp_integrate_nve_step_one": 184}


def kernels(args, cfg):
    import torch

    from azplugins_amd import _lib, update
    from azplugins_amd.state import Box

    N, L = cfg["xyz"].shape[0], float(cfg["L"][0])
    rng = np.random.default_rng(1)
    dev = "cuda:0"
    typeid = rng.integers(0, 3, N).astype(np.int64)
    pos0 = torch.from_numpy(np.c_[cfg["xyz"], typeid.view(np.float64)]).to(dev)
    pos = pos0.clone()
    vel = torch.from_numpy(np.c_[rng.normal(size=(N, 3)), np.ones(N)]).to(dev)
    force = torch.from_numpy(np.c_[rng.normal(0.0, 10.0, (N, 3)), np.zeros(N)]).to(dev)
    image = torch.zeros((N, 3), dtype=torch.int32, device=dev)
    mask = torch.tensor([0, 1, 0], dtype=torch.uint8, device=dev)
    lib, stream = _lib.lib(), _lib.raw_stream(dev)
    boxes = (Box.cube(L), Box.cube(0.999 * L))

    def resize_args(old, new, masked):
        a = _lib.BoxResizeArgs()
        a.d_pos, a.d_image, a.N, a.ntypes = pos.data_ptr(), image.data_ptr(), N, 3
        a.d_type_mask = mask.data_ptr() if masked else None
        a.M[:] = update.box_resize_matrix(old, new)
        a.box = new.to_c()
        return a

    pairs = {m: (resize_args(boxes[0], boxes[1], m), resize_args(boxes[1], boxes[0], m)) for m in (False, True)}
    n = _lib.NVEArgs()
    n.d_pos, n.d_vel, n.d_net_force, n.d_image = pos.data_ptr(), vel.data_ptr(), force.data_ptr(), image.data_ptr()
    n.box, n.dt, n.N = boxes[0].to_c(), 0.0, N  # (dt = 0: the same traffic and arithmetic, nothing moves)
    flip = [0]

    def resize(masked):
        def fn():
            _lib.check(lib.azp_box_resize(C.byref(pairs[masked][flip[0] & 1]), stream))
            flip[0] += 1
        return fn

    cases = {"azp_box_resize, All": resize(False), "azp_box_resize, Type mask (1 of 3 types)": resize(True),
             "azp_integrate_nve_step_one": lambda: _lib.check(lib.azp_integrate_nve_step_one(C.byref(n), stream))}

    def events(fn):
        pos.copy_(pos0)
        image.zero_()
        flip[0] = 0
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
        for k in (list(cases) if r % 2 == 0 else list(cases)[::-1]):
            times[k].append(events(cases[k]))
    assert bool(torch.isfinite(pos).all())
    return {k: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v))) for k, v in times.items()}


def steps(args, cfg, period):
    import torch

    import azplugins_amd as azp
    from azplugins_amd import update, variant

    N = cfg["xyz"].shape[0]
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(azp.Snapshot.from_arrays(cfg["xyz"], cfg["L"]))
    nl = azp.nlist.Cell(buffer=cfg["r_buff"])
    pot = azp.pair.PerturbedLennardJones(nlist=nl, default_r_cut=cfg["r_cut"])
    pot.params[("A", "A")] = cfg["params"]
    sim.operations.integrator = azp.Integrator(dt=0.005, forces=[pot], methods=[azp.ConstantVolume()])
    sim.operations.tuners.clear()
    sim.operations.tuners.append(azp.ParticleSorter(trigger_period=200))
    sim.run(0)
    sim.thermalize_particle_momenta(1.0, seed=7)
    sim.run(50)
    sim.operations.tuners[0].sort(sim)
    sim.run(10)
    _ = nl.size
    sim.run(10)
    if period:
        box0 = sim.state.box
        small = azp.Box(0.999 * box0.Lx, 0.999 * box0.Ly, 0.999 * box0.Lz)
        breathing = variant.box.Interpolate(box0, small, variant.Cycle(0.0, 1.0, sim.timestep, 0, 200, 0, 200))
        sim.operations.add(update.BoxResize(period, breathing))
        sim.run(2 * period)  # (the first resize loads the kernel)
    torch.cuda.synchronize()
    b0, g0 = nl.num_builds, sim.state.box_generation
    t0 = time.perf_counter()
    sim.run(args.steps)
    torch.cuda.synchronize()
    t = time.perf_counter() - t0
    assert bool(torch.isfinite(sim.state.pos[:N]).all())
    return dict(ms_per_step=1e3 * t / args.steps, builds=nl.num_builds - b0, resizes=sim.state.box_generation - g0, steps=args.steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncell", type=int, default=64, help="FCC cells per edge of the north-star box (64: N = 2^20)")
    ap.add_argument("--calls", type=int, default=200, help="timed kernel calls per case and repeat")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=300, help="timed MD steps per resize rate")
    ap.add_argument("--out", default=None, help="write the markdown summary here")
    ap.add_argument("--json", default=None, help="write the raw numbers here")
    args = ap.parse_args()

    import torch

    from azplugins_amd import synthetic as syn

    if not torch.cuda.is_available():
        raise SystemExit("box_resize_probe: no GPU (the numbers come from a GPU run only)")
    cfg = syn.config_north_star(args.ncell)
    N = cfg["xyz"].shape[0]
    res = dict(N=N, device=torch.cuda.get_device_name(0), calls=args.calls, repeats=args.repeats, us=kernels(args, cfg),
               steps={name: steps(args, cfg, period) for name, period in (("no updater", 0), ("BoxResize(Periodic(10))", 10), ("BoxResize(Periodic(1))", 1))})
    print(json.dumps(res), flush=True)
    lines = ["device: %s, N = %d" % (res["device"], N), "",
             "Kernels: device events around %d back-to-back calls after %d warm-up calls, %d repeats in alternating order, median "
             "(min - max)." % (args.calls, args.warmup, args.repeats), "",
             "| kernel | us per call | bytes per particle | achieved TB/s | share of the 8 TB/s HBM peak |", "|---|---|---|---|---|"]
    for k, u in res["us"].items():
        rate = BYTES[k] * N / (u["median"] * 1e-6)
        lines.append("| %s | %.1f (%.1f - %.1f) | %d | %.2f | %.2f |" % (k, u["median"], u["min"], u["max"], BYTES[k], rate / 1e12, rate / HBM_PEAK))
    lines += ["", "MD steps: host clock around run(%d) ending in a device synchronise, after the warm-up of tools/md_bench.py." % args.steps, "",
              "| run | ms per step | resizes | neighbor-list builds |", "|---|---|---|---|"]
    for name, s in res["steps"].items():
        lines.append("| %s | %.3f | %d | %d |" % (name, s["ms_per_step"], s["resizes"], s["builds"]))
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
