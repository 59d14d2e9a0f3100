"""methods.Langevin measured (profiles/langevin.md).

  kernels:   on the GPU. N = 2^20 particles with rotation: the fused azp_integrate_langevin_step_two_one against the three
             launches that do the same work with the kernels the project had before it (azp_integrate_langevin_flow_step_two_one
             at zero flow, azp_integrate_nve_rot_step_two, azp_integrate_nve_rot_step_one) on the same arrays. The two sides
             alternate; --repeats windows of --launches launches each, timed with device events; the spread is that of the
             windows of one side.
  c5:        on the GPU. The C5 workload of tools/md_bench.py (64 x 64 x 128 TwoPatchMorse colloids, dt 0.004, sorter every 200
             steps) stepped by ConstantVolume (NVE) and by methods.Langevin, both with rotation: ms per step of --steps steps after
             a run-in, host clock around a run that ends in a synchronise, the two alternating --repeats times in one process.
  reference: no GPU. What tests/langevin_ref.py with the oracle's TwoPatchMorse forces gives for the translational and
             rotational temperature of a 6 x 6 x 6 copy of C5 after the steps of tests/test_gpu_langevin.py's full-size run:
             the mean over --seeds independent runs and its standard error (the band of that test).

  python tools/langevin_probe.py kernels|c5|reference
"""

import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def kernels(args):
    import torch

    from azplugins_amd import _lib
    from azplugins_amd import synthetic as syn

    N, L = 2 ** 20, 110.0
    rng = np.random.default_rng(1)
    dev = "cuda:0"

    def rows(x):
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)

    q = rng.normal(size=(N, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    t = dict(pos=rows(syn.pos4(rng.uniform(-0.5 * L, 0.5 * L, (N, 3)), np.zeros(N, dtype=np.int64))),
             vel=rows(np.c_[rng.normal(size=(N, 3)), np.ones(N)]), accel=rows(np.c_[rng.normal(size=(N, 3)), np.zeros(N)]),
             force=rows(rng.normal(size=(N, 4))), image=torch.zeros((N, 3), dtype=torch.int32, device=dev),
             tag=torch.arange(N, dtype=torch.int32, device=dev), q=rows(q), p=rows(rng.normal(size=(N, 4))),
             I=rows(np.tile([0.1, 0.12, 0.14], (N, 1))), torque=rows(np.c_[rng.normal(size=(N, 3)), np.zeros(N)]),
             b=torch.zeros((N, 4), dtype=torch.float64, device=dev), gamma=rows([1.0]), gamma_r=rows([[1.0, 1.0, 1.0]]))
    start = {k: t[k].clone() for k in ("pos", "vel", "accel", "image", "q", "p", "b")}
    lib, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream

    new = _lib.LangevinArgs()
    old, rot = _lib.FlowMethodArgs(), _lib.NVERotArgs()
    for a in (new, old):
        a.d_pos, a.d_vel, a.d_accel, a.d_net_force = (t[k].data_ptr() for k in ("pos", "vel", "accel", "force"))
        a.d_image, a.d_tag, a.d_gamma = (t[k].data_ptr() for k in ("image", "tag", "gamma"))
        a.box = _lib.make_box(L)
        a.dt, a.kT, a.seed, a.N, a.ntypes = 0.004, 1.0, 3, N, 1
    new.d_orientation, new.d_angmom, new.d_inertia = (t[k].data_ptr() for k in ("q", "p", "I"))
    new.d_net_torque, new.d_langevin_torque, new.d_gamma_r = (t[k].data_ptr() for k in ("torque", "b", "gamma_r"))
    new.rotational = 1
    old.flow.kind = _lib.FLOW_CONSTANT
    rot.d_orientation, rot.d_angmom, rot.d_inertia, rot.d_net_torque = (t[k].data_ptr() for k in ("q", "p", "I", "torque"))
    rot.dt, rot.N = 0.004, N

    def fused(step):
        new.timestep = step
        _lib.check(lib.azp_integrate_langevin_step_two_one(C.byref(new), stream), "two_one")

    def three(step):
        old.timestep = step
        _lib.check(lib.azp_integrate_langevin_flow_step_two_one(C.byref(old), stream), "flow two_one")
        _lib.check(lib.azp_integrate_nve_rot_step_two(C.byref(rot), stream), "rot two")
        _lib.check(lib.azp_integrate_nve_rot_step_one(C.byref(rot), stream), "rot one")

    def window(side):
        for k, v in start.items():  # (every window integrates the same states)
            t[k].copy_(v)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for step in range(args.launches):
            side(step)
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / args.launches

    for side in (fused, three):  # code objects, clocks
        window(side)
    times = {fused: [], three: []}
    for _ in range(args.repeats):
        for side in (fused, three):
            times[side].append(window(side))
    # bytes that the fused kernel has to move per particle: pos 32 + 32, vel 32 + 32, accel 32, force 32, image 12 + 12,
    # tag 4, q 32 + 32, p 32 + 32, I 24, torque 32, b 32
    nbytes = 468 * N
    print("N = %d, %d windows of %d launches per side, us per time step (fused: one launch; parent: three)" % (N, args.repeats, args.launches))
    for name, side in (("fused two_one", fused), ("parent, three kernels", three)):
        v = np.sort(times[side])
        line = "%-22s median %.1f  min %.1f  max %.1f  (spread %.1f)" % (name, np.median(v), v[0], v[-1], v[-1] - v[0])
        if side is fused:
            line += "   %.2f TB/s of %d B/particle at the median" % (nbytes / np.median(v) * 1e-6, nbytes // N)
        print(line)
    # the translation is the same arithmetic on both sides, the rotation without friction would be: with friction the
    # results differ, so only what must agree is compared
    for k in ("pos", "vel", "accel", "image"):
        t[k].copy_(start[k])
    fused(0)
    a = {k: t[k].clone() for k in ("pos", "vel", "accel", "image")}
    for k in start:
        t[k].copy_(start[k])
    three(0)
    print("translation of the two sides bit-identical: %s" % all(torch.equal(a[k], t[k]) for k in a))


def c5(args):
    import torch

    import azplugins_amd as azp
    from azplugins_amd import methods
    from azplugins_amd import synthetic as syn

    cfg = syn.config_tpm()
    N = cfg["xyz"].shape[0]

    def make(method):
        snap = azp.Snapshot.from_arrays(cfg["xyz"], cfg["L"], orientation=cfg["orientation"])
        snap.particles.moment_inertia[:] = [0.1, 0.12, 0.14]
        sim = azp.Simulation(device="cuda:0", seed=1)
        sim.create_state_from_snapshot(snap)
        pot = azp.pair.TwoPatchMorse(nlist=azp.nlist.Cell(buffer=cfg["r_buff"]), default_r_cut=cfg["r_cut"], mode="shift")
        pot.params[("A", "A")] = cfg["params"]
        sim.operations.integrator = azp.Integrator(dt=0.004, forces=[pot], methods=[method], integrate_rotational_dof=True)
        sim.operations.tuners[:] = [azp.ParticleSorter(trigger_period=200)]
        sim.run(0)
        sim.thermalize_particle_momenta(1.0, seed=7)
        sim.run(70)  # (md_bench's run-in: melt the lattice a little, load the sorter's kernels)
        torch.cuda.synchronize()
        return sim

    sims = {"NVE (ConstantVolume)": make(azp.ConstantVolume()),
            "methods.Langevin": make(methods.Langevin(azp.All(), kT=1.0, default_gamma=5.0, default_gamma_r=(1.0, 1.0, 1.0)))}
    times = {k: [] for k in sims}
    for _ in range(args.repeats):
        for name, sim in sims.items():
            t0 = time.perf_counter()
            sim.run(args.steps)
            torch.cuda.synchronize()
            times[name].append(1e3 * (time.perf_counter() - t0) / args.steps)
    print("C5, N = %d, dt = 0.004, %d runs of %d steps per method, ms per step" % (N, args.repeats, args.steps))
    for name, v in times.items():
        print("%-22s median %.3f  min %.3f  max %.3f   kT_trans = %.3f" % (name, np.median(v), min(v), max(v), sims[name].kinetic_temperature()))


def reference(args):
    import langevin_ref as ref
    import oracle
    import test_gpu_langevin as T
    from azplugins_amd import synthetic as syn

    cfg = syn.config_tpm(6, 6, 6)
    N, L = cfg["xyz"].shape[0], np.asarray(cfg["L"], dtype=np.float64)
    box = oracle.make_box(cfg["L"])
    params = oracle.pack_pair_params("TwoPatchMorse", cfg["params"])
    tag = np.arange(N, dtype=np.uint32)
    sel = np.ones(N, bool)
    gamma, gamma_r = np.full(N, T.C5_GAMMA), np.tile(T.C5_GAMMA_R, (N, 1))

    def forces(h):
        pos = oracle.pos4(h["pos"])
        nl = oracle.build_nlist(pos, box, cfg["r_cut"])
        f, tq = oracle.aniso_forces_tpm(pos, h["q"], box, nl, params, cfg["r_cut"], "shift")
        return f[:, :3], tq[:, :3]

    out = []
    for seed in range(args.seeds):
        # Simulation.thermalize_particle_momenta restated (unit masses)
        vel = np.stack([syn.normal(1000 + seed, tag.astype(np.uint64), c) for c in range(3)], axis=1) * np.sqrt(T.C5_KT)
        vel -= vel.mean(axis=0)
        h = dict(pos=cfg["xyz"].copy(), vel=vel, mass=np.ones(N), image=np.zeros((N, 3), dtype=np.int32), tag=tag,
                 q=cfg["orientation"].copy(), p=np.zeros((N, 4)), I=np.tile(T.C5_INERTIA, (N, 1)), b=np.zeros((N, 3)))
        f, tq = forces(h)
        h["accel"] = f / h["mass"][:, None]
        for t in range(T.C5_STEPS):
            h = ref.langevin_step_one(h, tq, L, T.C5_DT, sel, True)
            f, tq = forces(h)
            h = ref.langevin_step_two(h, f, tq, gamma, gamma_r, T.C5_KT, T.C5_DT, seed + 1, t, sel, True)
        out.append(T.c5_temperatures(h["vel"], h["mass"], h["q"], h["p"], h["I"]))
        print("seed %d: T_trans = %.4f, T_rot = %.4f" % ((seed,) + out[-1]), flush=True)
    out = np.array(out)
    for k, name in enumerate(("T_trans", "T_rot")):
        print("%s = (%.4f, %.4f)  # mean, standard error of %d runs of N = %d" % (name, out[:, k].mean(),
              out[:, k].std(ddof=1) / np.sqrt(args.seeds), args.seeds, N))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernels", "c5", "reference"])
    ap.add_argument("--launches", type=int, default=200, help="kernels: time steps per window")
    ap.add_argument("--repeats", type=int, default=7, help="kernels: windows per side; c5: timed runs per method")
    ap.add_argument("--steps", type=int, default=200, help="c5: steps per timed run")
    ap.add_argument("--seeds", type=int, default=16, help="reference: independent runs")
    args = ap.parse_args()
    {"kernels": kernels, "c5": c5, "reference": reference}[args.mode](args)


if __name__ == "__main__":
    main()
