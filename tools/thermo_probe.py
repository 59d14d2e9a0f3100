"""Event-timed cost of compute.ThermodynamicQuantities and its recorder on the north-star liquid (PerturbedLJ,
N = 2^20 unless --ncell is given) after a run-in, all in one process:

  (a) one `azp_thermo_sums` call (twenty sums: vel + the pair force's energy column + its six virial rows), its bytes
      and the fraction of the HBM peak;
  (b) the torch path of `Simulation.kinetic_temperature()` (one sum, ends in `.item()`) on the same state;
  (c) what `compute_virial=True` adds to an MD step (the pair kernel's virial pass);
  (d) the MD step time with a recorder at period 1, at period 10, and without one.

  python tools/thermo_probe.py [--steps 400] [--calls 200] [--out profiles/thermo_probe.md] [--json ...]
"""

import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # B/s, MI355X spec
BYTES_PER_PARTICLE = 32 + 32 + 48  # vel row, force row (energy column), six virial streams


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncell", type=int, default=64, help="FCC cells per side (64: N = 2^20)")
    ap.add_argument("--run-in", type=int, default=400)
    ap.add_argument("--steps", type=int, default=400, help="MD steps per timed run")
    ap.add_argument("--calls", type=int, default=200, help="timed calls of (a) and (b)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None, help="write the markdown summary here")
    ap.add_argument("--json", default=None, help="write the raw numbers here")
    args = ap.parse_args()

    import torch

    import azplugins_amd as azp
    from azplugins_amd import compute
    from azplugins_amd import synthetic as syn

    if not torch.cuda.is_available():
        raise SystemExit("thermo_probe: no GPU (the numbers come from a GPU run only)")
    cfg = syn.config_north_star(args.ncell)
    N = cfg["xyz"].shape[0]
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(azp.Snapshot.from_arrays(cfg["xyz"], cfg["L"]))
    sim.thermalize_particle_momenta(1.0)
    nl = azp.nlist.Cell(buffer=cfg["r_buff"])
    plj = azp.pair.PerturbedLennardJones(nlist=nl, default_r_cut=cfg["r_cut"], mode="shift")
    plj.params[("A", "A")] = cfg["params"]
    sim.operations.integrator = azp.Integrator(dt=0.005, forces=[plj], methods=[azp.ConstantVolume()])
    sim.run(args.run_in)

    def events(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)  # ms

    def md_ms_per_step():
        # (two runs: the first absorbs whatever the change before it recompiles)
        sim.run(50)
        return events(lambda: sim.run(args.steps)) / args.steps

    res = dict(N=N, device=torch.cuda.get_device_name(0), steps=args.steps, calls=args.calls)
    try:
        res["commit"] = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        res["commit"] = "unknown"

    # (c) and the baseline of (d)
    res["md_ms_no_virial"] = md_ms_per_step()
    plj.compute_virial = True
    res["md_ms_virial"] = md_ms_per_step()
    thermo = compute.ThermodynamicQuantities(azp.All())
    sim.operations.add(thermo)
    res["md_ms_thermo_attached"] = md_ms_per_step()
    for period in (10, 1):
        rec = compute.ThermodynamicRecorder(thermo, period)
        sim.operations.add(rec)
        res["md_ms_recorder_%d" % period] = md_ms_per_step()
        res["rows_recorder_%d" % period] = int(rec.timesteps.size)
        sim.operations.remove(rec)
    res["virial_us_per_step"] = 1e3 * (res["md_ms_virial"] - res["md_ms_no_virial"])

    # (a) and (b) on the state the runs left
    row = torch.empty((1, 20), dtype=torch.float64, device="cuda:0")

    def ours():
        thermo._launch(row.data_ptr())

    def torch_path():
        return sim.kinetic_temperature()

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        return events(lambda: [fn() for _ in range(args.calls)]) * 1e3 / args.calls  # us

    res["thermo_sums_us"] = timed(ours)
    res["torch_kinetic_temperature_us"] = timed(torch_path)
    res["thermo_sums_us_again"] = timed(ours)  # (both in the same process, either order)
    res["bytes_per_call"] = BYTES_PER_PARTICLE * N
    res["hbm_fraction"] = res["bytes_per_call"] / (res["thermo_sums_us"] * 1e-6) / HBM_PEAK
    res["kT_thermo"] = thermo.kinetic_temperature
    res["kT_torch"] = sim.kinetic_temperature()
    res["pressure"] = thermo.pressure
    first, second = thermo._sums().clone(), thermo._sums().clone()
    res["bit_identical"] = bool(torch.equal(first, second))
    print(json.dumps(res), flush=True)

    lines = [
        "device: %s, commit %s, N = %d; MD figures over %d steps after a run-in, (a) and (b) over %d calls" % (
            res["device"], res["commit"], N, args.steps, args.calls),
        "",
        "| figure | value |", "|---|---|",
        "| (a) `azp_thermo_sums`, one call | %.1f us (%.1f us repeated after (b)); %.1f MB, %.2f of the 8 TB/s HBM peak |" % (
            res["thermo_sums_us"], res["thermo_sums_us_again"], res["bytes_per_call"] / 1e6, res["hbm_fraction"]),
        "| (b) `Simulation.kinetic_temperature()` (torch, one sum) | %.1f us |" % res["torch_kinetic_temperature_us"],
        "| (c) `compute_virial=True`, added to an MD step | %.1f us (%.4f -> %.4f ms per step) |" % (
            res["virial_us_per_step"], res["md_ms_no_virial"], res["md_ms_virial"]),
        "| (d) MD step, compute attached, no recorder | %.4f ms |" % res["md_ms_thermo_attached"],
        "| (d) MD step, recorder at period 10 | %.4f ms (%d rows) |" % (res["md_ms_recorder_10"], res["rows_recorder_10"]),
        "| (d) MD step, recorder at period 1 | %.4f ms (%d rows) |" % (res["md_ms_recorder_1"], res["rows_recorder_1"]),
        "| kT: compute / torch | %.15g / %.15g |" % (res["kT_thermo"], res["kT_torch"]),
        "| two calls bit-identical | %s |" % ("yes" if res["bit_identical"] else "no"),
    ]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    np.testing.assert_allclose(res["kT_thermo"], res["kT_torch"], rtol=1e-12)


if __name__ == "__main__":
    main()
