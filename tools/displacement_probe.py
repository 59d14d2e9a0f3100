"""Event-timed cost of the displacement kernels (compute.MeanSquaredDisplacement, compute.SelfIntermediateScattering;
csrc/displacement.hip), all in one process, after a warm-up, on the north-star liquid at N = 2^20: the FCC lattice at
rho* = 0.8 with kT = 1 velocities, run --melt NVE steps with the default particle sorter; the origin is taken half way
through the run-in. The header line says what share of the rows is still at its tag: the sorter's period is 200 steps,
so with the default --melt 100 the rows are still in tag order and the gathers through the reverse-tag table are
coalesced; --melt 250 measures real gathers.

  (a) azp_displacement_moments, one origin, without and with 200 bins, against the azp_thermo_sums pass of a
      ThermodynamicQuantities(All()) on the same state (both stream the particles once), with the bytes per particle the
      kernel asks for and the bandwidth that makes of its time;
  (b) the same at K = 8 and 32 origins in one launch (the origins are a grid dimension) against K launches of one (a
      build with another layout of the origins is measured by running parts "ab" with AZP_LIB_PATH and --label);
  (c) azp_self_scattering against StructureFactor forced to the direct path on the same vector set (about 2,000
      vectors), K = 1 and 8;
  (d) one MD step with and without the two recorders firing every 10 steps (ring of 8 origins, a new one every 4th firing).

Every figure is the median over --repeats windows of --calls calls, with the smallest and largest window; both sides of
a ratio come from this one process.

  python tools/displacement_probe.py [--ncell 64] [--melt 100] [--calls 5] [--repeats 5] [--commit HASH] [--out FILE.md] [--json FILE]
"""

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# bytes per particle and origin that dm_partial requests: origin position row 32 + origin image 12 + rtag 4, and through
# rtag: pos 32 + image 12 + tag 4
DM_BYTES = 96


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncell", type=int, default=64, help="FCC cells per side (64: N = 2^20)")
    ap.add_argument("--melt", type=int, default=100)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--md-steps", type=int, default=200)
    ap.add_argument("--commit", default=None, help="the commit the numbers belong to (default: git rev-parse)")
    ap.add_argument("--parts", default="abcd", help="which of the parts (a) to (d) to run")
    ap.add_argument("--label", default="", help="a word for the header line (a kernel variant loaded through AZP_LIB_PATH)")
    ap.add_argument("--out", default=None, help="write the markdown summary here")
    ap.add_argument("--json", default=None, help="write the raw numbers here")
    args = ap.parse_args()

    import torch

    import azplugins_amd as azp
    from azplugins_amd import _lib, compute
    from azplugins_amd import synthetic as syn

    if not torch.cuda.is_available():
        raise SystemExit("displacement_probe: no GPU (the numbers come from a GPU run only)")

    def windows(fn, calls=None):
        calls = calls or args.calls
        for _ in range(args.warmup):
            fn()
        out = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) / calls)
        return float(np.median(out)), float(min(out)), float(max(out))

    res = dict(device=torch.cuda.get_device_name(0), calls=args.calls, repeats=args.repeats, melt=args.melt, rows=[])
    res["commit"] = args.commit
    if res["commit"] is None:
        try:
            res["commit"] = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            res["commit"] = "unknown"

    def add(part, what, t, note=""):
        res["rows"].append(dict(part=part, what=what, ms=t[0], ms_min=t[1], ms_max=t[2], note=note))
        print(json.dumps(res["rows"][-1]), flush=True)

    cfg = syn.config_north_star(args.ncell)
    n = cfg["xyz"].shape[0]
    res["N"] = int(n)

    def liquid():
        sim = azp.Simulation(device="cuda:0", seed=1)
        sim.create_state_from_snapshot(azp.Snapshot.from_arrays(cfg["xyz"], cfg["L"]))
        plj = azp.pair.PerturbedLennardJones(nlist=azp.nlist.Cell(buffer=cfg["r_buff"]), default_r_cut=cfg["r_cut"], mode="shift")
        plj.params[("A", "A")] = cfg["params"]
        sim.operations.integrator = azp.Integrator(dt=0.005, forces=[plj], methods=[azp.ConstantVolume()])
        sim.run(0)
        sim.thermalize_particle_momenta(1.0, seed=7)
        return sim

    sim = liquid()
    st = sim.state
    msd = compute.MeanSquaredDisplacement(azp.All())
    vh = compute.MeanSquaredDisplacement(azp.All(), num_bins=200, r_max=2.0)
    thermo = compute.ThermodynamicQuantities(azp.All())
    q_max = 2.0 * np.pi * 9.9 / float(cfg["L"][0])
    fs = compute.SelfIntermediateScattering(azp.All(), q_max, 64)
    sf = compute.StructureFactor(azp.All(), azp.All(), q_max, 64)
    sf.path = _lib.SF_PATH_DIRECT
    for c in (msd, vh, thermo, fs, sf):
        sim.operations.add(c)
    sim.run(args.melt // 2)
    # a store of 32 origins, filled as the run-in goes on (the last 31 during its second half)
    stores = {c: c._store(st, 32) for c in (msd, fs)}
    for c in (msd, vh, fs):
        c.set_origin()
    for slot in range(32):
        for c, (p0, i0) in stores.items():
            c._scatter(st, p0, i0, slot)
        sim.run(max(1, (args.melt - args.melt // 2) // 32))
    torch.cuda.synchronize()
    tags = st.tag[:n].cpu().numpy()
    res["rows_in_tag_order"] = float((tags == np.arange(n)).mean())
    res["msd"] = msd.msd

    row = {c: torch.empty((32, c._row_width()), dtype=torch.float64, device=st.device) for c in (msd, vh, thermo, fs, sf)}
    if "a" in args.parts:
        # (a) one origin against the thermo pass
        t_thermo = windows(lambda: thermo._launch(row[thermo].data_ptr()))
        add("a", "azp_thermo_sums (All, one pair force with virial)", t_thermo, "112 B per particle requested")
        for c, label in ((msd, "no histogram"), (vh, "200 bins")):
            t = windows(lambda: c._launch(row[c].data_ptr()))
            add("a", "azp_displacement_moments, K = 1, %s" % label, t,
                "%.2f of the thermo pass; %d B per particle requested: %.0f GB/s" % (t[0] / t_thermo[0], DM_BYTES, DM_BYTES * n / t[0] * 1e-6))
        first, second = (msd._read("row").copy() for _ in range(2))
        assert np.array_equal(first, second), "two calls differ"

    if "b" in args.parts:
        # (b) K origins in one launch against K launches of one
        p0, i0 = stores[msd]
        for k in (8, 32):
            t_one = windows(lambda: msd._launch_slots(row[msd].data_ptr(), st, p0, i0, k, (1 << k) - 1))

            def each():
                for s in range(k):
                    msd._launch_slots(row[msd].data_ptr() + s * msd._row_width() * 8, st, p0[s:s + 1], i0[s:s + 1], 1, 1)

            t_each = windows(each, calls=max(1, args.calls // 2))
            add("b", "azp_displacement_moments, K = %d in one launch" % k, t_one,
                "%.3f ms per origin; %d launches of one: %.3f ms (%.2f times)" % (t_one[0] / k, k, t_each[0], t_each[0] / t_one[0]))

    if "c" in args.parts:
        # (c) self scattering against the static direct path
        n_vec = len(fs.vectors)
        assert np.array_equal(fs.vectors, sf.vectors)
        t_sf = windows(lambda: sf._launch(row[sf].data_ptr()))
        add("c", "azp_structure_factor_amplitudes, direct path, %d vectors" % n_vec, t_sf)
        p0, i0 = stores[fs]
        for k in (1, 8):
            t = windows(lambda: fs._launch_slots(row[fs].data_ptr(), st, p0, i0, k, (1 << k) - 1), calls=max(1, args.calls // (2 if k > 1 else 1)))
            add("c", "azp_self_scattering, %d vectors, K = %d" % (n_vec, k), t, "%.2f of the static direct path per origin" % (t[0] / k / t_sf[0]))

    if "d" in args.parts:
        # (d) the MD step with and without the recorders
        def step_ms(with_recorders):
            s = liquid()
            s.run(args.melt)
            if with_recorders:
                m2, f2 = compute.MeanSquaredDisplacement(azp.All(), num_bins=200, r_max=2.0), compute.SelfIntermediateScattering(azp.All(), q_max, 64)
                for op in (m2, f2, compute.MeanSquaredDisplacementRecorder(m2, 10, origins=8, origin_every=4),
                           compute.SelfIntermediateScatteringRecorder(f2, 10, origins=8, origin_every=4)):
                    s.operations.add(op)
            s.run(20)
            out = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                s.run(args.md_steps)
                torch.cuda.synchronize()
                out.append((time.perf_counter() - t0) / args.md_steps * 1e3)
            return float(np.median(out)), float(min(out)), float(max(out))

        t_plain = step_ms(False)
        t_rec = step_ms(True)
        add("d", "MD step, no recorder (%d steps, wall clock)" % args.md_steps, t_plain)
        add("d", "MD step, both recorders every 10 steps, ring of 8", t_rec,
            "%.3f times the plain step; %.3f ms per firing" % (t_rec[0] / t_plain[0], 10.0 * (t_rec[0] - t_plain[0])))

    lines = [("%s; " % args.label if args.label else "") + "device: %s, commit %s; N = %d after %d NVE steps (%.1f %% of the rows still at their tag; msd %.3g); ms per call, median "
             "[min, max] over %d windows of %d calls" % (res["device"], res["commit"], n, args.melt, 100.0 * res["rows_in_tag_order"], res["msd"],
                                                        args.repeats, args.calls), "",
             "| part | call | ms per call | note |", "|---|---|---|---|"]
    for r in res["rows"]:
        lines.append("| %s | `%s` | %.3f [%.3f, %.3f] | %s |" % (r["part"], r["what"], r["ms"], r["ms_min"], r["ms_max"], r["note"]))
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
