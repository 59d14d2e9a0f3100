"""Event-timed cost of compute.PressureProfile beside its two neighbours, all in one process, after a run-in:

  N = 2^20 on the north-star liquid (FCC at rho* = 0.8), PerturbedLJ with r_cut = 3.0, profile along z with 100 and 1000
  bins (and with 1 bin: no spreading loop, every term on the same six words), the rows in the particle sorter's order and
  in a random order; at 1000 bins also with max_term so small that every term is refused (the walk, the evaluator and the
  spreading loop without conversions and atomics). Per case:
    profile, pairs     azp_pressure_profile_begin + azp_pressure_profile_pairs_perturbed_lennard_jones (the cells path)
    profile, whole     PressureProfile._launch: the same plus the kinetic field (keys, sort, sums)
    rdf                azp_rdf_counts at r_max = 3.0, 300 bins: the same walk without an evaluator
    generic pair       azp_pair_forces_perturbed_lennard_jones on the neighbor list of the same state, without a plan and
                       without virials: the same evaluator without spreading

Every figure is the mean over --repeats windows of --calls calls, with the smallest and largest window.

  python tools/pressure_profile_probe.py [--ncell 64] [--calls 10] [--repeats 5] [--out profiles/...md] [--json ...]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncell", type=int, default=64, help="FCC cells per side (64: N = 2^20)")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="write the markdown summary here")
    ap.add_argument("--json", default=None, help="write the raw numbers here")
    args = ap.parse_args()

    import torch

    import azplugins_amd as azp
    from azplugins_amd import _lib, compute
    from azplugins_amd import synthetic as syn

    if not torch.cuda.is_available():
        raise SystemExit("pressure_profile_probe: no GPU (the numbers come from a GPU run only)")

    def windows(fn):
        """ms per call: (mean, min, max) over the windows."""
        for _ in range(args.warmup):
            fn()
        out = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) / args.calls)
        return float(np.mean(out)), float(min(out)), float(max(out))

    cfg = syn.config_north_star(args.ncell)
    n = cfg["xyz"].shape[0]
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(azp.Snapshot.from_arrays(cfg["xyz"], cfg["L"]))
    sim.operations.tuners.clear()
    pot = azp.pair.PerturbedLennardJones(nlist=azp.nlist.Cell(buffer=0.4), default_r_cut=3.0, mode="shift")
    pot.params[("A", "A")] = cfg["params"]
    pot.use_plan = False  # (the generic kernel on the HOOMD-format list)
    sim.operations.integrator = azp.Integrator(dt=0.005, forces=[pot], methods=[azp.ConstantVolume()])
    sim.run(0)
    lib = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream

    res = dict(device=torch.cuda.get_device_name(0), calls=args.calls, repeats=args.repeats, N=int(n), rows=[])
    try:
        res["commit"] = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        res["commit"] = "unknown"

    def add(order, what, t, note=""):
        res["rows"].append(dict(order=order, what=what, ms=t[0], ms_min=t[1], ms_max=t[2], note=note))
        print(json.dumps(res["rows"][-1]), flush=True)

    def reorder(how):
        st = sim.state
        if how == "sorted":
            azp.ParticleSorter(particles_per_block=256).sort(sim)
        else:
            perm = torch.from_numpy(np.random.default_rng(5).permutation(n)).to(st.device)
            for name in ("pos", "vel", "tag", "image"):
                a = getattr(st, name)
                a[:n] = a[:n].index_select(0, perm)
            st.position_generation += 1
            st.order_generation += 1
        sim.run(0)  # (the neighbor list of the new order)

    rows = {}
    for order in ("sorted", "shuffled"):
        reorder(order)
        for nb in (1, 100, 1000):
            prof = compute.PressureProfile("z", nb)
            sim.operations.add(prof)
            row = torch.empty((1, prof._row_width()), dtype=torch.int64, device="cuda:0")
            whole = windows(lambda: prof._launch(row.data_ptr()))
            torch.cuda.synchronize()
            host = row.cpu().numpy()[0, : 6 * nb + 4]
            assert host[-2] == 0, "terms were refused"
            rows.setdefault(nb, []).append(host[:-4].copy())
            # the configurational part alone: the argument struct of _launch, the two calls themselves
            a = _lib.PressureProfileArgs()
            st = sim.state
            a.d_pos, a.d_tag, a.N, a.ntypes, a.box = st.pos.data_ptr(), st.tag.data_ptr(), st.N, 1, st.box.to_c()
            a.axis, a.num_bins, a.lower, a.scale = 2, nb, -0.5 * st.box.Lz, nb / st.box.Lz
            a.max_term, a.wrap, a.shift = prof.max_term, 1, compute.pressure_profile_shift(st.N, prof.max_term)[0]
            a.d_rcutsq, a.d_ronsq = pot._tables["rcutsq"].data_ptr(), pot._tables["ronsq"].data_ptr()
            a.r_max, a.shift_mode, a.path, a.d_out = 3.0, 1, 0, row.data_ptr()
            prof._set_scratch(a, "azp_pressure_profile_scratch_size")
            params = pot._tables["params"].data_ptr()

            def pairs():
                _lib.check(lib.azp_pressure_profile_begin(C.byref(a), stream))
                _lib.check(lib.azp_pressure_profile_pairs_perturbed_lennard_jones(C.byref(a), params, stream))

            t = windows(pairs)
            torch.cuda.synchronize()
            again = row.cpu().numpy()[0, : 6 * nb + 4]
            assert np.array_equal(again, host), "two calls differ"
            add(order, "profile, pairs, %d bins" % nb, t, "%.1f pairs and %.1f terms per particle" % (host[-4] / n, host[-3] / n))
            add(order, "profile, whole, %d bins" % nb, whole)
            if nb == 1000:
                # where the time goes: the same walk and spreading loop with every non-zero term refused (no conversion, no
                # atomic; the refusals are counted in registers)
                a.max_term = 2.0 ** -60
                add(order, "profile, pairs, %d bins, every term refused" % nb, windows(pairs), "the loop without the atomics")
            sim.operations.remove(prof)
        rdf = compute.RadialDistributionFunction(azp.All(), azp.All(), 3.0, 300)
        sim.operations.add(rdf)
        out = torch.empty((1, 304), dtype=torch.int64, device="cuda:0")
        add(order, "rdf, 300 bins", windows(lambda: rdf._launch(out.data_ptr())), "ordered pairs: twice the profile's")
        sim.operations.remove(rdf)
        pa = pot._pair_args()
        pa.compute_virial = 0
        add(order, "generic pair kernel", windows(lambda: _lib.check(getattr(lib, pot._entry)(C.byref(pa), params, stream))),
            "every listed pair from both sides (r_list = 3.4)")
    for nb, pair in rows.items():
        assert np.array_equal(*pair), "the row depends on the order of the rows (%d bins)" % nb

    lines = ["device: %s, commit %s; N = %d; ms per call, mean [min, max] over %d windows of %d calls" % (
        res["device"], res["commit"], n, args.repeats, args.calls), "",
        "| rows | call | ms per call | note |", "|---|---|---|---|"]
    for r in res["rows"]:
        lines.append("| %s | %s | %.3f [%.3f, %.3f] | %s |" % (r["order"], r["what"], r["ms"], r["ms_min"], r["ms_max"], r["note"]))
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
