"""Event-timed cost of azp_structure_factor_amplitudes (compute.StructureFactor), all in one process, after a warm-up:

  the north-star liquid (FCC at rho* = 0.8) at N = 2^20 with about 10^3 wavevectors, with the dense sets |m| <= 15 and
  |m| <= 30 (the largest at which the powers path exists in a cube) and with the largest thinned set under the cap (the
  bounding block at its 2^24 triples, 256 per |q| bin); N = 2^17 with about 10^3 wavevectors. Both paths wherever both
  exist, A = B = All.

For scale, next to each:
  (a) the formulation a user could write with torch on the device: pos @ q.T, cos and sin, column sums, in float64, in
      chunks of particles of at most --torch-bytes of phases;
  (b) one PerturbedLJ force launch on the same system;
  (c) the FP64-rate VALU issue bound of the inner loop: VALU instructions per (staged particle, wave of 64 vectors) of
      this commit's ISA (INNER_VALU below, counted from hipcc --save-temps) x 4 cycles per wave64 instruction, over
      1,024 SIMDs at 2.4 GHz.

Every figure is the median over --repeats windows of --calls calls, with the smallest and largest window.

  python tools/structure_factor_probe.py [--ncell 64] [--calls 5] [--repeats 5] [--out profiles/structure_factor_probe.md] [--json ...]
"""

import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# VALU instructions of one trip of the inner loop (one staged particle, one wave), same_groups kernels:
# direct: 32 FP64 (15 v_fmac, 5 v_mul, 5 v_add, 1 v_fma, v_rndne, v_fract, v_cvt, 3 v_cmp) + 12 v_cndmask + 11 v_mov_b64
#         + 9 integer / bit operations, and two LDS reads; powers: 10 FP64 (4 v_mul, 4 v_fmac, 2 v_add) + 3 v_xor +
#         3 v_add_u32 + 1 v_cmp, and three ds_read_b128.
INNER_VALU = {1: 64, 2: 17}
SIMDS, CLOCK_HZ, CYCLES_PER_VALU = 1024, 2.4e9, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncell", type=int, default=64, help="FCC cells per side of the large system (64: N = 2^20)")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--torch-bytes", type=float, default=2.0e9)
    ap.add_argument("--out", default=None, help="write the markdown summary here")
    ap.add_argument("--json", default=None, help="write the raw numbers here")
    args = ap.parse_args()

    import torch

    import azplugins_amd as azp
    from azplugins_amd import _lib, compute
    from azplugins_amd import synthetic as syn

    if not torch.cuda.is_available():
        raise SystemExit("structure_factor_probe: no GPU (the numbers come from a GPU run only)")

    def windows(fn, calls=None, repeats=None):
        """ms per call: (median, min, max) over the windows (a heavy case names fewer calls and warms up once)."""
        warmup = args.warmup if calls is None else 1
        calls, repeats = calls or args.calls, repeats or args.repeats
        for _ in range(warmup):
            fn()
        out = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) / calls)
        return float(np.median(out)), float(min(out)), float(max(out))

    res = dict(device=torch.cuda.get_device_name(0), calls=args.calls, repeats=args.repeats, rows=[])
    try:
        res["commit"] = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        res["commit"] = "unknown"

    def add(case, n, nv, what, t, note=""):
        res["rows"].append(dict(case=case, N=int(n), n_vectors=int(nv), what=what, ms=t[0], ms_min=t[1], ms_max=t[2], note=note))
        print(json.dumps(res["rows"][-1]), flush=True)

    def sf_time(sim, q_max, num_bins, per_bin, path, heavy):
        sf = compute.StructureFactor(azp.All(), azp.All(), q_max, num_bins, max_vectors_per_bin=per_bin)
        sf.path = path
        sim.operations.add(sf)
        row = torch.empty((1, sf._row_width()), dtype=torch.float64, device="cuda:0")
        t = windows(lambda: sf._launch(row.data_ptr()), *((2, 3) if heavy else (None, None)))
        host = row.cpu().numpy()[0]
        m = sf.vectors
        sim.operations.remove(sf)
        return t, host, m

    def torch_time(sim, m, heavy):
        st = sim.state
        q = torch.from_numpy(compute.reciprocal_vectors(st.box, m)).to(st.device)
        x = st.pos[: st.N, :3]
        rows = max(1, min(st.N, int(args.torch_bytes / (8.0 * len(m)))))

        def run():
            re = torch.zeros(len(m), dtype=torch.float64, device=st.device)
            im = torch.zeros(len(m), dtype=torch.float64, device=st.device)
            for c0 in range(0, st.N, rows):
                phase = x[c0:c0 + rows] @ q.T
                re.add_(torch.cos(phase).sum(dim=0))
                im.sub_(torch.sin(phase).sum(dim=0))
            return re, im

        t = windows(run, *((1, 2) if heavy else (None, None)))
        re, im = run()
        return t, re.cpu().numpy(), im.cpu().numpy()

    def force_time(cfg):
        sim = azp.Simulation(device="cuda:0", seed=1)
        sim.create_state_from_snapshot(azp.Snapshot.from_arrays(cfg["xyz"], cfg["L"]))
        plj = azp.pair.PerturbedLennardJones(nlist=azp.nlist.Cell(buffer=cfg["r_buff"]), default_r_cut=cfg["r_cut"], mode="shift")
        plj.params[("A", "A")] = cfg["params"]
        sim.operations.integrator = azp.Integrator(dt=0.005, forces=[plj], methods=[azp.ConstantVolume()])
        sim.operations.tuners.clear()
        sim.run(0)
        return windows(lambda: plj.compute(sim.timestep))

    def bound_ms(n, nv, path):
        return n * -(-nv // 64) * INNER_VALU[path] * CYCLES_PER_VALU / (SIMDS * CLOCK_HZ) * 1e3

    def case(name, cfg, radius, num_bins, per_bin, heavy=False):
        n = cfg["xyz"].shape[0]
        sim = azp.Simulation(device="cuda:0", seed=1)
        sim.create_state_from_snapshot(azp.Snapshot.from_arrays(cfg["xyz"], cfg["L"]))
        q_max = 2.0 * np.pi * radius / float(cfg["L"][0])
        rows = {}
        for path, label in ((_lib.SF_PATH_DIRECT, "direct"), (_lib.SF_PATH_POWERS, "powers")):
            try:
                t, rows[path], m = sf_time(sim, q_max, num_bins, per_bin, path, heavy)
            except _lib.AzpError:
                add(name, n, 0, "azp_structure_factor_amplitudes (%s)" % label, (float("nan"),) * 3, "refused: the tables do not fit the LDS budget")
                continue
            if not heavy:
                again = sf_time(sim, q_max, num_bins, per_bin, path, heavy)[1]
                assert np.array_equal(rows[path].view(np.int64), again.view(np.int64)), "two calls differ"
            b = bound_ms(n, len(m), path)
            add(name, n, len(m), "azp_structure_factor_amplitudes (%s)" % label, t,
                "VALU issue bound %.3f ms (%.0f %% of it reached); indices up to %d" % (b, 100.0 * b / t[0], np.abs(m).max()))
        if len(rows) == 2:
            d = np.abs(rows[1] - rows[2]).max()
            res["rows"][-1]["note"] += "; paths differ by at most %.2g" % d
        t, re, im = torch_time(sim, m, heavy)
        nv = len(m)
        d = max(np.abs(re - rows[1][:nv]).max(), np.abs(im - rows[1][nv:2 * nv]).max())
        add(name, n, nv, "torch: pos @ q.T, cos, sin, sums", t, "differs from the direct path by at most %.2g" % d)
        return sim

    big = syn.config_north_star(args.ncell)
    n_big = big["xyz"].shape[0]
    case("north star, ~10^3 vectors", big, 7.8, 64, None)
    case("north star, dense, indices up to 15", big, 15.5, 64, None)
    case("north star, dense, indices up to 30", big, 30.5, 64, None, heavy=True)
    # the bounding block at 2^24 triples (|m_k| <= 127), 256 bins of at most 256 vectors
    case("north star, thinned under the cap", big, 127.5 * args.ncell / 64.0, 256, 256, heavy=True)
    add("north star", n_big, 0, "one PerturbedLJ force launch", force_time(big))
    small = syn.config_north_star(args.ncell // 2)
    case("N / 8, ~10^3 vectors", small, 7.8, 64, None)
    add("N / 8", small["xyz"].shape[0], 0, "one PerturbedLJ force launch", force_time(small))

    lines = ["device: %s, commit %s; ms per call, median [min, max] over %d windows of %d calls (the thinned case and indices up to 30: 3 windows of 2, "
             "torch 2 of 1)" % (res["device"], res["commit"], args.repeats, args.calls), "",
             "| case | N | vectors | call | ms per call | note |", "|---|---|---|---|---|---|"]
    for r in res["rows"]:
        lines.append("| %s | %d | %d | `%s` | %.3f [%.3f, %.3f] | %s |" % (r["case"], r["N"], r["n_vectors"], r["what"], r["ms"], r["ms_min"], r["ms_max"], r["note"]))
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
