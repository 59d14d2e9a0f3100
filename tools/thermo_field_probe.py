"""Event-timed cost of compute.ThermodynamicField's kernels at N = 2^20 (north-star FCC lattice,
azplugins_amd.synthetic; one force array with a virial), with the particles in lattice (sorted) order and shuffled:
one bin, a 100-bin z profile, a 100 x 100 Cartesian field and a 50 x 8 x 20 cylindrical field. Per case the
microseconds of the key kernel, of torch.sort, of the segment heads and of the segmented sum (the tree), each timed on
its own (device events around `--calls` back-to-back calls after a warm-up), beside
  - azp_velocity_field_sums + normalize on the same field (csrc/velocity_field.hip, which this work does not change),
  - azp_thermo_sums (ThermodynamicQuantities: the whole box, same force array) for the one-bin case,
  - one pass over the bytes the tree's first level reads (order 8 + segment 4 + vel 32 + pos 32 + force 32 + virial 48 =
    156 B per particle) at the 8 TB/s HBM peak bench.py uses.

  python tools/thermo_field_probe.py [--calls 30] [--out profiles/thermo_field_table.md] [--json FILE]
"""

import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # B/s, MI355X spec (bench.py)
LEVEL1_BYTES = 8 + 4 + 32 + 32 + 32 + 48


def _cases(L):
    return [
        ("one bin", "cartesian", (0, 0, 0), (0, 0, 0), (0, 0, 0)),
        ("z profile 100", "cartesian", (0, 0, 100), (0, 0, -L[2] / 2), (0, 0, L[2] / 2)),
        ("Cartesian 100x100", "cartesian", (100, 100, 0), (-L[0] / 2, -L[1] / 2, 0), (L[0] / 2, L[1] / 2, 0)),
        ("Cylindrical 50x8x20", "cylindrical", (50, 8, 20), (0, 0, -L[2] / 2), (L[0] / 2, 2 * math.pi, L[2] / 2)),
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ncell", type=int, default=64, help="FCC cells per edge (64: N = 2^20)")
    ap.add_argument("--out", default=None, help="write the markdown table here")
    ap.add_argument("--json", default=None, help="write the raw numbers here")
    args = ap.parse_args()

    import torch

    import azplugins_amd as azp
    from azplugins_amd import _lib
    from azplugins_amd import synthetic as syn

    if not torch.cuda.is_available():
        raise SystemExit("thermo_field_probe: no GPU (the numbers come from a GPU run only)")
    dev = torch.device("cuda:0")
    cfg = syn.config_north_star(ncell=args.ncell)
    N = cfg["xyz"].shape[0]
    L = [float(v) for v in cfg["L"]]
    tag = np.arange(N, dtype=np.uint64)
    vel = np.stack([syn.normal(21, tag, c) for c in range(3)] + [1.0 + syn.u01(22, tag, 0)], axis=1)
    pos = syn.pos4(cfg["xyz"])
    rng = np.random.default_rng(0)
    orders = {"sorted": np.arange(N), "shuffled": rng.permutation(N)}
    lib = _lib.lib()
    stream = _lib.raw_stream(dev)
    box = azp.Box(*L).to_c()
    force = torch.from_numpy(rng.normal(size=(N, 4))).to(dev)
    virial = torch.from_numpy(rng.normal(size=(6, N))).to(dev)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.calls

    rows = []
    for order_name, order in orders.items():
        d_pos = torch.from_numpy(np.ascontiguousarray(pos[order])).to(dev)
        d_vel = torch.from_numpy(np.ascontiguousarray(vel[order])).to(dev)
        d_tag = torch.from_numpy(order.astype(np.int32)).to(dev)
        # ThermodynamicQuantities on the same arrays (the whole box)
        t = _lib.ThermoArgs()
        t.d_vel, t.N, t.n_forces = d_vel.data_ptr(), N, 1
        t.d_force[0], t.d_virial[0] = force.data_ptr(), virial.data_ptr()
        need = C.c_uint64(0)
        _lib.check(lib.azp_thermo_scratch_size(C.byref(t), C.byref(need)))
        t_scratch = torch.empty(max(int(need.value), 8), dtype=torch.uint8, device=dev)
        t_out = torch.empty(_lib.THERMO_NSUMS, dtype=torch.float64, device=dev)
        t.d_scratch, t.scratch_bytes, t.d_out = t_scratch.data_ptr(), t_scratch.numel(), t_out.data_ptr()
        thermo_us = timed(lambda: _lib.check(lib.azp_thermo_sums(C.byref(t), stream)))
        for name, coords, nb, lo, hi in _cases(L):
            n_bins = int(np.prod([k for k in nb if k > 0])) if any(nb) else 1
            code = _lib.COORDINATES_CYLINDRICAL if coords == "cylindrical" else _lib.COORDINATES_CARTESIAN
            a = _lib.ThermoFieldArgs()
            a.d_pos, a.d_vel, a.d_tag, a.N = d_pos.data_ptr(), d_vel.data_ptr(), d_tag.data_ptr(), N
            a.coordinates, a.box, a.ntypes, a.n_forces = code, box, 1, 1
            a.d_force[0], a.d_virial[0] = force.data_ptr(), virial.data_ptr()
            v = _lib.VelocityFieldArgs()
            v.d_pos, v.d_vel, v.N, v.coordinates, v.box = d_pos.data_ptr(), d_vel.data_ptr(), N, code, box
            for d in range(3):
                a.num_bins[d], a.lower[d], a.upper[d] = nb[d], lo[d], hi[d]
                v.num_bins[d], v.lower[d], v.upper[d] = nb[d], lo[d], hi[d]
            _lib.check(lib.azp_thermo_field_scratch_size(C.byref(a), C.byref(need)))
            scratch_bytes = int(need.value)
            scratch = torch.empty(max(scratch_bytes, 8), dtype=torch.uint8, device=dev)
            keys = torch.empty(N, dtype=torch.int64, device=dev)
            out = torch.empty((n_bins, _lib.THERMO_FIELD_NSUMS + 1), dtype=torch.float64, device=dev)
            a.d_keys, a.d_out, a.d_scratch, a.scratch_bytes = keys.data_ptr(), out.data_ptr(), scratch.data_ptr(), scratch.numel()
            _lib.check(lib.azp_thermo_field_keys(C.byref(a), stream))
            skeys, perm = torch.sort(keys)
            a.d_sorted_keys, a.d_order = skeys.data_ptr(), perm.data_ptr()

            def phase(code):
                def fn():
                    a.phases = code
                    _lib.check(lib.azp_thermo_field_sums(C.byref(a), stream))
                return fn

            keys_us = timed(lambda: _lib.check(lib.azp_thermo_field_keys(C.byref(a), stream)))
            sort_us = timed(lambda: torch.sort(keys))
            heads_us = timed(phase(_lib.THERMO_FIELD_HEADS))
            tree_us = timed(phase(_lib.THERMO_FIELD_LEVELS))
            all_us = timed(phase(0))
            phase(0)()
            r1 = out.clone()
            phase(0)()
            identical = bool(torch.equal(r1, out))
            counted = float(out[:, 0].sum().item())
            # the velocity field on the same bins
            _lib.check(lib.azp_velocity_field_scratch_size(C.byref(v), C.byref(need)))
            v_scratch = torch.empty(max(int(need.value), 8), dtype=torch.uint8, device=dev)
            v_sums = torch.empty((n_bins, 4), dtype=torch.float64, device=dev)
            v_out = torch.empty((n_bins, 3), dtype=torch.float64, device=dev)
            v.d_sums, v.d_scratch, v.scratch_bytes = v_sums.data_ptr(), v_scratch.data_ptr(), v_scratch.numel()

            def velocity_field():
                _lib.check(lib.azp_velocity_field_sums(C.byref(v), stream))
                _lib.check(lib.azp_velocity_field_normalize(v_sums.data_ptr(), n_bins, v_out.data_ptr(), stream))

            vf_us = timed(velocity_field)
            mass_diff = float((v_sums[:, 0] - out[:, 1]).abs().max().item())
            bound_us = LEVEL1_BYTES * N / HBM_PEAK * 1e6
            total = keys_us + sort_us + all_us
            rows.append(dict(case=name, order=order_name, bins=n_bins, counted=counted, scratch_bytes=scratch_bytes, keys_us=keys_us,
                             sort_us=sort_us, heads_us=heads_us, tree_us=tree_us, heads_and_tree_us=all_us, total_us=total,
                             velocity_field_us=vf_us, velocity_field_tiles=(n_bins + 511) // 512,
                             thermo_us=thermo_us if n_bins == 1 else None, bound_us=bound_us, tree_fraction_of_bound=bound_us / tree_us,
                             total_over_velocity_field=total / vf_us, bit_identical=identical, max_mass_diff_vs_velocity_field=mass_diff))
            print(json.dumps(rows[-1]), flush=True)
    dev_name = torch.cuda.get_device_name(0)
    head = "device: %s, N = %d, %d calls after %d warm-up calls" % (dev_name, N, args.calls, args.warmup)
    lines = ["| case | order | bins | keys us | sort us | heads us | tree us | total us | tree: fraction of the %d B/particle bound (%.1f us) | "
             "velocity field us (tiles) | total / velocity field | thermo us | bit-identical |" % (LEVEL1_BYTES, rows[0]["bound_us"]),
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %s | %s | %d | %.1f | %.1f | %.1f | %.1f | %.1f | %.2f | %.1f (%d) | %.2f | %s | %s |" % (
            r["case"], r["order"], r["bins"], r["keys_us"], r["sort_us"], r["heads_us"], r["tree_us"], r["total_us"],
            r["tree_fraction_of_bound"], r["velocity_field_us"], r["velocity_field_tiles"], r["total_over_velocity_field"],
            "%.1f" % r["thermo_us"] if r["thermo_us"] is not None else "-", "yes" if r["bit_identical"] else "no"))
    table = "\n".join(lines)
    print(head)
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write(head + "\n\n" + table + "\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
