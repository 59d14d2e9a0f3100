"""Event-timed cost of the velocity-field computes at N = 2^20 (north-star FCC lattice, azplugins_amd.synthetic):
the center-of-mass velocity, a 100-bin Cartesian profile, a 100 x 100 Cartesian field and a 50 x 8 x 20 cylindrical
field, each with the particles in lattice (sorted) order and shuffled. Per case: microseconds per call of libazp's
sums + normalize (device events around `--calls` back-to-back calls after a warm-up), the fraction of the bound of
one pass over pos + vel (64 B per particle at the 8 TB/s HBM peak), the same quantity computed naively in torch
(binning + index_add_ of float64 rows) beside it, and whether each gives bit-identical results on two calls.

  python tools/velocity_field_probe.py [--calls 50] [--out profiles/velocity_field.md]
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

HBM_PEAK = 8.0e12  # B/s, MI355X spec
BYTES_PER_PARTICLE = 64  # pos + vel, one pass


def _cases(L):
    return [
        ("VelocityCompute", "cartesian", (0, 0, 0), (0, 0, 0), (0, 0, 0)),
        ("Cartesian 100", "cartesian", (100, 0, 0), (-L[0] / 2, 0, 0), (L[0] / 2, 0, 0)),
        ("Cartesian 100x100", "cartesian", (100, 100, 0), (-L[0] / 2, -L[1] / 2, 0), (L[0] / 2, L[1] / 2, 0)),
        ("Cylindrical 50x8x20", "cylindrical", (50, 8, 20), (0, 0, -L[2] / 2), (L[0] / 2, 2 * math.pi, L[2] / 2)),
    ]


def _torch_naive(pos, vel, num_bins, lower, upper, cyl, L):
    """The scatter-add a user would write: bin in torch, then index_add_ of (m, m v) rows."""
    import torch

    x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
    Lt = torch.tensor(L, dtype=torch.float64, device=pos.device)
    xyz = pos[:, :3] - Lt * torch.floor(pos[:, :3] / Lt + 0.5)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    m = vel[:, 3]
    p = vel[:, :3] * m[:, None]
    ok = torch.ones_like(m, dtype=torch.bool)
    idx = [torch.zeros_like(m, dtype=torch.int64) for _ in range(3)]
    coords = [x, y, z]
    if cyl:
        r = torch.sqrt(x * x + y * y)
        th = torch.atan2(y, x)
        th = torch.where(th < 0, th + 2 * math.pi, th)
        coords = [r, th, z]
        rs = torch.where(r > 0, r, torch.ones_like(r))
        c = torch.where(r > 0, x / rs, torch.ones_like(r))
        s = torch.where(r > 0, y / rs, torch.zeros_like(r))
        p = torch.stack([c * p[:, 0] + s * p[:, 1], -s * p[:, 0] + c * p[:, 1], p[:, 2]], dim=1)
    for d in range(3):
        if num_bins[d] > 0:
            f = torch.floor(((coords[d] - lower[d]) / (upper[d] - lower[d])) * num_bins[d])
            ok &= (f >= 0) & (f < num_bins[d])
            idx[d] = f.clamp(0, num_bins[d] - 1).to(torch.int64)
    ny = max(num_bins[1], 1)
    nz = max(num_bins[2], 1)
    b = idx[2] + nz * (idx[1] + ny * idx[0])
    n_bins = max(num_bins[0], 1) * ny * nz
    rows = torch.cat([m[:, None], p], dim=1)[ok]
    sums = torch.zeros((n_bins, 4), dtype=torch.float64, device=pos.device)
    sums.index_add_(0, b[ok], rows)
    return sums


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="write the markdown table here")
    ap.add_argument("--json", default=None, help="write the raw numbers here")
    args = ap.parse_args()

    import torch

    import azplugins_amd as azp
    from azplugins_amd import _lib
    from azplugins_amd import synthetic as syn

    if not torch.cuda.is_available():
        raise SystemExit("velocity_field_probe: no GPU (the numbers come from a GPU run only)")
    dev = torch.device("cuda:0")
    cfg = syn.config_north_star()
    N = cfg["xyz"].shape[0]
    L = [float(v) for v in cfg["L"]]
    tag = np.arange(N, dtype=np.uint64)
    vel = np.stack([syn.normal(21, tag, c) for c in range(3)] + [1.0 + syn.u01(22, tag, 0)], axis=1)
    pos = syn.pos4(cfg["xyz"])
    shuffle = np.random.default_rng(0).permutation(N)
    orders = {"sorted": np.arange(N), "shuffled": shuffle}
    lib = _lib.lib()
    stream = _lib.raw_stream(dev)
    box = azp.Box(*L).to_c()
    rows = []
    for order_name, order in orders.items():
        d_pos = torch.from_numpy(np.ascontiguousarray(pos[order])).to(dev)
        d_vel = torch.from_numpy(np.ascontiguousarray(vel[order])).to(dev)
        for name, coords, nb, lo, hi in _cases(L):
            n_bins = int(np.prod([k for k in nb if k > 0])) if any(nb) else 1
            a = _lib.VelocityFieldArgs()
            a.d_pos, a.d_vel, a.N = d_pos.data_ptr(), d_vel.data_ptr(), N
            a.coordinates = _lib.COORDINATES_CYLINDRICAL if coords == "cylindrical" else _lib.COORDINATES_CARTESIAN
            a.box = box
            for d in range(3):
                a.num_bins[d], a.lower[d], a.upper[d] = nb[d], lo[d], hi[d]
            need = C.c_uint64(0)
            _lib.check(lib.azp_velocity_field_scratch_size(C.byref(a), C.byref(need)))
            scratch = torch.empty(max(int(need.value), 8), dtype=torch.uint8, device=dev)
            sums = torch.empty((n_bins, 4), dtype=torch.float64, device=dev)
            v_out = torch.empty((n_bins, 3), dtype=torch.float64, device=dev)
            a.d_sums, a.d_scratch, a.scratch_bytes = sums.data_ptr(), scratch.data_ptr(), scratch.numel()

            def ours():
                _lib.check(lib.azp_velocity_field_sums(C.byref(a), stream))
                _lib.check(lib.azp_velocity_field_normalize(sums.data_ptr(), n_bins, v_out.data_ptr(), stream))

            def naive():
                s = _torch_naive(d_pos, d_vel, nb, lo, hi, coords == "cylindrical", L)
                m = s[:, 0:1]
                return torch.where(m > 0, s[:, 1:] / torch.where(m > 0, m, torch.ones_like(m)), torch.zeros_like(s[:, 1:]))

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

            t_ours = timed(ours)
            ours()
            r1 = v_out.clone()
            ours()
            r2 = v_out.clone()
            t_naive = timed(naive)
            n1, n2 = naive(), naive()
            torch.cuda.synchronize()
            bound_us = BYTES_PER_PARTICLE * N / HBM_PEAK * 1e6
            tiles = (n_bins + 511) // 512
            rows.append(dict(case=name, order=order_name, bins=n_bins, tiles=tiles, scratch_bytes=int(need.value), us=t_ours,
                             bound_us=bound_us, frac_of_bound=bound_us / t_ours, torch_us=t_naive,
                             ours_bit_identical=bool(torch.equal(r1, r2)), torch_bit_identical=bool(torch.equal(n1, n2)),
                             max_abs_diff_vs_torch=float((r1 - n1).abs().max().item())))
            print(json.dumps(rows[-1]), flush=True)
    dev_name = torch.cuda.get_device_name(0)
    lines = ["| case | order | bins | tiles | us / call | bound us (64 B/particle @ 8 TB/s) | fraction of bound | torch index_add_ us | "
             "ours bit-identical | torch bit-identical |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %s | %s | %d | %d | %.1f | %.1f | %.2f | %.1f | %s | %s |" % (
            r["case"], r["order"], r["bins"], r["tiles"], r["us"], r["bound_us"], r["frac_of_bound"], r["torch_us"],
            "yes" if r["ours_bit_identical"] else "no", "yes" if r["torch_bit_identical"] else "no"))
    table = "\n".join(lines)
    print("device: %s, N = %d, %d calls after %d warm-up calls" % (dev_name, N, args.calls, args.warmup))
    print(table)
    if args.out:
        with open(args.out, "w") as f:
            f.write("device: %s, N = %d, %d calls after %d warm-up calls\n\n%s\n" % (dev_name, N, args.calls, args.warmup, table))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
