"""Event-timed cost of azp_nlist_bin alone (csrc/cell_bin.hpp + the per-cell sort of csrc/nlist.hip), through the C ABI,
after a run-in: the north-star liquid (N = 2^20, FCC at rho* = 0.8) on --dims^3 cells of the whole box, in shuffled
and in cell-sorted memory order. 32^3 cells take the single-workgroup scan (8 blocks of 4,096: its longest run), 41^3
the three-kernel scan. Every figure is the mean over --repeats windows of --calls calls, with the smallest and largest
window. AZP_LIB_PATH picks another build of libazp.so (a parent commit, a variant); --label names it in the output.

  python tools/cell_bin_probe.py [--ncell 64] [--dims 32 41] [--label NAME] [--json FILE]
"""

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncell", type=int, default=64, help="FCC cells per side (64: N = 2^20)")
    ap.add_argument("--dims", type=int, nargs="*", default=[32, 41], help="grid cells per side")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--label", default=None)
    ap.add_argument("--json", default=None, help="write the raw numbers here")
    args = ap.parse_args()

    import torch

    from azplugins_amd import _lib
    from azplugins_amd import synthetic as syn

    if not torch.cuda.is_available():
        raise SystemExit("cell_bin_probe: no GPU (the numbers come from a GPU run only)")
    label = args.label or os.path.basename(_lib.LIB_PATH)
    cfg = syn.config_north_star(args.ncell)
    xyz, L = cfg["xyz"], np.asarray(cfg["L"], dtype=np.float64)
    n = xyz.shape[0]
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    for dim in args.dims:
        ncell = dim ** 3
        c = np.minimum(np.floor((xyz + 0.5 * L) / (L / dim)).astype(np.int64), dim - 1)
        cell = (c[:, 2] * dim + c[:, 1]) * dim + c[:, 0]
        orders = (("shuffled", np.random.default_rng(11).permutation(n)), ("cell-sorted", np.argsort(cell, kind="stable")))
        for name, perm in orders:
            pos = torch.from_numpy(syn.pos4(xyz[perm])).to("cuda:0")
            a = _lib.NlistArgs()
            a.N, a.n_total, a.ntypes = n, n, 1
            a.d_pos = pos.data_ptr()
            a.box = _lib.make_box(L)
            for k in range(3):
                a.grid.dim[k], a.grid.width[k], a.grid.lo[k], a.grid.periodic[k] = dim, L[k] / dim, -0.5 * L[k], 1
            t = {key: torch.zeros(size, dtype=torch.int32, device="cuda:0")
                 for key, size in (("order", n), ("cell_start", ncell + 1), ("cell_of", n), ("cursor", ncell), ("order_tmp", n))}
            a.d_order, a.d_cell_start, a.d_cell_of = t["order"].data_ptr(), t["cell_start"].data_ptr(), t["cell_of"].data_ptr()

            def call():
                _lib.check(_lib.lib().azp_nlist_bin(C.byref(a), t["cursor"].data_ptr(), t["order_tmp"].data_ptr(), stream), "azp_nlist_bin")

            for _ in range(args.warmup):
                call()
            out = []
            for _ in range(args.repeats):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.calls):
                    call()
                e1.record()
                torch.cuda.synchronize()
                out.append(1e3 * e0.elapsed_time(e1) / args.calls)
            # the result against the stable sort, so that a timing is never that of a wrong answer
            got = t["cell_of"].cpu().numpy().astype(np.int64)
            ref = np.argsort(got, kind="stable")
            assert np.count_nonzero(got != cell[perm]) < 10  # (a particle within rounding of a face may differ)
            assert np.array_equal(t["order"].cpu().numpy().astype(np.int64), ref)
            assert np.array_equal(t["cell_start"].cpu().numpy().astype(np.int64), np.searchsorted(got[ref], np.arange(ncell + 1)))
            rows.append(dict(label=label, dims=dim, order=name, N=n, us=float(np.mean(out)), us_min=min(out), us_max=max(out)))
            print(json.dumps(rows[-1]), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
