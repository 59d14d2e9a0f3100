#!/usr/bin/env python3
"""Condense the output of tools/profile_passes.sh (gpurun_out/<dir>) into the files kept under profiles/:
r02_kernel_stats.md, r02_bench.json, r02_md_bench.log, r02_plan_cells.md.

    python tools/condense_profiles.py gpurun_out/r02w
"""
import collections
import csv
import glob
import os
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
O = os.path.abspath(sys.argv[1])
P = os.path.join(ROOT, "profiles")


def stats(d, match=("azp::",), top=14):
    f = glob.glob(os.path.join(O, d, "*", "*_kernel_stats.csv"))[0]
    out = ["name,calls,total_ms,avg_us,pct,min_us,max_us"]
    for r in csv.DictReader(open(f)):
        if any(m in r["Name"] for m in match):
            out.append('"%s",%s,%.3f,%.1f,%s,%.1f,%.1f' % (r["Name"][:110], r["Calls"], float(r["TotalDurationNs"]) / 1e6, float(r["AverageNs"]) / 1e3,
                                                         r["Percentage"][:6], float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3))
    return "\n".join(out[: top + 1])


md = ["# rocprofv3 --kernel-trace --stats summaries, round 2 (one MI355X), final binary of the round", "",
      "(the tile plan is compiled straight from the cell list: `plan_cells_kernel` replaces `nlist_cell_kernel` + `plan_build_kernel` on the rebuild "
      "path; the first version of this file, with the list-based pipeline, is in the git history)", ""]
md += ["## bench_stats: `rocprofv3 --kernel-trace --stats -- python3 bench.py --full --no-cpu-baseline --no-side-figures --steps 80 --warmup 8`", "",
       stats("bench_stats"), ""]
md += ["## md_stats: `rocprofv3 --kernel-trace --stats -- python3 tools/md_bench.py --steps 300`", "",
       stats("md_stats", match=("azp::", "rocprim", "copyBuffer", "at::native"), top=18), ""]
md += ["## c4_stats: `rocprofv3 --kernel-trace --stats -- python3 tools/xtiled_probe.py c4`", "", stats("c4_stats"), ""]
md += ["## c5_stats: `rocprofv3 --kernel-trace --stats -- python3 tools/xtiled_probe.py c5`", "", stats("c5_stats"), ""]
open(os.path.join(P, "r02_kernel_stats.md"), "w").write("\n".join(md))
shutil.copy(os.path.join(O, "bench_default.json"), os.path.join(P, "r02_bench.json"))
log = open(os.path.join(O, "md_bench.log")).read().strip().splitlines()[-4:]
log2 = open(os.path.join(O, "md_bench_noprof.log")).read().strip().splitlines()[-4:]
open(os.path.join(P, "r02_md_bench.log"), "w").write("# under rocprofv3 --kernel-trace --stats\n" + "\n".join(log) + "\n# without the profiler\n" + "\n".join(log2) + "\n")

pc = ["# `plan_cells_kernel` (azp_pair_plan_build_from_cells) on the north-star system, N = 1,048,576, 4,096 tiles", "",
      "`python3 tools/plan_cells_probe.py` (cell binning excluded; HIP events around 10 builds). `AZP_PLAN_CELLS_STOP=p` leaves the kernel after phase p "
      "in the profiling build of the library (`make variant SRC=pair_plan_cells NAME=pcprof DEFS=-DAZP_PLAN_CELLS_PROFILE`, "
      "`AZP_LIB_PATH=tools/libazp_pcprof.so`; the plan is then marked invalid); bit 9 (512) skips the row walk. The hooks are compiled out of libazp.so.", "",
      "| run | ms per build |", "|---|---|"]
names = ["whole build, lattice snapshot (bench.py's list)", "phases 0-1: cell set, sort, run table",
         "+ phase 2: candidate tests, raw rows, row walk (class counts, bitmap)", "phases 0-2 without the row walk",
         "+ phase 3: slots, stage list, class cursors",
         "whole build after 100 NVE steps at kT = 1 and a particle sort (Hilbert order: tiles are compact blobs, not aligned cubes)"]
lines = open(os.path.join(O, "plan_cells_phases.log")).read().strip().splitlines()
for n, l in zip(names, lines):
    pc.append("| %s | %s |" % (n, l.split("build_from_cells")[1].split("ms")[0].strip()))
pc += ["", "Phase 4 (compiled rows) is the difference between the whole build and the phase-3 figure.", "",
       "## PMC passes (`rocprofv3 --kernel-trace --pmc ... -- python3 tools/plan_cells_probe.py --reps 3`), mean per launch", "",
       "| counter | mean per launch |", "|---|---|"]
vals = {}
for d in ("pc_sq", "pc_fetch", "pc_write"):
    f = glob.glob(os.path.join(O, d, "*", "*counter_collection.csv"))[0]
    agg = collections.defaultdict(float)
    for r in csv.DictReader(open(f)):
        if "plan_cells" in r["Kernel_Name"]:
            agg[(r["Counter_Name"], r["Dispatch_Id"])] += float(r["Counter_Value"])
    per = collections.defaultdict(list)
    for (c, _), v in agg.items():
        per[c].append(v)
    for c, v in sorted(per.items()):
        vals[c] = sum(v) / len(v)
        pc.append("| %s | %.4g (%d launches) |" % (c, vals[c], len(v)))
pc += ["", "FETCH_SIZE / WRITE_SIZE in KiB as rocprofv3 reports them, uncorrected: the kernel's accesses are 32-byte gathers and 2-byte",
       "scattered stores, widths the guide (MI355X_MICROARCH.md, HBM section) calls uncalibrated -- 2-byte stores appear to be tallied",
       "per request, not per byte (the kernel writes about 0.28 GB of raw rows, 0.30 GB of compiled rows and 25 MB of stage lists per",
       "build). SQ_INSTS_VALU x 4 cycles / 1,024 SIMDs = %.2f M cycles of VALU issue per build: the kernel is bound by VALU issue" % (vals.get("SQ_INSTS_VALU", 0) * 4 / 1024 / 1e6),
       "(candidate tests: 850 per particle, two per step with packed FP32 math) at the ~1.6-1.8 GHz the chip holds under this load.",
       "SQ_LDS_IDX_ACTIVE / 256 CUs = %.2f M cycles: the per-lane LDS reads of the staged candidates are the co-limit." % (vals.get("SQ_LDS_IDX_ACTIVE", 0) / 256 / 1e6)]
pc += ["", "Experiments on the final kernel that changed nothing (same box, 1.37-1.41 ms): three workgroups per CU instead of four",
       "(4 KiB of padding in LDS), candidates as 16-byte records read with `ds_read_b128` instead of three `ds_read2_b32`, 16 raw",
       "entries in flight in the row walks instead of 8, XCD-aware tile order. 2,048 candidates per batch (two workgroups per CU): 1.72 ms.",
       "",
       "One that changed the wrong thing: batches made of every n-th cell of the sorted cell array instead of contiguous ranges (in a",
       "liquid a contiguous range is a slab of space that only some of the four waves' members are next to: 1.44x the mean wave's work per",
       "batch against 1.04x). The build of the melted system went from 1.68 to 1.54 ms, the MD step from 0.453 to 0.476 ms: the rows then list",
       "their entries batch by batch instead of in ascending slot order, and the force kernel, LDS-bound as much as VALU-bound, pays more",
       "for that than the build saves. Not kept.",
       "",
       "And one that bought robustness at a price: 1,024 instead of 512 cells around a tile with a 16-bit run table (first cell | length;",
       "the candidate bounds then come from two more LDS reads at every run transition). The thin boundary shells of a decomposed DPD fluid",
       "then compile from the cells too, but the build of the north-star system goes from 1.40 to 1.45 ms (liquid: 1.63 to 1.68). Not kept:",
       "those tiles fall back to the list-based compiler, which handles them."]
open(os.path.join(P, "r02_plan_cells.md"), "w").write("\n".join(pc) + "\n")
print("\n".join(pc))
