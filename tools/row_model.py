#!/usr/bin/env python3
"""CPU model of the slots the tile kernel walks over one rebuild cycle (numpy only, ~20 s, outside any timed path).

What it models: ``synthetic.config_north_star(16)`` (N = 16,384: 64 tiles, 256 waves), rows ordered as the
plan orders them -- core | sure | near | buffer shell 0 .. S-1, ascending neighbor index inside a class -- and a rebuild
cycle of 8 steps of ballistic motion x + v dt k (Maxwell velocities at kT = 1, dt = 0.005) under the displacement bound
of the full-size run, 0.028 k. Per wave and step it counts the batches of 4 entries per lane the kernel walks for a given
row-end granularity (whole 16-byte chunks = 2 batches, or single batches) and shell count, and how many of those hold a
pair in range for at least one lane ("hot"); the others ("cold") are rejected by the skip test after their 12 gathers.
"tile" is the mean over tiles of the longest of the four waves: what a workgroup occupies its slot for.

    python tools/row_model.py [--ncell 16] [--json]

Not a measurement: it prices nothing, it only counts slots. profiles/row_ends.md sets it against the plan's own tables.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from azplugins_amd import synthetic as syn  # noqa: E402

STEPS = 8
BOUND_PER_STEP = 0.028  # fastest of 2^20 particles at kT = 1, dt = 0.005
DT = 0.005


def neighbor_rows(xyz, L, r_list):
    """Full neighbor rows as padded arrays [particle, entry] (indices ascending; valid marks real entries) and the
    separations when the list is built; by blocks of 256 rows."""
    n = xyz.shape[0]
    rows = []
    for b0 in range(0, n, 256):
        d2 = np.zeros((min(256, n - b0), n))
        for c in range(3):
            d = xyz[b0:b0 + 256, None, c] - xyz[None, :, c]
            d -= L[c] * np.rint(d / L[c])
            d2 += d * d
        d2[np.arange(d2.shape[0]), np.arange(b0, b0 + d2.shape[0])] = np.inf
        rows += [np.nonzero(d2[i] <= r_list * r_list)[0] for i in range(d2.shape[0])]
    width = (max(len(r) for r in rows) + 7) // 8 * 8
    idx = np.tile(np.arange(n)[:, None], (1, width))
    valid = np.zeros((n, width), dtype=bool)
    for i, r in enumerate(rows):
        idx[i, :len(r)] = r
        valid[i, :len(r)] = True
    return idx, valid


def separations(xyz, L, idx):
    d = xyz[:, None, :] - xyz[idx]
    d -= L * np.rint(d / L)
    return np.sqrt((d * d).sum(axis=2))


def row_classes(r, valid, r_cut, r_buff, r_inner, shells, stored):
    """Row class of every entry as the plan compilers cut them (single-precision margins included): 0 core, 1 sure,
    2 near, 3 + s buffer shell s; padding last. ``stored``: shell classes a row really has; the shells from stored - 1 on
    are filed together (a shell is a lower bound, so filing an entry lower is conservative)."""
    w = r_buff / shells
    cls = np.full(r.shape, 2, dtype=np.int64)
    cls[r < r_cut - r_buff - 2e-4] = 1
    cls[r < r_inner] = 0
    out = r * r >= r_cut * r_cut * 1.0001
    s = np.floor((r[out] * 0.99995 - r_cut) / w)
    cls[out] = 3 + np.clip(s, 0, min(shells, stored) - 1).astype(np.int64)
    cls[~valid] = 3 + shells
    return cls


def model(cfg, shells, stored, half):
    n = cfg["xyz"].shape[0]
    r_cut, r_buff = cfg["r_cut"], cfg["r_buff"]
    r_inner = 2.0 ** (1.0 / 6.0) * cfg["params"]["sigma"] + r_buff + 1e-3  # what azplugins_amd.pair passes
    valid, r_step = cfg["_valid"], cfg["_r_step"]
    w = r_buff / shells
    n_waves = n // 64
    cls = row_classes(r_step[0], valid, r_cut, r_buff, r_inner, shells, stored)
    order = np.argsort(cls, axis=1, kind="stable")  # class by class, ascending neighbor index inside a class
    cls_sorted = np.take_along_axis(cls, order, axis=1)
    # entries up to the end of "near" [0] / of shell s [1 + s], per row
    ends = np.stack([(cls_sorted < 3 + s).sum(axis=1) for s in range(shells + 1)], axis=1)
    walked = np.zeros((STEPS, n_waves))
    hot = np.zeros((STEPS, n_waves))
    tile_longest = np.zeros((STEPS, n_waves // 4))
    for k in range(STEPS):
        n_sh = min(int(np.ceil(2.0 * BOUND_PER_STEP * k * (1 + 1e-12) / w)), shells)
        longest = ends[:, n_sh].reshape(n_waves, 64).max(axis=1)
        nb = (longest + 3) // 4 if half else 2 * ((longest + 7) // 8)
        inr = np.take_along_axis((r_step[k] < r_cut) & valid, order, axis=1)
        any_in = inr.reshape(n_waves, 64, -1, 4).any(axis=(1, 3))  # [wave, batch]
        any_in &= np.arange(any_in.shape[1])[None, :] < nb[:, None]
        walked[k] = nb
        hot[k] = any_in.sum(axis=1)
        tile_longest[k] = nb.reshape(-1, 4).max(axis=1)  # a workgroup holds its LDS and its slot until its slowest wave ends
    in_range_len = ((r_step[0] < r_cut) & valid).sum(axis=1)
    return dict(shells=shells, stored_shell_classes=min(shells, stored), row_end="batch" if half else "chunk",
                in_range_row_mean=float(in_range_len.mean()), in_range_row_std=float(in_range_len.std()),
                walked_by_step=[float(v) for v in walked.mean(axis=1)], hot_by_step=[float(v) for v in hot.mean(axis=1)],
                walked_mean=float(walked.mean()), hot_mean=float(hot.mean()),
                tile_longest_mean=float(tile_longest.mean()))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--ncell", type=int, default=16)
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    cfg = syn.config_north_star(args.ncell)
    idx, cfg["_valid"] = neighbor_rows(cfg["xyz"], cfg["L"], cfg["r_cut"] + cfg["r_buff"])
    tag = np.arange(cfg["xyz"].shape[0], dtype=np.uint64)
    vel = np.stack([syn.normal(77, tag, c) for c in range(3)], axis=1)  # Maxwell, kT = 1, unit mass
    cfg["_r_step"] = [separations(cfg["xyz"] + vel * (DT * k), cfg["L"], idx) for k in range(STEPS)]
    cases = [(8, 8, False), (8, 8, True), (16, 16, False), (16, 16, True), (16, 13, True), (32, 32, True)]
    out = [model(cfg, *c) for c in cases]
    if args.json:
        print(json.dumps(out))
        return
    print("N = %d, %d waves; in-range row length %.1f +- %.1f" % (cfg["xyz"].shape[0], cfg["xyz"].shape[0] // 64,
                                                                out[0]["in_range_row_mean"], out[0]["in_range_row_std"]))
    print("%7s %7s %7s | %s | %7s %7s %7s" % ("shells", "classes", "row end", " ".join("step %d" % k for k in range(STEPS)), "walked", "hot", "tile"))
    for r in out:
        print("%7d %7d %7s | %s | %7.2f %7.2f %7.2f" % (r["shells"], r["stored_shell_classes"], r["row_end"],
                                                         " ".join("%6.2f" % v for v in r["walked_by_step"]), r["walked_mean"], r["hot_mean"],
                                                         r["tile_longest_mean"]))


if __name__ == "__main__":
    main()
