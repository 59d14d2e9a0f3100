"""Writes tests/golden/wall_cases.json: known answers of the two wall potentials, V(r) and F = -dV/dr without shift,
computed with mpmath at 50 digits (F by mp.diff of V) and rounded to double. Six named cases (the ones quoted in
DESIGN 4.13), one more distance per potential that the GPU test uses as r_cut ("cut": the shift energy), and 200 random
distances per potential; for the colloid a in {0.5, 1.5, 2.5} and a gap r - a in [0.2, 3].

    python tests/golden/make_wall_cases.py           # rewrite the fixture
    python tests/golden/make_wall_cases.py --check   # print the float64 deviation of tests/wall_ref.py on it

The deviation is max(|E - E_mp|, |F - F_mp|) / max(|F_mp|, |E_mp|, 1e-3), the scale the GPU tests use."""

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "wall_cases.json")
N_RANDOM = 200
CUT = {"lj93": 3.0, "colloid": 4.5}


def _mp():
    import mpmath as mp

    mp.mp.dps = 50
    return mp


def lj93_mp(p, r):
    mp = _mp()
    eps, sigma = mp.mpf(p["epsilon"]), mp.mpf(p["sigma"])

    def V(x):
        return eps * (mp.mpf(2) / 15 * (sigma / x) ** 9 - (sigma / x) ** 3)

    return V(mp.mpf(r)), -mp.diff(V, mp.mpf(r))


def colloid_mp(p, r):
    mp = _mp()
    A, sigma, a = mp.mpf(p["A"]), mp.mpf(p["sigma"]), mp.mpf(p["a"])
    C1, C2 = A * sigma ** 6 / 7560, A / 6

    def V(z):
        return (C1 * ((7 * a - z) / (z - a) ** 7 + (7 * a + z) / (z + a) ** 7)
                - C2 * (2 * a * z / (z * z - a * a) + mp.log((z - a) / (z + a))))

    return V(mp.mpf(r)), -mp.diff(V, mp.mpf(r))


def cases():
    rng = np.random.default_rng(20250117)
    lj = [dict(epsilon=2.0, sigma=1.5, r=r) for r in (1.0, 1.5, 2.5)]
    for _ in range(N_RANDOM):
        sigma = float(rng.uniform(0.8, 1.6))
        lj.append(dict(epsilon=float(rng.uniform(0.5, 3.0)), sigma=sigma, r=float(rng.uniform(0.7, 3.0) * sigma)))
    co = [dict(A=100.0, sigma=1.0, a=1.5, r=r) for r in (2.0, 2.5, 4.0)]
    for k in range(N_RANDOM):
        a = (0.5, 1.5, 2.5)[k % 3]
        co.append(dict(A=float(rng.uniform(10.0, 200.0)), sigma=float(rng.uniform(0.8, 1.2)), a=a,
                       r=a + float(rng.uniform(0.2, 3.0))))
    return lj, co


def build():
    out = {}
    lj, co = cases()
    for name, rows, fn in (("lj93", lj, lj93_mp), ("colloid", co, colloid_mp)):
        done = []
        for row in rows:
            p = {k: v for k, v in row.items() if k != "r"}
            E, F = fn(p, row["r"])
            done.append(dict(row, E=float(E), F=float(F)))
        cut = dict(rows[0], r=CUT[name])
        E, F = fn({k: v for k, v in cut.items() if k != "r"}, cut["r"])
        out[name] = dict(named=done[:3], cut=dict(cut, E=float(E), F=float(F)), random=done[3:])
    return out


def deviation(data):
    sys.path.insert(0, os.path.dirname(HERE))
    import wall_ref

    worst = {}
    for name in ("lj93", "colloid"):
        w = 0.0
        for row in data[name]["named"] + [data[name]["cut"]] + data[name]["random"]:
            E, F = wall_ref.POTENTIALS[name](row, row["r"])
            w = max(w, max(abs(E - row["E"]), abs(F - row["F"])) / max(abs(row["F"]), abs(row["E"]), 1e-3))
        worst[name] = w
    return worst


if __name__ == "__main__":
    if "--check" in sys.argv:
        with open(OUT) as f:
            data = json.load(f)
    else:
        data = build()
        with open(OUT, "w") as f:
            json.dump(data, f, indent=0)
            f.write("\n")
    for name, w in deviation(data).items():
        print("%s: float64 deviation of wall_ref on the fixture %.3e" % (name, w))
