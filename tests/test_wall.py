"""azplugins_amd.wall without a GPU: the NumPy restatement (tests/wall_ref.py) against the mpmath fixture
(tests/golden/wall_cases.json), its own consistency (F = -dE/dd, continuity at r_extrap), the C ABI (struct layout,
exported symbols, argument errors, the two parameter folds) and the validation of the Python classes."""

import ctypes as C
import json
import math
import os
import pickle
import subprocess
import tempfile

import numpy as np
import pytest

import wall_ref as ref
from azplugins_amd import _lib, wall

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "wall_cases.json")) as _f:
    CASES = json.load(_f)

# max(|E - E_mp|, |F - F_mp|) / max(|F_mp|, |E_mp|, 1e-3) of wall_ref on the fixture, as printed by
# `python tests/golden/make_wall_cases.py --check` (1.790e-15 and 1.991e-14), rounded up
F64_DEVIATION = {"lj93": 1.8e-15, "colloid": 2.0e-14}

LJ = dict(epsilon=2.0, sigma=1.5, r_cut=4.0, r_extrap=1.2)
CO = dict(A=100.0, sigma=1.0, a=1.5, r_cut=4.5, r_extrap=1.8)


def _ulps(a, b):
    return abs(a - b) / math.ulp(max(abs(a), abs(b))) if a != b else 0.0


@pytest.mark.parametrize("kind", ["lj93", "colloid"])
def test_ref_matches_mpmath_fixture(kind):
    rows = CASES[kind]["named"] + CASES[kind]["random"]
    assert len(CASES[kind]["named"]) == 3 and len(CASES[kind]["random"]) >= 200
    worst = 0.0
    for row in rows:
        E, F = ref.POTENTIALS[kind](row, row["r"])
        worst = max(worst, max(abs(E - row["E"]), abs(F - row["F"])) / max(abs(row["F"]), abs(row["E"]), 1e-3))
    print("%s: float64 deviation %.3e" % (kind, worst))
    assert worst <= F64_DEVIATION[kind]
    # vectorised evaluation (what the GPU tests use) agrees with the one-at-a-time results
    for row in rows[:3]:
        E, F = ref.POTENTIALS[kind](row, np.array([row["r"]]))
        assert abs(E[0] - row["E"]) <= F64_DEVIATION[kind] * max(abs(row["F"]), abs(row["E"]))


def test_fixture_named_cases_are_the_documented_values():
    want = {"lj93": [(3.5015625, 72.0140625), (-1.73333333333333, -2.4), (-0.4293126144, -0.50872541184)],
            "colloid": [(-10.3194612349897, 129.705264761091), (-8.03926338005167, -13.3085141863142),
                        (-1.40435641184175, -1.18966502652157)]}
    for kind, rows in want.items():
        for row, (E, F) in zip(CASES[kind]["named"], rows):
            assert row["E"] == pytest.approx(E, rel=1e-13) and row["F"] == pytest.approx(F, rel=1e-13)
    a = {row["a"] for row in CASES["colloid"]["random"]}
    assert a == {0.5, 1.5, 2.5}
    gaps = [row["r"] - row["a"] for row in CASES["colloid"]["random"]]
    assert min(gaps) >= 0.2 and max(gaps) <= 3.0


WALLS = [dict(kind="plane", origin=(1.0, 0.5, -3.0), normal=(1.0, 2.0, 2.0)),
         dict(kind="sphere", radius=4.5, origin=(0.5, -0.5, 0.25), inside=True),
         dict(kind="sphere", radius=3.0, origin=(0.5, -0.5, 0.25), inside=False),
         dict(kind="cylinder", radius=4.5, origin=(0.5, -0.5, 0.0), axis=(0.0, 0.0, 1.0), inside=True),
         dict(kind="cylinder", radius=2.5, origin=(0.0, 0.0, 0.0), axis=(1.0, 1.0, 0.0), inside=False)]


@pytest.mark.parametrize("kind,p", [("lj93", LJ), ("colloid", CO)])
@pytest.mark.parametrize("mode", ["none", "shift"])
def test_ref_force_is_minus_energy_gradient(kind, p, mode):
    """F = -dE/dx by central differences, through every geometry, standard and extrapolated branch."""
    rng = np.random.default_rng(3)
    pos = rng.uniform(-6.0, 6.0, (1500, 3))
    tid = np.zeros(1500, dtype=int)
    h = 1e-6
    for q in (p, dict(p, r_extrap=0.0)):
        for geom in WALLS:
            F, E, D = ref.evaluate(kind, [geom], [q], mode, pos, tid, 12.0)
            # leave out what a step of h carries across a branch point or, in standard mode, into the core
            lo = q["a"] + 0.2 if (kind == "colloid" and q["r_extrap"] == 0.0) else 0.0
            ok = (np.abs(D[0] - q["r_cut"]) > 1e-3) & (np.abs(D[0]) > 1e-3) & ((D[0] > lo + 1e-3) | (D[0] <= 0.0) | (q["r_extrap"] > 0.0))
            ok &= np.abs(D[0] - q["r_extrap"]) > 1e-3
            assert (ok & (E[0] != 0.0)).sum() > 20
            for k in range(3):
                dp = np.zeros(3)
                dp[k] = h
                Ep = ref.evaluate(kind, [geom], [q], mode, pos + dp, tid, 12.0)[1][0]
                Em = ref.evaluate(kind, [geom], [q], mode, pos - dp, tid, 12.0)[1][0]
                num = -(Ep - Em) / (2 * h)
                scale = np.maximum(np.abs(F[0]).max(axis=1), 1.0)
                assert np.all(np.abs(num - F[0][:, k])[ok] <= 1e-5 * scale[ok])


@pytest.mark.parametrize("kind,p", [("lj93", LJ), ("colloid", CO)])
@pytest.mark.parametrize("mode", ["none", "shift"])
def test_ref_continuous_across_r_extrap(kind, p, mode):
    e = p["r_extrap"]
    geom = dict(kind="plane", origin=(0.0, 0.0, 0.0), normal=(0.0, 0.0, 1.0))  # (d is z, exactly)
    z = np.array([e - 1e-9, e, e + 1e-9])
    pos = np.stack([np.zeros(3), np.zeros(3), z], axis=1)
    F, E, D = ref.evaluate(kind, [geom], [p], mode, pos, np.zeros(3, dtype=int), 20.0)
    V, Fe = ref.POTENTIALS[kind](p, e)
    slope = abs(Fe) + 1.0
    assert abs(E[0][0] - E[0][1]) < 4e-9 * slope and abs(E[0][2] - E[0][1]) < 4e-9 * slope
    assert abs(F[0][0, 2] - F[0][1, 2]) < 1e-6 * slope and abs(F[0][2, 2] - F[0][1, 2]) < 1e-6 * slope * 50
    # at d == r_extrap exactly the standard branch is taken: V(e) - shift, -V'(e)
    shift = ref.POTENTIALS[kind](p, p["r_cut"])[0] if mode == "shift" else 0.0
    assert E[0][1] == V - shift and F[0][1, 2] == Fe
    # far behind the wall the extrapolation goes on, linearly
    far = ref.evaluate(kind, [geom], [p], mode, np.array([[0.0, 0.0, -2.5]]), [0], 20.0)
    assert far[1][0][0] == (V - shift) + Fe * (e + 2.5) and far[0][0][0, 2] == Fe


def test_abi_wall_struct_layout():
    names = ["azp_wall", "azp_wall_args"]
    fields = ["d_force", "d_virial", "virial_pitch", "N", "ntypes", "d_pos", "box", "d_params", "n_walls", "block_size", "walls"]
    wfields = ["kind", "inside", "origin", "axis", "radius"]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "azp.h"\nint main(){' + "".join(
        'printf("%%zu\\n", sizeof(%s));' % n for n in names) + "".join(
        'printf("%%zu\\n", offsetof(azp_wall_args, %s));' % f for f in fields) + "".join(
        'printf("%%zu\\n", offsetof(azp_wall, %s));' % f for f in wfields) + \
        'printf("%d\\n%d\\n", AZP_WALL_MAX, AZP_WALL_PARAM_DOUBLES);return 0;}'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    assert got[0] == C.sizeof(_lib.Wall) == 64
    assert got[1] == C.sizeof(_lib.WallArgs)
    for k, f in enumerate(fields):
        assert got[2 + k] == getattr(_lib.WallArgs, f).offset, f
    for k, f in enumerate(wfields):
        assert got[2 + len(fields) + k] == getattr(_lib.Wall, f).offset, f
    assert got[-2:] == [_lib.WALL_MAX, _lib.WALL_PARAM_DOUBLES] == [16, 8]


def test_abi_wall_symbols_and_argument_errors():
    lib = _lib.lib()
    plane = _lib.Wall(_lib.WALL_PLANE, 0, (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 0.0)

    def args(**kw):
        a = _lib.WallArgs()
        a.n_walls = 1
        a.walls[0] = plane
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    need = C.c_uint64(0)
    for name in ("azp_wall_forces_lj93", "azp_wall_forces_colloid"):
        fn = getattr(lib, name)
        assert fn(None, None) == -1
        assert fn(C.byref(args()), None) == 0               # N = 0: nothing to do
        assert fn(C.byref(args(n_walls=0)), None) == -1
        assert fn(C.byref(args(n_walls=17)), None) == -1
        assert fn(C.byref(args(block_size=96)), None) == -1
        assert fn(C.byref(args(block_size=512)), None) == -1
        assert fn(C.byref(args(block_size=128)), None) == 0
        bad = args()
        bad.walls[0].kind = 3
        assert fn(C.byref(bad), None) == -1
        assert fn(C.byref(args(ntypes=1025)), None) == _lib.ERROR_TOO_MANY_TYPES
        assert fn(C.byref(args(N=4, ntypes=1)), None) == -1  # no arrays
    for name in ("azp_wall_net_forces_lj93", "azp_wall_net_forces_colloid"):
        fn = getattr(lib, name)
        assert fn(None, None, None, 0, None) == -1
        assert fn(C.byref(args()), None, None, 0, None) == -1   # no output
        assert fn(C.byref(args(n_walls=17)), None, None, 0, None) == -1
        assert fn(C.byref(args(N=4, ntypes=1)), None, None, 0, None) == -1
    assert lib.azp_wall_net_forces_scratch_size(C.byref(args(N=1000, n_walls=3)), C.byref(need)) == 0
    assert need.value == 4 * 3 * 8 * 4                       # ceil(1000 / 256) partials of 4 doubles for 3 walls
    assert lib.azp_wall_net_forces_scratch_size(C.byref(args(n_walls=0)), C.byref(need)) == -1
    assert lib.azp_wall_net_forces_scratch_size(C.byref(args()), None) == -1


def _row(name, *a):
    row = (C.c_double * _lib.WALL_PARAM_DOUBLES)(*([7.0] * _lib.WALL_PARAM_DOUBLES))
    rc = getattr(_lib.lib(), name)(*a, row)
    return rc, list(row)


@pytest.mark.parametrize("mode", ["none", "shift"])
def test_params_make_agrees_with_ref_fold(mode):
    shift_mode = 1 if mode == "shift" else 0
    lj_sets = [LJ, dict(LJ, r_extrap=0.0), dict(epsilon=0.7, sigma=0.9, r_cut=2.7, r_extrap=0.81),
               dict(epsilon=1.0, sigma=1.0, r_cut=3.0, r_extrap=1.8)]
    for p in lj_sets:
        rc, row = _row("azp_wall_lj93_params_make", p["epsilon"], p["sigma"], p["r_cut"], p["r_extrap"], shift_mode)
        assert rc == 0
        c, e, shift, Ve, Fe = ref.fold("lj93", p, mode)
        assert row[2] == c and row[3] == e and row[7] == 0.0
        assert row[0] == p["epsilon"] and row[1] == p["sigma"]  # (LJ93 keeps them as given: csrc/wall_forces.hip)
        for got, want in zip(row[4:7], (shift, Ve, Fe)):
            assert _ulps(got, want) <= 4, (p, got, want)
    co_sets = [CO, dict(CO, r_extrap=0.0), dict(A=40.0, sigma=1.1, a=0.5, r_cut=2.5, r_extrap=0.8),
               dict(A=150.0, sigma=0.9, a=2.5, r_cut=5.0, r_extrap=2.8)]
    for p in co_sets:
        rc, row = _row("azp_wall_colloid_params_make", p["A"], p["sigma"], p["a"], p["r_cut"], p["r_extrap"], shift_mode)
        assert rc == 0
        c, e, shift, Ve, Fe = ref.fold("colloid", p, mode)
        assert row[2] == c and row[3] == e and row[7] == p["a"]
        assert _ulps(row[0], p["A"] * p["sigma"] ** 6 / 7560.0) <= 4 and _ulps(row[1], p["A"] / 6.0) <= 1
        for got, want in zip(row[4:7], (shift, Ve, Fe)):
            assert _ulps(got, want) <= 4, (p, got, want)
    # a type that feels nothing: a row of zeros
    for a in ((0.0, 1.0, 3.0, 0.0), (1.0, 1.0, 0.0, 0.0)):
        assert _row("azp_wall_lj93_params_make", *a, shift_mode) == (0, [0.0] * 8)
    for a in ((0.0, 1.0, 1.5, 3.0, 0.0), (10.0, 1.0, 0.0, 3.0, 0.0), (10.0, 1.0, -1.0, 3.0, 0.0), (10.0, 1.0, 1.5, 0.0, 0.0)):
        assert _row("azp_wall_colloid_params_make", *a, shift_mode) == (0, [0.0] * 8)
    # rejected: r_extrap >= r_cut, negative lengths, xplor, the colloid's radius at or beyond r_cut / r_extrap
    assert _row("azp_wall_lj93_params_make", 1.0, 1.0, 3.0, 3.0, shift_mode)[0] == -1
    assert _row("azp_wall_lj93_params_make", 1.0, 1.0, -3.0, 0.0, shift_mode)[0] == -1
    assert _row("azp_wall_lj93_params_make", 1.0, 1.0, 3.0, -0.1, shift_mode)[0] == -1
    assert _row("azp_wall_lj93_params_make", 1.0, 1.0, 3.0, 0.0, 2)[0] == -1
    assert _row("azp_wall_colloid_params_make", 10.0, 1.0, 1.5, 1.5, 0.0, shift_mode)[0] == -1
    assert _row("azp_wall_colloid_params_make", 10.0, 1.0, 1.5, 3.0, 1.5, shift_mode)[0] == -1
    assert _lib.lib().azp_wall_lj93_params_make(1.0, 1.0, 3.0, 0.0, 0, None) == -1


def test_geometries_validate_normalise_and_pickle():
    p = wall.Plane(origin=(1, 0.5, -3), normal=(1, 2, 2))
    assert p.origin == (1.0, 0.5, -3.0) and p.normal == (1.0 / 3.0, 2.0 / 3.0, 2.0 / 3.0)
    assert tuple(ref.unit((1, 2, 2))) == p.normal
    assert wall.Plane().normal == (0.0, 0.0, 1.0) and wall.Plane().origin == (0.0, 0.0, 0.0)
    with pytest.raises(ValueError):
        wall.Plane(normal=(0, 0, 0))
    with pytest.raises(ValueError):
        wall.Cylinder(2.0, axis=(0, 0, 0))
    with pytest.raises(ValueError):
        wall.Plane(origin=(0, 0))
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            wall.Sphere(bad)
    c = wall.Cylinder(2.5, origin=(0, 0, 1), axis=(1, 1, 0), inside=False)
    assert c.axis == tuple(ref.unit((1, 1, 0))) and c.inside is False and c.radius == 2.5
    s = wall.Sphere(4.5, origin=(0.5, -0.5, 0.25))
    assert s.inside is True
    for g in (p, c, s):
        other = pickle.loads(pickle.dumps(g))
        assert other == g and type(other) is type(g) and repr(other) == repr(g)
    assert wall.Sphere(4.5) != wall.Sphere(4.5, inside=False) and wall.Sphere(4.5) != wall.Cylinder(4.5)
    # the C mirror
    w = c._c()
    assert (w.kind, w.inside, tuple(w.origin), tuple(w.axis), w.radius) == (_lib.WALL_CYLINDER, 0, (0.0, 0.0, 1.0), c.axis, 2.5)
    w = p._c()
    assert (w.kind, tuple(w.origin), tuple(w.axis)) == (_lib.WALL_PLANE, p.origin, p.normal)
    assert s._c().kind == _lib.WALL_SPHERE and s._c().inside == 1 and s._c().radius == 4.5


def test_potential_validation():
    import azplugins_amd as azp

    assert azp.wall is wall
    plane = wall.Plane()
    for cls in (wall.LJ93, wall.Colloid):
        with pytest.raises(ValueError):
            cls(walls=[])
        with pytest.raises(ValueError):
            cls(walls=[plane] * 17)
        assert len(cls(walls=[plane] * 16).walls) == 16
        with pytest.raises(ValueError):
            cls(walls=[plane], mode="xplor")
        with pytest.raises(TypeError):
            cls(walls=[(0, 0, 1)])
        w = cls(walls=[plane])
        assert w.mode == "shift" and cls(walls=[plane], mode="none").mode == "none"
        with pytest.raises(ValueError):
            w.mode = "xplor"
        with pytest.raises(azp.AzpError):
            w.forces  # not attached
        with pytest.raises(azp.AzpError):
            w.wall_forces
    lj = wall.LJ93(walls=[plane])
    lj.params["A"] = dict(epsilon=1.0, sigma=1.0, r_cut=3.0)
    assert lj.params["A"] == dict(epsilon=1.0, sigma=1.0, r_cut=3.0, r_extrap=0.0)
    lj.params["A"]["r_extrap"] = 1.8
    assert lj.params["A"]["r_extrap"] == 1.8
    for bad in (dict(epsilon=1.0, sigma=1.0, r_cut=3.0, r_extrap=3.0), dict(epsilon=1.0, sigma=1.0, r_cut=3.0, r_extrap=3.5),
                dict(epsilon=1.0, sigma=1.0, r_cut=-3.0), dict(epsilon=1.0, sigma=1.0, r_cut=3.0, a=1.0),
                dict(epsilon=1.0, sigma=1.0)):
        with pytest.raises(ValueError):
            lj.params["B"] = bad
    assert "B" not in lj.params
    lj.params["C"] = dict(epsilon=1.0, sigma=1.0, r_cut=0.0)  # disabled
    co = wall.Colloid(walls=[plane])
    co.params["A"] = dict(A=100.0, sigma=1.0, a=1.5, r_cut=4.0, r_extrap=1.8)
    for bad in (dict(A=100.0, sigma=1.0, a=1.5, r_cut=1.5), dict(A=100.0, sigma=1.0, a=1.5, r_cut=1.0),
                dict(A=100.0, sigma=1.0, a=1.5, r_cut=4.0, r_extrap=1.5), dict(A=100.0, sigma=1.0, a=1.5, r_cut=4.0, r_extrap=0.7),
                dict(A=100.0, sigma=1.0, a=1.5, r_cut=4.0, r_extrap=4.0), dict(A=100.0, sigma=1.0, a=1.5, r_cut=4.0, epsilon=1.0),
                dict(A=100.0, sigma=1.0, r_cut=4.0)):
        with pytest.raises(ValueError):
            co.params["B"] = bad
    co.params["C"] = dict(A=100.0, sigma=1.0, a=1.5, r_cut=0.0)  # disabled: r_cut <= a is not an error
    # the rows the classes hand to the kernel are libazp's fold
    assert lj._row(lj.params.get_raw("A"))[2:4] == [3.0, 1.8] and lj._row(lj.params.get_raw("C")) == [0.0] * 8
    c, e, shift, Ve, Fe = ref.fold("colloid", co.params.get_raw("A"), "shift")
    row = co._row(co.params.get_raw("A"))
    assert row[2:4] == [c, e] and row[7] == 1.5 and all(_ulps(g, w) <= 4 for g, w in zip(row[4:7], (shift, Ve, Fe)))
    co.mode = "none"
    assert co._row(co.params.get_raw("A"))[4] == 0.0
