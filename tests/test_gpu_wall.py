"""azplugins_amd.wall on the GPU, through ``azp.Simulation`` with the wall among ``Integrator.forces``: known answers
(tests/golden/wall_cases.json, mpmath), random parity against the NumPy restatement (tests/wall_ref.py) for every
geometry, potential, mode and branch, several walls in one launch, the wall in a force list with a pair force and a
ThermodynamicQuantities, NVE in a slit, type changes, and the net force on each wall."""

import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import azplugins_amd as azp
import box_cases
import box_ref
import reduction_ref as red
import wall_ref as ref
from azplugins_amd import _lib
from azplugins_amd import synthetic as syn

pytestmark = pytest.mark.gpu

# Deviation of the float64 restatement from the mpmath fixture on the fixture's own inputs, max(|dE|, |dF|) /
# max(|F|, |E|, 1e-3), as printed by `python tests/golden/make_wall_cases.py --check`; the GPU gets four times that
# (another operation order, refined reciprocals instead of divisions).
F64_DEVIATION = {"lj93": 1.790e-15, "colloid": 1.991e-14}
BOUND = {k: 4.0 * v for k, v in F64_DEVIATION.items()}

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wall_cases.json")) as _f:
    CASES = json.load(_f)

CLS = {"lj93": azp.wall.LJ93, "colloid": azp.wall.Colloid}
L = 12.0
TYPES = ("A", "B", "C")

SINGLE = {
    "plane_z": dict(kind="plane", origin=(0.0, 0.0, -4.0), normal=(0.0, 0.0, 1.0)),
    "plane_oblique": dict(kind="plane", origin=(1.0, 0.5, -3.0), normal=(1.0, 2.0, 2.0)),
    "sphere_in": dict(kind="sphere", radius=4.5, origin=(0.5, -0.5, 0.25), inside=True),
    "sphere_out": dict(kind="sphere", radius=3.0, origin=(0.5, -0.5, 0.25), inside=False),
    "cylinder_in": dict(kind="cylinder", radius=4.5, origin=(0.5, -0.5, 0.0), axis=(0.0, 0.0, 1.0), inside=True),
    "cylinder_out": dict(kind="cylinder", radius=2.5, origin=(0.0, 0.0, 0.0), axis=(1.0, 1.0, 0.0), inside=False),
}
SLIT = [dict(kind="plane", origin=(0.0, 0.0, -4.0), normal=(0.0, 0.0, 1.0)),
        dict(kind="plane", origin=(0.0, 0.0, 4.0), normal=(0.0, 0.0, -1.0))]
NARROW_SLIT = [dict(kind="plane", origin=(0.0, 0.0, -2.5), normal=(0.0, 0.0, 1.0)),
               dict(kind="plane", origin=(0.0, 0.0, 2.5), normal=(0.0, 0.0, -1.0))]
MORE_PLANES = [dict(kind="plane", origin=o, normal=n) for o, n in (
    ((0.0, 0.0, 4.5), (0.0, 0.0, -1.0)), ((-4.5, 0.0, 0.0), (1.0, 0.0, 0.0)), ((4.5, 0.0, 0.0), (-1.0, 0.0, 0.0)),
    ((0.0, -4.5, 0.0), (0.0, 1.0, 0.0)), ((0.0, 4.5, 0.0), (0.0, -1.0, 0.0)), ((-3.0, -3.0, 0.0), (1.0, 1.0, 0.0)),
    ((3.0, 3.0, 0.0), (-1.0, -1.0, 0.0)), ((0.0, 3.0, -3.0), (0.0, -1.0, 1.0)), ((2.0, -1.0, 3.0), (-2.0, 1.0, -2.0)),
    ((-2.0, 2.0, 1.0), (3.0, -1.0, 0.5)))]
ALL16 = list(SINGLE.values()) + MORE_PLANES


def to_azp(w):
    if w["kind"] == "plane":
        return azp.wall.Plane(origin=w["origin"], normal=w["normal"])
    if w["kind"] == "sphere":
        return azp.wall.Sphere(w["radius"], origin=w["origin"], inside=w["inside"])
    return azp.wall.Cylinder(w["radius"], origin=w["origin"], axis=w["axis"], inside=w["inside"])


def type_params(kind, extrap):
    """Types A and B feel the wall with different parameters, C is disabled (r_cut = 0)."""
    if kind == "lj93":
        e = 1.8 if extrap else 0.0
        return [dict(epsilon=1.0, sigma=1.0, r_cut=2.5, r_extrap=e), dict(epsilon=2.0, sigma=1.2, r_cut=2.8, r_extrap=e),
                dict(epsilon=1.0, sigma=1.0, r_cut=0.0, r_extrap=0.0)]
    return [dict(A=50.0, sigma=1.0, a=0.5, r_cut=2.0, r_extrap=0.8 if extrap else 0.0),
            dict(A=100.0, sigma=1.0, a=1.5, r_cut=4.0, r_extrap=1.8 if extrap else 0.0),
            dict(A=100.0, sigma=1.0, a=1.5, r_cut=0.0, r_extrap=0.0)]


_positions = {}


def positions(kind, walls_key, walls, n, extrap, seed=0):
    """Uniform positions in the box, types cycling A, B, C. For the colloid in standard mode a particle with
    0 < d < a + 0.2 for any wall is drawn again until there is none (every particle stays in the comparison)."""
    key = (kind if (kind == "colloid" and not extrap) else "any", walls_key if (kind == "colloid" and not extrap) else "", n, seed)
    if key not in _positions:
        rng = np.random.default_rng(1000 * n + seed)
        pos = rng.uniform(-0.5 * L, 0.5 * L, (n, 3))
        tid = np.arange(n) % 3
        if key[0] == "colloid":
            a = np.array([p["a"] for p in type_params("colloid", False)])[tid]
            a[tid == 2] = -np.inf  # (the disabled type may sit anywhere)
            for _ in range(10000):
                bad = np.zeros(n, dtype=bool)
                for w in walls:
                    d = ref.distance(w, ref.wrap(pos, L))[0]
                    bad |= (d > 0.0) & (d < a + 0.2)
                if not bad.any():
                    break
                pos[bad] = rng.uniform(-0.5 * L, 0.5 * L, (int(bad.sum()), 3))
            assert not bad.any()
        _positions[key] = (pos, tid)
    return _positions[key]


def make_sim(pos, tid, forces, box=L, vel=None, dt=0.0, types=TYPES):
    snap = azp.Snapshot.from_arrays(pos, [box] * 3 if np.isscalar(box) else box, typeid=tid, types=types, velocity=vel)
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(snap)
    sim.operations.tuners.clear()  # keep the memory order: rows are compared by index
    sim.operations.integrator = azp.Integrator(dt=dt, forces=list(forces), methods=[azp.ConstantVolume()])
    return sim


def make_wall(kind, walls, params, mode):
    f = CLS[kind]([to_azp(w) for w in walls], mode=mode)
    for t, p in zip(TYPES, params):
        f.params[t] = p
    return f


def scale_of(F, E):
    return np.maximum(np.maximum(np.linalg.norm(F, axis=-1), np.abs(E)), 1e-3)


def assert_close(kind, got_F, got_E, want_F, want_E, scale, what=""):
    err = np.maximum(np.abs(got_F - want_F).max(axis=-1), np.abs(got_E - want_E)) / scale
    print("%s %s: worst deviation %.3e of the bound %.3e" % (kind, what, err.max() if err.size else 0.0, BOUND[kind]))
    assert np.all(np.isfinite(got_F)) and np.all(np.isfinite(got_E))
    assert np.all(err <= BOUND[kind]), (what, float(err.max()), int(err.argmax()))


# ---------------------------------------------------------------------------------------------------------------------
# 1. known answers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["none", "shift"])
@pytest.mark.parametrize("extrap", [False, True])
@pytest.mark.parametrize("kind", ["lj93", "colloid"])
def test_known_answers(kind, extrap, mode):
    """A plane at z = -5 with normal +z; the fixture's distances, a particle exactly at r_cut (exactly zero), one
    exactly at r_extrap (standard branch) and, extrapolated, one below r_extrap."""
    named, cut = CASES[kind]["named"], CASES[kind]["cut"]
    r_cut = cut["r"]
    e = named[1 if kind == "lj93" else 0]["r"] if extrap else 0.0  # LJ93: 1.5, colloid: 2.0 (fixture distances)
    shift = cut["E"] if mode == "shift" else 0.0
    p = {k: v for k, v in named[0].items() if k not in ("r", "E", "F")}
    p.update(r_cut=r_cut, r_extrap=e)
    d = [row["r"] for row in named] + [r_cut]
    want_E = [row["E"] - shift for row in named] + [0.0]
    want_F = [row["F"] for row in named] + [0.0]
    if extrap:
        at_e = next(row for row in named if row["r"] == e)
        for k, row in enumerate(named):
            if row["r"] < e:  # (LJ93 at 1.0 lies below r_extrap = 1.5)
                want_E[k], want_F[k] = at_e["E"] - shift + at_e["F"] * (e - row["r"]), at_e["F"]
        for below in (0.75, -1.0):  # below r_extrap (the colloid: inside its radius), and behind the wall
            d.append(below)
            want_E.append(at_e["E"] - shift + at_e["F"] * (e - below))
            want_F.append(at_e["F"])
    else:
        d.append(-1.0)  # behind the wall: nothing
        want_E.append(0.0)
        want_F.append(0.0)
    d = np.array(d)
    pos = np.stack([np.linspace(-3.0, 3.0, d.size), np.zeros(d.size), d - 5.0], axis=1)  # (d - 5) + 5 is exact here
    assert np.array_equal((pos[:, 2] + 5.0), d)
    wall = CLS[kind]([azp.wall.Plane(origin=(0, 0, -5), normal=(0, 0, 1))], mode=mode)
    wall.params["A"] = p
    sim = make_sim(pos, np.zeros(d.size, dtype=int), [wall], box=20.0, types=("A",))
    sim.run(0)
    F, E = wall.forces, wall.energies
    want_E, want_F = np.array(want_E), np.array(want_F)
    assert np.array_equal(F[:, :2], np.zeros((d.size, 2)))
    assert_close(kind, F[:, 2:], E, want_F[:, None], want_E, scale_of(want_F[:, None], want_E), "known answers")
    at_cut = list(d).index(r_cut)
    assert F[at_cut, 2] == 0.0 and E[at_cut] == 0.0
    if not extrap:
        assert F[-1, 2] == 0.0 and E[-1] == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# 2. random parity against wall_ref
# ---------------------------------------------------------------------------------------------------------------------
def _abi_forces(wall, st, block_size):
    import torch

    a = wall._args()
    out = torch.full((st.N, 4), float("nan"), dtype=torch.float64, device=st.device)
    a.d_force = out.data_ptr()
    a.block_size = block_size
    _lib.check(getattr(_lib.lib(), wall._entry)(C.byref(a), _lib.raw_stream(st.device)), wall._entry)
    return out.cpu().numpy()


@pytest.mark.parametrize("geometry", list(SINGLE))
@pytest.mark.parametrize("kind", ["lj93", "colloid"])
def test_random_parity(kind, geometry):
    w = SINGLE[geometry]
    for extrap in (False, True):
        params = type_params(kind, extrap)
        for n in (1, 63, 257, 1000):
            pos, tid = positions(kind, geometry, [w], n, extrap)
            for mode in ("none", "shift"):
                F, E, D = ref.evaluate(kind, [w], params, mode, pos, tid, L)
                wall = make_wall(kind, [w], params, mode)
                sim = make_sim(pos, tid, [wall])
                sim.run(0)
                got = np.c_[wall.forces, wall.energies]
                what = "%s extrap=%s N=%d %s" % (geometry, extrap, n, mode)
                assert_close(kind, got[:, :3], got[:, 3], F[0], E[0], scale_of(F[0], E[0]), what)
                # branches, on the reference
                c = np.array([p["r_cut"] for p in params])[tid]
                e = np.array([p["r_extrap"] for p in params])[tid]
                d = D[0]
                on = tid != 2
                linear = on & (e > 0.0) & (d < e)
                in_range = on & ~linear & (d > 0.0) & (d < c)
                out = ~(linear | in_range)
                assert np.array_equal(got[out], np.zeros((int(out.sum()), 4)))  # exact zeros out of range
                if n == 1000:
                    counts = dict(in_range=int(in_range.sum()), out_of_range=int((on & (d >= c)).sum()),
                                  behind=int((on & (d <= 0.0)).sum()))
                    if extrap:
                        counts["below_r_extrap"] = int(linear.sum())
                    print(what, counts)
                    assert min(counts.values()) >= 5, counts
                    assert np.abs(got[in_range | linear, :3]).max() > 0.0
                for bs in (64, 256):
                    assert np.array_equal(_abi_forces(wall, sim.state, bs), got), (what, bs)


TILTED = {
    "plane": dict(kind="plane", origin=(0.5, 0.2, -2.0), normal=(1.0, 2.0, 2.0)),
    "sphere": dict(kind="sphere", radius=3.0, origin=(0.3, -0.2, 0.1), inside=True),
    "cylinder": dict(kind="cylinder", radius=2.6, origin=(0.2, -0.3, 0.0), axis=(0.0, 0.0, 1.0), inside=True),
}


@pytest.mark.parametrize("geometry", list(TILTED))
@pytest.mark.parametrize("kind,extrap", [("lj93", False), ("colloid", True)])
def test_random_parity_tilted_box(kind, extrap, geometry):
    """The walls read the position after wrap_into_box: N = 4096 in the tilted box of tests/box_cases.py, positions scaled
    by 1.08 in fractional coordinates, so that about 8 % lie one image outside along each lattice direction and the wrap
    takes its tilted branches. Reference, bound and the net force on the wall as in test_random_parity and
    test_wall_forces."""
    Lt, tilt, periodic = box_cases.BOXES["tilt3"]
    n = 4096
    frac = np.random.default_rng(11).uniform(-0.5, 0.5, (n, 3)) * 1.08
    pos = frac @ box_ref.box_matrix(Lt, tilt).T
    tid = np.arange(n) % 3
    outside = np.abs(frac) >= 0.5
    assert np.all(outside.sum(axis=0) > 0.05 * n) and (outside.sum(axis=1) >= 2).sum() > 20
    # (no particle where the kernel's FMA and numpy's product and sum could decide differently)
    assert box_cases.face_distance(pos, Lt, tilt, periodic) > box_cases.FACE_MARGIN
    w = TILTED[geometry]
    params = type_params(kind, extrap)
    F, E, D = ref.evaluate(kind, [w], params, "shift", pos, tid, Lt, tilt=tilt)
    wall = make_wall(kind, [w], params, "shift")
    sim = make_sim(pos, tid, [wall], box=azp.Box(Lt[0], Lt[1], Lt[2], *tilt))
    sim.run(0)
    f, e = wall.forces, wall.energies
    scale = scale_of(F[0], E[0])
    assert_close(kind, f, e, F[0], E[0], scale, "%s in the tilted box" % geometry)
    felt = np.abs(E[0]) > 0.0
    assert felt.sum() > n // 20 and (felt & outside.any(axis=1)).sum() > 20, (int(felt.sum()), int((felt & outside.any(axis=1)).sum()))
    # the wrap matters to the answer: without it the particles outside get other forces
    F_far = ref.evaluate(kind, [w], params, "shift", pos, tid, Lt, tilt=tilt, periodic=(0, 0, 0))[0]
    assert (np.abs(F_far[0] - F[0]).max(axis=1) > 1e-6 * scale).sum() > 20
    # the net force on the wall: against the sum of the kernel's own rows (test_wall_forces) and of the reference's
    got = wall.wall_forces[0]
    total = float(np.linalg.norm(f, axis=1).sum())
    assert total > 0.0
    assert np.all(np.abs(got - [-math.fsum(f[:, c]) for c in range(3)]) <= BOUND[kind] * total), got
    assert np.all(np.abs(got - [-math.fsum(F[0][:, c]) for c in range(3)]) <= 2.0 * BOUND[kind] * float(scale.sum())), got


# ---------------------------------------------------------------------------------------------------------------------
# 3. several walls
# ---------------------------------------------------------------------------------------------------------------------
# (the colloid in standard mode is non-finite in the core 0 < d <= a: with 16 walls across the box no particle of radius
# 1.5 can be drawn outside every core, so the colloid meets the 16 walls in extrapolated mode and the slit in both)
@pytest.mark.parametrize("kind,extrap,walls_key", [("lj93", False, "slit"), ("lj93", True, "slit"), ("lj93", False, "all16"),
                                                   ("lj93", True, "all16"), ("colloid", False, "slit"), ("colloid", True, "slit"),
                                                   ("colloid", True, "all16")])
def test_several_walls(kind, extrap, walls_key):
    walls = NARROW_SLIT if walls_key == "slit" else ALL16  # (narrow: particles in the middle feel both planes)
    assert len(ALL16) == 16
    params = type_params(kind, extrap)
    pos, tid = positions(kind, walls_key, walls, 1000, extrap, seed=3)
    F, E, D = ref.evaluate(kind, walls, params, "shift", pos, tid, L)
    want_F, want_E = ref.total(F, E)
    wall = make_wall(kind, walls, params, "shift")
    sim = make_sim(pos, tid, [wall])
    sim.run(0)
    got = np.c_[wall.forces, wall.energies]
    scale = np.maximum(np.maximum(np.linalg.norm(F, axis=-1).sum(axis=0), np.abs(E).sum(axis=0)), 1e-3)
    assert_close(kind, got[:, :3], got[:, 3], want_F, want_E, scale, "%s extrap=%s" % (walls_key, extrap))
    assert (np.count_nonzero(E, axis=0) >= 2).sum() >= 5  # particles that feel more than one wall
    sim.run(0)
    assert np.array_equal(np.c_[wall.forces, wall.energies], got)  # bitwise


# ---------------------------------------------------------------------------------------------------------------------
# 4. in a force list
# ---------------------------------------------------------------------------------------------------------------------
def test_in_a_force_list_with_thermo():
    import torch

    cfg = syn.config_plj_sc(10)
    pos = cfg["xyz"][::2]  # every second site of the jittered lattice: 500 particles all over the box
    assert pos.shape[0] == 500
    box = cfg["L"]
    h = 0.5 * float(box[2])
    slit = [dict(kind="plane", origin=(0.0, 0.0, -h + 0.3), normal=(0.0, 0.0, 1.0)),
            dict(kind="plane", origin=(0.0, 0.0, h - 0.3), normal=(0.0, 0.0, -1.0))]
    params = [dict(epsilon=1.5, sigma=1.0, r_cut=2.5, r_extrap=0.7)]
    wall = azp.wall.LJ93([to_azp(w) for w in slit], mode="shift")
    wall.params["A"] = params[0]
    nl = azp.nlist.Cell(buffer=0.4)
    plj = azp.pair.PerturbedLennardJones(nlist=nl, default_r_cut=2.5, mode="shift")
    plj.params[("A", "A")] = cfg["params"]
    sim = make_sim(pos, np.zeros(500, dtype=int), [plj, wall], box=box, types=("A",))
    sim.run(0)
    assert torch.equal(sim.state.net_force, plj.force_tensor + wall.force_tensor)  # the azp_sum_forces path
    F, E, _ = ref.evaluate("lj93", slit, params, "shift", pos, np.zeros(500, dtype=int), box)
    want_F, want_E = ref.total(F, E)
    scale = np.maximum(np.maximum(np.linalg.norm(F, axis=-1).sum(axis=0), np.abs(E).sum(axis=0)), 1e-3)
    assert_close("lj93", wall.forces, wall.energies, want_F, want_E, scale, "force list")
    assert np.count_nonzero(want_E) > 50 and wall.virials is None
    thermo = azp.compute.ThermodynamicQuantities(azp.All())
    sim.operations.add(thermo)
    sim.run(0)
    wall._virial.fill_(7.0)  # the kernel call has to write the zeros, whatever the buffer held
    sim.run(0)
    assert wall.compute_virial and wall.virials.shape == (500, 6)
    assert np.array_equal(wall.virials, np.zeros((500, 6)))
    pe = thermo.potential_energy
    assert abs(wall.energy) > 1.0
    assert abs(pe - (plj.energy + wall.energy)) <= 1e-12 * (abs(plj.energy) + abs(wall.energy))
    assert np.isfinite(thermo.pressure)


# ---------------------------------------------------------------------------------------------------------------------
# 5. NVE in a slit
# ---------------------------------------------------------------------------------------------------------------------
def test_nve_in_a_slit():
    """64 non-interacting particles between two LJ93 planes, velocities along the normal: positions and velocities
    after 200 steps against a NumPy velocity Verlet on wall_ref. 1e-9 is a cap, not a measurement: a wrong sign, a
    missing wall or a wrong branch is off by O(1); the bound only has to absorb rounding amplified at the turning
    points."""
    rng = np.random.default_rng(5)
    n, dt, steps = 64, 0.002, 200
    pos = np.stack([rng.uniform(-5, 5, n), rng.uniform(-5, 5, n), rng.uniform(-3.0, 3.0, n)], axis=1)
    vel = np.zeros((n, 3))
    vel[:, 2] = rng.uniform(3.0, 6.0, n) * rng.choice([-1.0, 1.0], n)  # (0.4 time units: up to 2.4 lengths)
    params = [dict(epsilon=1.0, sigma=1.0, r_cut=2.5, r_extrap=0.0)]
    wall = azp.wall.LJ93([to_azp(w) for w in SLIT], mode="shift")
    wall.params["A"] = params[0]
    tid = np.zeros(n, dtype=int)
    sim = make_sim(pos, tid, [wall], vel=vel, dt=dt, types=("A",))
    sim.run(steps)

    def force(x):
        F, E, _ = ref.evaluate("lj93", SLIT, params, "shift", x, tid, L)
        return ref.total(F, E)[0]

    x, v = pos.copy(), vel.copy()
    f = force(x)
    turned = np.zeros(n, dtype=bool)
    for _ in range(steps):
        v = v + 0.5 * dt * f  # (mass 1)
        x = ref.wrap(x + dt * v, L)
        f = force(x)
        v_new = v + 0.5 * dt * f
        turned |= np.sign(v_new[:, 2]) != np.sign(vel[:, 2])
        v = v_new
    assert turned.sum() >= 5  # particles did bounce off the walls
    got_x = sim.state.pos[:, :3].cpu().numpy()
    got_v = sim.state.vel[:, :3].cpu().numpy()
    print("NVE slit: |dx| %.3e |dv| %.3e" % (np.abs(got_x - x).max(), np.abs(got_v - v).max()))
    assert np.abs(got_x - x).max() < 1e-9 and np.abs(got_v - v).max() < 1e-9
    assert np.array_equal(got_x[:, :2], pos[:, :2])


# ---------------------------------------------------------------------------------------------------------------------
# 6. type changes
# ---------------------------------------------------------------------------------------------------------------------
def test_type_changes_take_the_new_rows():
    pos, _ = positions("lj93", "", [], 257, True)
    w = SINGLE["sphere_in"]
    params = type_params("lj93", False)
    wall = make_wall("lj93", [w], params, "shift")
    tid = np.zeros(257, dtype=int)
    sim = make_sim(pos, tid, [wall])
    sim.run(0)
    F, E, _ = ref.evaluate("lj93", [w], params, "shift", pos, tid, L)
    assert_close("lj93", wall.forces, wall.energies, F[0], E[0], scale_of(F[0], E[0]), "before the update")
    sim.operations.updaters.append(azp.update.TypeUpdater(trigger=1, inside_type="B", outside_type="A", lo=-2.0, hi=3.0))
    sim.run(1)  # dt = 0: nothing moves, the updater flips the types, the forces are evaluated again
    new_tid = np.where((pos[:, 2] >= -2.0) & (pos[:, 2] <= 3.0), 1, 0)
    assert np.array_equal(sim.state.typeid_host, new_tid) and 50 < new_tid.sum() < 200
    F2, E2, _ = ref.evaluate("lj93", [w], params, "shift", pos, new_tid, L)
    assert_close("lj93", wall.forces, wall.energies, F2[0], E2[0], scale_of(F2[0], E2[0]), "after the update")
    assert np.abs(E2[0] - E[0]).max() > 1e-3  # the rows differ where it matters


# ---------------------------------------------------------------------------------------------------------------------
# 7. wall_forces
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,extrap", [("lj93", False), ("colloid", True)])
def test_wall_forces(kind, extrap):
    import torch

    walls = list(SINGLE.values()) + SLIT[1:]
    params = type_params(kind, extrap)
    pos, tid = positions(kind, "", walls, 1000, extrap, seed=7)
    wall = make_wall(kind, walls, params, "shift")
    sim = make_sim(pos, tid, [wall])
    sim.run(0)
    got = wall.wall_forces
    assert got.shape == (len(walls), 3)
    energies = []
    for k, w in enumerate(walls):
        one = make_wall(kind, [w], params, "shift")
        sim1 = make_sim(pos, tid, [one])
        sim1.run(0)
        f, e = one.forces, one.energies
        want = [-math.fsum(f[:, c]) for c in range(3)]
        total = float(np.linalg.norm(f, axis=1).sum())
        assert total > 0.0
        assert np.all(np.abs(got[k] - want) <= BOUND[kind] * total), (k, got[k], want)
        energies.append((math.fsum(e), max(float(np.abs(e).sum()), 1e-3)))
        assert np.array_equal(one.wall_forces[0], got[k])  # the same particles in the same order: the same bits
    assert np.array_equal(wall.wall_forces, got)  # bitwise, two calls
    # too small a scratch is an argument error, not a fault
    st = sim.state
    a = wall._args()
    need = C.c_uint64(0)
    _lib.check(_lib.lib().azp_wall_net_forces_scratch_size(C.byref(a), C.byref(need)), "scratch size")
    assert need.value == 4 * len(walls) * 8 * 4
    out = torch.zeros((len(walls), 4), dtype=torch.float64, device=st.device)
    scratch = torch.zeros(int(need.value), dtype=torch.uint8, device=st.device)
    fn = getattr(_lib.lib(), wall._net_entry)
    stream = _lib.raw_stream(st.device)
    assert fn(C.byref(a), out.data_ptr(), scratch.data_ptr(), need.value - 1, stream) == -1
    assert fn(C.byref(a), out.data_ptr(), None, need.value, stream) == -1
    assert fn(C.byref(a), out.data_ptr(), scratch.data_ptr(), need.value, stream) == 0
    rows = out.cpu().numpy()
    assert np.array_equal(rows[:, :3], got)
    for k, (want_e, total_e) in enumerate(energies):  # the fourth column: the energy of each wall
        assert abs(rows[k, 3] - want_e) <= BOUND[kind] * total_e


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("kind,extrap,n,geometries", [("lj93", False, 1000, "all"), ("colloid", True, 1000, "all"),
                                                      ("lj93", False, 20000, "all"), ("colloid", True, 20000, "all"),
                                                      ("lj93", False, 524289, "plane_z")])
def test_wall_forces_order_bit_for_bit(kind, extrap, n, geometries):
    """One wall at a time: its net force and energy are the documented tree (csrc/azp_reduce.hpp, restated in
    tests/reduction_ref.py) over the per-particle forces and energies of that wall, in every bit -- wall_term gives the
    same bits in both kernels, as the single-wall assertion of test_wall_forces already assumes. 1,000 particles: 4
    partials; 20,000: 79, a second trip of the fold's lanes; 524,289: two particles per lane in the wall's own loop."""
    params = type_params(kind, extrap)
    pos, tid = positions(kind, "", [], n, extrap, seed=11)
    for g in (list(SINGLE) if geometries == "all" else [geometries]):
        one = make_wall(kind, [SINGLE[g]], params, "shift")
        sim = make_sim(pos, tid, [one])
        sim.run(0)
        f, e = one.forces, one.energies
        got_f = one.wall_forces[0]
        got_e = one._net[0][0, 3].item()  # the row the call left behind: force on the wall, then its energy
        want_f = -red.tree_sum(f.T)
        want_e = red.tree_sum(e)
        print("%s %s N=%d: %r %r | tree %r %r" % (kind, g, n, got_f.tolist(), got_e, want_f.tolist(), float(want_e)))
        assert np.count_nonzero(e) >= n // 100
        assert np.array_equal(_bits(got_f), _bits(want_f)), g
        assert _bits(got_e) == _bits(want_e), g
