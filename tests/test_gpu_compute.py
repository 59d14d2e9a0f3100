"""azplugins_amd.compute on the GPU (csrc/velocity_field.hip): the reference's known answers
(tests/golden/compute_cases.json), forty seeded random systems against the numpy reference
(tests/velocity_field_ref.py), field shapes up to more bins than one tile holds, bit-identical repeated calls (also at
N = 2^20), invariance under a particle sort, bins and bounds changed after attach, and a decomposed run on two ranks
(every rank gets the same result, computed from its owned rows only)."""

import json
import os
import socket

import numpy as np
import pytest

import velocity_field_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12


@pytest.fixture(scope="module")
def cases():
    with open(os.path.join(ROOT, "tests", "golden", "compute_cases.json")) as f:
        return json.load(f)


def _sim(xyz, vel, mass, box, typeid=None, types=("A",)):
    import azplugins_amd as azp

    snap = azp.Snapshot.from_arrays(np.asarray(xyz, dtype=np.float64).reshape(-1, 3), box, typeid=typeid, types=types,
                                    velocity=np.asarray(vel, dtype=np.float64).reshape(-1, 3))
    snap.particles.mass[:] = np.asarray(mass, dtype=np.float64)
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(snap)
    return sim


def _field(cls_name, num_bins, lower, upper, filter):
    from azplugins_amd import compute

    cls = compute.CartesianVelocityFieldCompute if cls_name == "Cartesian" else compute.CylindricalVelocityFieldCompute
    return cls(num_bins=num_bins, lower_bounds=lower, upper_bounds=upper, filter=filter)


def _check(got, want, step):
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    if step.get("exact"):
        np.testing.assert_equal(got, want)
    else:
        np.testing.assert_allclose(got, want, atol=step.get("atol", 0.0))


# ---------------------------------------------------------------------------------------------------------------------
# 1. golden cases
# ---------------------------------------------------------------------------------------------------------------------
def test_golden_velocity_compute(cases):
    import azplugins_amd as azp
    from azplugins_amd import compute

    c = cases["velocity_compute"]
    sim = _sim(c["position"], c["velocity"], c["mass"], azp.Box.cube(c["L"]), typeid=c["typeid"], types=c["types"])
    for chk in c["checks"]:
        flt = azp.All() if chk["filter"] == "All" else azp.Type(chk["filter"])
        v = compute.VelocityCompute(filter=flt)
        sim.operations.add(v)
        got = v.velocity
        assert isinstance(got, tuple) and len(got) == 3
        np.testing.assert_allclose(got, chk["velocity"])
    # no filter: no particles
    v0 = compute.VelocityCompute()
    sim.operations.add(v0)
    np.testing.assert_equal(v0.velocity, [0, 0, 0])
    sim.operations.remove(v0)
    with pytest.raises(compute.DataAccessError):
        v0.velocity


@pytest.mark.parametrize("name", ["cartesian_basic", "cylindrical_basic"])
def test_golden_basic(cases, name):
    """Test 1 and 6: the reference's steps set num_bins and the bounds after attach."""
    import azplugins_amd as azp

    c = cases[name]
    sim = _sim(c["position"], c["velocity"], c["mass"], azp.Box.cube(c["L"]))
    first = c["steps"][0]
    f = _field(c["cls"], first["num_bins"], first["lower"], first["upper"], azp.All())
    sim.operations.add(f)
    for step in c["steps"]:
        if "num_bins" in step:
            f.num_bins = step["num_bins"]
        if "lower" in step:
            f.lower_bounds = step["lower"]
        if "upper" in step:
            f.upper_bounds = step["upper"]
        _check(f.velocities, step["velocities"], step)


def test_golden_no_particles(cases):
    import azplugins_amd as azp

    for c in cases["no_particles"]:
        s = cases[c["snapshot"]]
        sim = _sim(s["position"], s["velocity"], s["mass"], azp.Box.cube(s["L"]))
        f = _field(c["cls"], c["num_bins"], c["lower"], c["upper"], None)
        sim.operations.add(f)
        np.testing.assert_equal(f.velocities, c["velocities"])


def test_golden_binning_shape(cases):
    import azplugins_amd as azp

    for c in cases["binning_shape"]:
        sim = _sim([[-0.5, 0, 0], [0.5, 0, 0]], np.zeros((2, 3)), [1, 1], azp.Box.cube(c["L"]))
        f = _field(c["cls"], [2, 3, 4], c["lower"], c["upper"], None)
        sim.operations.add(f)
        for step in c["steps"]:
            f.num_bins = step["num_bins"]
            assert list(f.velocities.shape) == step["velocities_shape"]
            if step["coordinates"] is None:
                assert f.coordinates is None
            else:
                np.testing.assert_allclose(f.coordinates, step["coordinates"])


# ---------------------------------------------------------------------------------------------------------------------
# 2. seeded random systems against the numpy reference
# ---------------------------------------------------------------------------------------------------------------------
def _random_system(seed):
    import azplugins_amd as azp

    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(300, 3000))
    L = rng.uniform(8.0, 14.0, 3)
    tilt = (0.0, 0.0, 0.0)
    periodic = [True, True, True]
    kind = seed % 4
    if kind == 1:
        tilt = tuple(rng.uniform(-0.3, 0.3, 3))
    if kind == 2:
        periodic[int(rng.integers(0, 3))] = False
    cylindrical = (seed // 4) % 2 == 1  # (each of the four box kinds with both coordinate systems)
    # fractional positions in the box, a tenth of them one box length outside along a periodic axis
    f = rng.uniform(-0.5, 0.5, (n, 3))
    xy, xz, yz = tilt
    xyz = np.stack([f[:, 0] * L[0] + f[:, 1] * L[1] * xy + f[:, 2] * L[2] * xz, f[:, 1] * L[1] + f[:, 2] * L[2] * yz,
                    f[:, 2] * L[2]], axis=1)
    out = rng.random(n) < 0.1
    out[:20] = False  # (the edge particles placed below stay where they are put)
    ax = int(np.flatnonzero(periodic)[0])
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    lattice = np.array([[L[0], 0, 0], [L[1] * xy, L[1], 0], [L[2] * xz, L[2] * yz, L[2]]])
    xyz[out] += sign[out, None] * lattice[ax]
    num_bins = [int(rng.integers(0, 7)) for _ in range(3)]
    if cylindrical:
        lower = [0.0, 0.0, -0.4 * L[2]]
        upper = [0.5 * min(L[0], L[1]), 2.0 * np.pi if seed % 3 else 1.5 * np.pi, 0.4 * L[2]]
    else:
        lower = [-0.4 * L[0], -0.45 * L[1], -0.3 * L[2]]
        upper = [0.4 * L[0], 0.45 * L[1], 0.5 * L[2]]
    if kind == 0:
        # bins with exact edges (integer bounds, a power-of-two bin count), particles placed on lower and upper edges
        nb = 4
        num_bins[0] = nb
        lower[0], upper[0] = (0.0, 4.0) if cylindrical else (-4.0, 4.0)
        edges = lower[0] + np.arange(nb + 1) * (upper[0] - lower[0]) / nb
        k = np.arange(min(n, 3 * (nb + 1)))
        xyz[k, 0] = edges[k % (nb + 1)]
        xyz[k, 1] = 0.0  # (on the x axis: r = |x|, theta = 0 or pi)
        if cylindrical:
            xyz[k, 0] = np.abs(xyz[k, 0])
        xyz[k[-1] + 1, :2] = 0.0  # r = 0 exactly
    vel = rng.normal(0.0, 1.0, (n, 3))
    mass = rng.uniform(0.5, 3.0, n)
    typeid = rng.integers(0, 3, n)
    if cylindrical and num_bins[1] > 0:
        # keep particles more than 1e-9 away from theta bin edges (atan2 may differ by an ulp between device and numpy);
        # theta = 0 exactly (the x axis, r >= 0) is exact on both
        wr = ref.wrap(xyz, L, tilt, periodic)
        th = np.arctan2(wr[:, 1], wr[:, 0])
        th = np.where(th < 0, th + 2 * np.pi, th)
        w = (upper[1] - lower[1]) / num_bins[1]
        d = np.abs((th - lower[1]) / w - np.round((th - lower[1]) / w)) * w
        keep = (d > 1e-9) | (th == 0.0)
        xyz, vel, mass, typeid = xyz[keep], vel[keep], mass[keep], typeid[keep]
    box = azp.Box(L[0], L[1], L[2], *tilt, periodic=periodic)
    return dict(xyz=xyz, vel=vel, mass=mass, typeid=typeid, box=box, L=L, tilt=tilt, periodic=periodic, num_bins=num_bins,
                lower=lower, upper=upper, cylindrical=cylindrical, types_filter=(seed % 3 == 0))


def _reference(sysd, include):
    s, scale = ref.sums(sysd["xyz"], sysd["vel"], sysd["mass"], sysd["num_bins"], sysd["lower"], sysd["upper"],
                        cylindrical=sysd["cylindrical"], L=sysd["L"], tilt=sysd["tilt"], periodic=sysd["periodic"], include=include)
    return s, scale


def _assert_close(got, s, scale):
    """|delta p| <= 1e-12 sum|m v| per bin, compared as velocities (bins without mass: exactly 0)."""
    want = ref.normalize(s)
    got = got.reshape(-1, 3)
    m = s[:, 0]
    empty = m == 0
    np.testing.assert_equal(got[empty], 0.0)
    err = np.abs(got[~empty] - want[~empty]) * m[~empty, None]
    assert np.all(err <= TOL * scale[~empty, None] + 1e-300), err.max()


@pytest.mark.parametrize("seed", range(40))
def test_random_systems(seed):
    import azplugins_amd as azp

    sysd = _random_system(seed)
    types = ("A", "B", "C")
    sim = _sim(sysd["xyz"], sysd["vel"], sysd["mass"], sysd["box"], typeid=sysd["typeid"], types=types)
    flt = azp.Type(["A", "C"]) if sysd["types_filter"] else azp.All()
    include = np.isin(sysd["typeid"], [0, 2]) if sysd["types_filter"] else None
    f = _field("Cylindrical" if sysd["cylindrical"] else "Cartesian", sysd["num_bins"], sysd["lower"], sysd["upper"], flt)
    sim.operations.add(f)
    got = f.velocities
    assert got.shape == ref.compact_shape(sysd["num_bins"])
    s, scale = _reference(sysd, include)
    _assert_close(got, s, scale)
    np.testing.assert_array_equal(f.velocities, got)  # 4. bit-identical repeat


# ---------------------------------------------------------------------------------------------------------------------
# 3. field shapes, more bins than one tile
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_bins", [(0, 0, 0), (7, 0, 0), (0, 13, 9), (5, 6, 7), (128, 128, 4)])
@pytest.mark.parametrize("cls", ["Cartesian", "Cylindrical"])
def test_field_shapes(num_bins, cls):
    import azplugins_amd as azp

    rng = np.random.default_rng(7)
    n = 20000
    L = np.array([12.0, 12.0, 12.0])
    xyz = rng.uniform(-6.0, 6.0, (n, 3))
    vel = rng.normal(size=(n, 3))
    mass = rng.uniform(0.5, 3.0, n)
    lower, upper = ((-6, -6, -6), (6, 6, 6)) if cls == "Cartesian" else ((0, 0, -6), (6, 2 * np.pi, 6))
    sim = _sim(xyz, vel, mass, azp.Box.cube(12.0))
    f = _field(cls, num_bins, lower, upper, azp.All())
    sim.operations.add(f)
    got = f.velocities
    assert got.shape == ref.compact_shape(num_bins)
    s, scale = ref.sums(xyz, vel, mass, num_bins, lower, upper, cylindrical=cls == "Cylindrical", L=L)
    _assert_close(got, s, scale)


# ---------------------------------------------------------------------------------------------------------------------
# 4. bit-identical at N = 2^20 (north-star lattice, 100-bin profile), 5. particle sort
# ---------------------------------------------------------------------------------------------------------------------
def test_north_star_profile_deterministic():
    import azplugins_amd as azp
    from azplugins_amd import compute
    from azplugins_amd import synthetic as syn

    cfg = syn.config_north_star()
    n = cfg["xyz"].shape[0]
    assert n == 2**20
    tag = np.arange(n, dtype=np.uint64)
    vel = np.stack([syn.normal(11, tag, c) for c in range(3)], axis=1)
    vel[:, 1] += 0.1 * np.sin(2 * np.pi * cfg["xyz"][:, 0] / cfg["L"][0])
    mass = 1.0 + syn.u01(12, tag, 0)
    sim = _sim(cfg["xyz"], vel, mass, azp.Box(*cfg["L"]))
    L = cfg["L"]
    f = compute.CartesianVelocityFieldCompute(num_bins=(100, 0, 0), lower_bounds=(-L[0] / 2, 0, 0), upper_bounds=(L[0] / 2, 0, 0),
                                              filter=azp.All())
    v_cm = compute.VelocityCompute(filter=azp.All())
    sim.operations.computes.extend([f, v_cm])
    a, b = f.velocities, f.velocities
    assert np.array_equal(a, b)
    c1, c2 = v_cm.velocity, v_cm.velocity
    assert c1 == c2
    s, scale = ref.sums(cfg["xyz"], vel, mass, (100, 0, 0), (-L[0] / 2, 0, 0), (L[0] / 2, 0, 0), L=L)
    _assert_close(a, s, scale)
    s1, scale1 = ref.sums(cfg["xyz"], vel, mass, (0, 0, 0), L=L)
    _assert_close(np.array(c1), s1, scale1)

    # a particle sort reorders every row: the result moves by rounding only
    azp.ParticleSorter().sort(sim)
    _assert_close(f.velocities, s, scale)
    _assert_close(np.array(v_cm.velocity), s1, scale1)


@pytest.mark.parametrize("cls", ["Cartesian", "Cylindrical"])
def test_sorted_equals_unsorted(cls):
    import azplugins_amd as azp

    rng = np.random.default_rng(3)
    n = 50000
    xyz = rng.uniform(-10.0, 10.0, (n, 3))
    vel = rng.normal(size=(n, 3))
    mass = rng.uniform(0.5, 3.0, n)
    lower, upper = ((-10, -10, 0), (10, 10, 0)) if cls == "Cartesian" else ((0, 0, -10), (10, 2 * np.pi, 10))
    nb = (40, 40, 0) if cls == "Cartesian" else (10, 8, 5)
    sim = _sim(xyz, vel, mass, azp.Box.cube(20.0))
    f = _field(cls, nb, lower, upper, azp.All())
    sim.operations.add(f)
    before = f.velocities
    azp.ParticleSorter().sort(sim)
    after = f.velocities
    s, scale = ref.sums(xyz, vel, mass, nb, lower, upper, cylindrical=cls == "Cylindrical", L=(20.0, 20.0, 20.0))
    _assert_close(before, s, scale)
    _assert_close(after, s, scale)


def test_resize_after_attach():
    """6. num_bins and bounds set after attach: the shape and the values follow, the buffers are resized."""
    import azplugins_amd as azp

    rng = np.random.default_rng(5)
    n = 5000
    xyz = rng.uniform(-5.0, 5.0, (n, 3))
    vel = rng.normal(size=(n, 3))
    mass = np.ones(n)
    sim = _sim(xyz, vel, mass, azp.Box.cube(10.0))
    f = _field("Cartesian", (2, 0, 0), (-5, -5, -5), (5, 5, 5), azp.All())
    sim.operations.add(f)
    for nb, lo, hi in (((2, 0, 0), (-5, -5, -5), (5, 5, 5)), ((128, 128, 4), (-5, -5, -5), (5, 5, 5)), ((3, 1, 0), (-1, -2, 0), (1, 2, 0)),
                       ((0, 0, 0), (0, 0, 0), (0, 0, 0))):
        f.num_bins, f.lower_bounds, f.upper_bounds = nb, lo, hi
        got = f.velocities
        assert got.shape == ref.compact_shape(nb)
        s, scale = ref.sums(xyz, vel, mass, nb, lo, hi, L=(10.0, 10.0, 10.0))
        _assert_close(got, s, scale)


# ---------------------------------------------------------------------------------------------------------------------
# 7. decomposed run: two ranks on one GPU, gloo
# ---------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dd_config():
    from azplugins_amd import synthetic as syn

    cfg = syn.config_plj_sc(16)
    n = cfg["xyz"].shape[0]
    tag = np.arange(n, dtype=np.uint64)
    v = np.stack([syn.normal(81, tag, c) for c in range(3)], axis=1) * np.sqrt(1.5)
    cfg["vel"] = v - v.mean(axis=0) + np.array([0.5, 0.0, 0.0])
    cfg["steps"] = 100
    cfg["dt"] = 0.005
    return cfg


def _dd_fields(L):
    return dict(cart=("Cartesian", (6, 4, 0), (-L[0] / 2, -L[1] / 2, 0), (L[0] / 2, L[1] / 2, 0)),
                cyl=("Cylindrical", (4, 6, 3), (0, 0, -L[2] / 2), (L[0] / 2, 2 * np.pi, L[2] / 2)))


def _dd_worker(rank, world, port, out_dir):
    import torch
    import torch.distributed as dist

    import azplugins_amd as azp
    from azplugins_amd import compute
    from azplugins_amd import decomposition as dd

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    cfg = _dd_config()
    dec = dd.Decomposition(cfg["L"], world, cfg["r_cut"] + cfg["r_buff"])
    sim, dom = dd.rank_simulation(cfg, dec, rank, "cuda:0", seed=1)
    nl = azp.nlist.Cell(buffer=cfg["r_buff"])
    pot = azp.pair.PerturbedLennardJones(nlist=nl, default_r_cut=cfg["r_cut"], mode="shift")
    pot.params[("A", "A")] = cfg["params"]
    sim.operations.integrator = azp.Integrator(dt=cfg["dt"], forces=[pot], methods=[azp.ConstantVolume()])
    sim.run(cfg["steps"])
    v_cm = compute.VelocityCompute(filter=azp.All())
    sim.operations.add(v_cm)
    out = dict(v_cm=np.array(v_cm.velocity))
    for key, (cls, nb, lo, hi) in _dd_fields(cfg["L"]).items():
        f = _field(cls, nb, lo, hi, azp.All())
        sim.operations.add(f)
        out[key] = f.velocities
    torch.cuda.synchronize()
    st = sim.state
    N = st.N
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), tag=st.tag[:N].cpu().numpy().view(np.uint32), pos=st.pos[:N, :3].cpu().numpy(),
             vel=st.vel[:N].cpu().numpy(), n_ghost=np.array([st.n_ghost]), rebuilds=np.array([dom.num_rebuilds]),
             migrated=np.array([dom.num_migrated]), **out)
    dist.barrier()
    dist.destroy_process_group()


def test_decomposed_run():
    import torch.multiprocessing as mp

    import tempfile

    world = 2
    cfg = _dd_config()
    n = cfg["xyz"].shape[0]
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_dd_worker, args=(world, _free_port(), d), nprocs=world, join=True)
        res = [dict(np.load(os.path.join(d, "rank%d.npz" % r))) for r in range(world)]
    for key in ("v_cm", "cart", "cyl"):
        assert np.array_equal(res[0][key], res[1][key]), key
    assert sum(int(r["n_ghost"][0]) for r in res) > 0  # (ghost rows exist and must not be counted)
    assert sum(int(r["migrated"][0]) for r in res) > 0  # particles changed ranks during the run
    tags = np.concatenate([r["tag"] for r in res]).astype(np.int64)
    assert tags.size == n and np.array_equal(np.sort(tags), np.arange(n))
    pos = np.concatenate([r["pos"] for r in res])
    vel4 = np.concatenate([r["vel"] for r in res])
    L = cfg["L"]
    s, scale = ref.sums(pos, vel4[:, :3], vel4[:, 3], (0, 0, 0), L=L)
    _assert_close(res[0]["v_cm"], s, scale)
    for key, (cls, nb, lo, hi) in _dd_fields(L).items():
        s, scale = ref.sums(pos, vel4[:, :3], vel4[:, 3], nb, lo, hi, cylindrical=cls == "Cylindrical", L=L)
        _assert_close(res[0][key], s, scale)
