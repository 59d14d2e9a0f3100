"""minimize.FIRE on the GPU (csrc/fire.hip) against tests/fire_ref.py: the measure pass, step two with partials and step
one bit for bit through the C ABI, the advance over a grid of states and sums, a driven trajectory on a harmonic well, and
minimizations of Lennard-Jones dimers and of bonded chains through ``Simulation.run``."""

import ctypes as C
import itertools
import math

import numpy as np
import pytest

import fire_ref as ref
from azplugins_amd import _lib

pytestmark = pytest.mark.gpu

# 63 * 256 to 64 * 256 + 1: 63, 64 and 65 partials, the fold's step from one round of a wave to two; the last: two
# particles per lane, 1025 partials per slot
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 63 * 256, 64 * 256, 64 * 256 + 1, 2048 * 256 + 1]
L_BOX = (6.0, 7.0, 8.0)
PARAMS = dict(dt_max=0.05, force_tol=1e-3, energy_tol=1e-7, finc_dt=1.1, fdec_dt=0.5, alpha_start=0.1, fdec_alpha=0.99,
              min_steps_adapt=5, min_steps_conv=10)


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _stream():
    return _lib.raw_stream("cuda:0")


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def _call(name, a):
    _lib.check(getattr(_lib.lib(), name)(C.byref(a), _stream()), name)


def _ref_params(p):
    """The keyword arguments of ``ref.advance`` behind the constants of an argument struct."""
    return dict(dt_max=p["dt_max"], force_tol=p["force_tol"], energy_tol=p["energy_tol"], min_steps_adapt=p["min_steps_adapt"],
                finc_dt=p["finc_dt"], fdec_dt=p["fdec_dt"], alpha_start=p["alpha_start"], fdec_alpha=p["fdec_alpha"],
                min_steps_conv=p["min_steps_conv"])


def _set_params(a, p):
    for k, v in p.items():
        setattr(a, k, v)


class _Particles:
    """Host arrays and their device copies behind one azp_fire_args."""

    def __init__(self, N, seed, v_scale=1.0, L=L_BOX, pos=None, force_scale=5.0):
        import torch

        rng = np.random.default_rng(seed)
        self.L = np.asarray(L, dtype=np.float64)
        self.N = N
        self.pos = rng.uniform(-0.5, 0.5, (N, 3)) * self.L if pos is None else np.array(pos, dtype=np.float64)
        self.vel = rng.normal(0.0, v_scale, (N, 3))
        self.mass = rng.uniform(0.5, 2.0, N)
        self.force = rng.normal(0.0, force_scale, (N, 3))
        self.energy = rng.normal(size=N)
        self.image = rng.integers(-3, 4, (N, 3)).astype(np.int32)
        self.type_w = rng.integers(0, 3, N).astype(np.int64).view(np.float64)
        self.d_pos = _dev(np.c_[self.pos, self.type_w])
        self.d_vel = _dev(np.c_[self.vel, self.mass])
        self.d_force = _dev(np.c_[self.force, self.energy])
        self.d_image = _dev(self.image)
        need = C.c_uint64(0)
        _lib.check(_lib.lib().azp_fire_partials_size(N, C.byref(need)))
        self.d_partials = torch.full((need.value // 8,), float("nan"), dtype=torch.float64, device="cuda:0")
        self.d_state = torch.zeros(_lib.FIRE_NSTATE, dtype=torch.float64, device="cuda:0")

    def args(self, **params):
        a = _lib.FireArgs()
        a.d_pos, a.d_vel, a.d_net_force = self.d_pos.data_ptr(), self.d_vel.data_ptr(), self.d_force.data_ptr()
        a.d_image = self.d_image.data_ptr()
        a.d_partials, a.partials_bytes = self.d_partials.data_ptr(), self.d_partials.numel() * 8
        a.d_state = self.d_state.data_ptr()
        a.box = _lib.make_box(tuple(self.L))
        _set_params(a, dict(PARAMS, **params))
        a.N = self.N
        return a

    def set_state(self, state):
        self.d_state.copy_(_dev(ref.to_array(state)))

    def state(self):
        return self.d_state.cpu().numpy()


def _assert_state(got, want, what=""):
    """Every slot bit for bit (MIX too: ADVANCE_REL is measured 0); the unused slots stay 0."""
    want = ref.to_array(want)
    for k, name in enumerate(ref.SLOTS):
        if name == "mix" and ref.ADVANCE_REL > 0.0:
            assert abs(got[k] - want[k]) <= ref.ADVANCE_REL * abs(want[k]), (what, name, got[k], want[k])
        else:
            assert _bits(got[k]) == _bits(want[k]), (what, name, got[k], want[k])
    assert not np.any(got[len(ref.SLOTS):])


# ---------------------------------------------------------------------------------------------------------------------
# 1. the measure pass and step two with partials, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
def test_measure_and_step_two(N):
    p = _Particles(N, seed=1000 + N % 97)
    a = p.args()
    s0 = dict(ref.new_state(0.05), dt=0.01)
    p.set_state(s0)
    _call("azp_fire_measure", a)
    _call("azp_fire_advance", a)  # (the fold: the four sums land in the state)
    got = p.state()
    np.testing.assert_array_equal(_bits(p.d_vel.cpu().numpy()), _bits(np.c_[p.vel, p.mass]))  # the measure pass writes no velocity
    sums0 = ref.measure(p.vel, p.force, p.energy)
    for k, name in enumerate(("P", "VV", "FF", "U")):
        assert _bits(got[getattr(_lib, "FIRE_" + name)]) == _bits(sums0[k]), (name, got[getattr(_lib, "FIRE_" + name)], sums0[k])
    _assert_state(got, ref.advance(sums0, s0, N, **_ref_params(PARAMS)), "after the measure pass")
    # step two with the DT the test sets
    s1 = dict(ref.new_state(0.05), dt=0.02)
    p.set_state(s1)
    _call("azp_fire_step_two", a)
    _call("azp_fire_advance", a)
    got_v = p.d_vel.cpu().numpy()
    v1, sums1 = ref.step_two(p.vel, p.mass, p.force, p.energy, s1)
    np.testing.assert_array_equal(_bits(got_v[:, :3]), _bits(v1))
    np.testing.assert_array_equal(_bits(got_v[:, 3]), _bits(p.mass))
    _assert_state(p.state(), ref.advance(sums1, s1, N, **_ref_params(PARAMS)), "after step two")
    assert sums1[0] != sums0[0] and sums1[1] != sums0[1] and sums1[2] == sums0[2] and sums1[3] == sums0[3]
    # a measure pass after step two leaves the partials that step two left
    left = p.d_partials.clone()
    _call("azp_fire_measure", a)
    np.testing.assert_array_equal(_bits(p.d_partials.cpu().numpy()), _bits(left.cpu().numpy()))
    # a flag set: step two neither moves a velocity nor writes a partial
    for flag in ("converged", "nonfinite"):
        p.set_state(dict(s1, **{flag: 1.0}))
        p.d_partials.fill_(-7.0)
        _call("azp_fire_step_two", a)
        np.testing.assert_array_equal(_bits(p.d_vel.cpu().numpy()), _bits(got_v))
        assert bool((p.d_partials == -7.0).all())


# ---------------------------------------------------------------------------------------------------------------------
# 2. step one, bit for bit, with the coefficients the test writes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
def test_step_one(N):
    # velocities of scale 8 and DT = 0.05: |v| dt ~ 0.4 in a box of edges 6 to 8, a few percent cross a periodic face
    p = _Particles(N, seed=2000 + N % 97, v_scale=8.0)
    a = p.args()
    s = dict(ref.new_state(0.05), keep=0.9, mix=0.03, dt=0.05)
    before = [t.clone() for t in (p.d_pos, p.d_vel, p.d_image)]
    for flag in ("converged", "nonfinite"):
        p.set_state(dict(s, **{flag: 1.0}))
        _call("azp_fire_step_one", a)
        for t, b in zip((p.d_pos, p.d_vel, p.d_image), before):
            np.testing.assert_array_equal(t.cpu().numpy().view(np.int32), b.cpu().numpy().view(np.int32))
    p.set_state(s)
    _call("azp_fire_step_one", a)
    pos, vel, image = ref.step_one(p.pos, p.vel, p.mass, p.force, p.image, p.L, s)
    got_v, got_p, got_i = p.d_vel.cpu().numpy(), p.d_pos.cpu().numpy(), p.d_image.cpu().numpy()
    np.testing.assert_array_equal(_bits(got_v[:, :3]), _bits(vel))
    np.testing.assert_array_equal(_bits(got_v[:, 3]), _bits(p.mass))
    np.testing.assert_array_equal(_bits(got_p[:, :3]), _bits(pos))
    np.testing.assert_array_equal(_bits(got_p[:, 3]), _bits(p.type_w))
    np.testing.assert_array_equal(got_i, image)
    assert np.all(got_p[:, :3] >= -0.5 * p.L) and np.all(got_p[:, :3] < 0.5 * p.L)
    _assert_state(p.state(), s, "step one writes no state")
    if N >= 63:
        assert (image != p.image).any()  # some did cross


# ---------------------------------------------------------------------------------------------------------------------
# 3. the advance over a grid
# ---------------------------------------------------------------------------------------------------------------------
GRID_N = 2  # one workgroup, one partial per slot: the four partials ARE the sums; thresholds below are for N = 2


def advance_grid():
    """(sums (P, VV, FF, U), state, params) of every case. force_tol = 1e-3 and N = 2 put the threshold of FF at 6e-6;
    energy_tol = 1e-7 puts the one of |U - U_PREV| at 2e-7."""
    cases = []
    U = -1.0
    for msc in (0, 10):
        prm = dict(PARAMS, min_steps_conv=msc)
        msa = prm["min_steps_adapt"]
        n_steps_set = (0.0, 1.0, 2.0) if msc == 0 else (9.0, 10.0, 11.0)  # below, at and above max(1, min_steps_conv)
        for P, FF, VV, n_pos, dt, n_steps, dU, alpha in itertools.product(
                (-2.5, 0.0, 3.0), (0.0, 1e-30, 5.9e-6, 6.1e-6, 1.0, 1e12), (0.0, 1.0), (0.0, float(msa), float(msa + 1)),
                (0.05, 0.05 / 1.05, 0.0185), n_steps_set, (0.0, 1.9e-7, -2.1e-7), (0.1, 0.0437)):
            s = dict(ref.new_state(0.05), dt=dt, alpha=alpha, n_pos=n_pos, n_steps=n_steps, u_prev=U + dU, keep=0.77, mix=0.33)
            cases.append(((P, VV, FF, U), s, prm))
    # a NaN sum and an infinite sum in every slot, states that are already converged or already non-finite
    prm = dict(PARAMS)
    base = dict(ref.new_state(0.05), n_steps=20.0, n_pos=3.0, u_prev=-1.0, keep=0.77, mix=0.33)
    for slot, bad in itertools.product(range(4), (float("nan"), float("inf"), -float("inf"))):
        sums = [3.0, 1.0, 1.0, -1.0]
        sums[slot] = bad
        cases.append((tuple(sums), dict(base), prm))
    for flag, sums in itertools.product(("converged", "nonfinite"), ((3.0, 1.0, 1.0, -1.0), (-3.0, 1.0, 1e12, 5.0),
                                                                    (float("nan"), 1.0, 1.0, 1.0), (0.0, 0.0, 0.0, -1.0))):
        cases.append((sums, dict(base, keep=0.0, mix=0.0, **{flag: 1.0}), prm))
    return cases


def run_advance_grid(cases):
    """Every case on the device (one launch each, one readback for all): the states the device left, (n, NSTATE)."""
    import torch

    n = len(cases)
    d_state = _dev(np.array([ref.to_array(s) for _, s, _ in cases]))
    d_partial = _dev(np.array([sums for sums, _, _ in cases], dtype=np.float64))
    lib, stream = _lib.lib(), _stream()
    a = _lib.FireArgs()
    a.N, a.partials_bytes = GRID_N, 32
    for i, (_, _, prm) in enumerate(cases):
        a.d_state = d_state.data_ptr() + i * 8 * _lib.FIRE_NSTATE
        a.d_partials = d_partial.data_ptr() + i * 32
        _set_params(a, prm)
        _lib.check(lib.azp_fire_advance(C.byref(a), stream), "azp_fire_advance")
    torch.cuda.synchronize()
    assert d_state.shape == (n, _lib.FIRE_NSTATE)
    return d_state.cpu().numpy()


def test_advance_over_the_grid():
    cases = advance_grid()
    got = run_advance_grid(cases)
    k_mix = ref.SLOTS.index("mix")
    worst, seen = 0.0, dict(converged=0, nonfinite=0, grown=0, capped=0, dropped=0, kept=0)
    for i, (sums, s0, prm) in enumerate(cases):
        want = ref.advance(sums, s0, GRID_N, **_ref_params(prm))
        w = ref.to_array(want)
        for k, name in enumerate(ref.SLOTS):
            if name != "mix":
                assert _bits(got[i, k]) == _bits(w[k]), (i, name, got[i, k], w[k], sums, s0)
        if w[k_mix] == 0.0:
            assert got[i, k_mix] == 0.0, (i, sums, s0)
        else:
            worst = max(worst, abs(got[i, k_mix] - w[k_mix]) / abs(w[k_mix]))
        assert not np.any(got[i, len(ref.SLOTS):])
        # which paths the grid walks
        fresh = not (s0["converged"] or s0["nonfinite"])
        seen["converged"] += fresh and want["converged"] == 1.0
        seen["nonfinite"] += fresh and want["nonfinite"] == 1.0
        seen["kept"] += want == s0
        seen["grown"] += want["dt"] > s0["dt"]
        seen["capped"] += want["dt"] > s0["dt"] and want["dt"] == prm["dt_max"] and s0["dt"] * prm["finc_dt"] > prm["dt_max"]
        seen["dropped"] += want["dt"] < s0["dt"]
    print("advance grid: %d cases, largest relative deviation of MIX %.3g (ADVANCE_REL = %.3g); paths: %s"
          % (len(cases), worst, ref.ADVANCE_REL, seen))
    assert all(v > 0 for v in seen.values()), seen
    assert worst <= 1e-10, "a deviation of this size is a bug, not a tolerance"
    assert worst <= ref.ADVANCE_REL


# ---------------------------------------------------------------------------------------------------------------------
# 4. a driven trajectory through the C ABI
# ---------------------------------------------------------------------------------------------------------------------
WELL_K = np.array([1.0, 4.0, 9.0])
WELL_L = (1000.0, 1000.0, 1000.0)


def well_force(pos):
    """U = 1/2 sum k_c x_c^2: (force, each particle's energy), in a fixed order of operations."""
    f = -(WELL_K * pos)
    e = 0.5 * (((WELL_K[0] * pos[:, 0]) * pos[:, 0] + (WELL_K[1] * pos[:, 1]) * pos[:, 1]) + (WELL_K[2] * pos[:, 2]) * pos[:, 2])
    return f, e


def test_driven_trajectory_on_the_well():
    import torch

    N, steps, dt = 257, 300, 0.05
    rng = np.random.default_rng(257)
    p = _Particles(N, seed=4, L=WELL_L, pos=rng.normal(0.0, 1.0, (N, 3)))
    p.vel[:] = 0.0
    p.image[:] = 0
    p.d_vel.copy_(_dev(np.c_[p.vel, p.mass]))
    p.d_image.zero_()
    prm = dict(PARAMS, dt_max=dt, force_tol=1e-7, energy_tol=1e-7)
    a = p.args(**prm)
    log = {}
    want = ref.minimize(well_force, p.pos, p.vel, p.mass, p.L, dt, 1e-7, 1e-7, steps, stop_at_convergence=False,
                        record=lambda k, x, v, s: log.__setitem__(k, (x.copy(), v.copy(), dict(s))))

    def upload_forces():
        f, e = well_force(p.d_pos.cpu().numpy()[:, :3])
        p.d_force.copy_(_dev(np.c_[f, e]))

    p.set_state(ref.new_state(dt))
    upload_forces()
    _call("azp_fire_measure", a)
    for k in range(steps):
        _call("azp_fire_advance", a)
        _call("azp_fire_step_one", a)
        upload_forces()
        _call("azp_fire_step_two", a)
        if k % 10 == 9 or k == steps - 1:
            x, v, s = log[k]
            np.testing.assert_array_equal(_bits(p.d_pos.cpu().numpy()[:, :3]), _bits(x), err_msg="positions after step %d" % k)
            np.testing.assert_array_equal(_bits(p.d_vel.cpu().numpy()[:, :3]), _bits(v), err_msg="velocities after step %d" % k)
            _assert_state(p.state(), s, "state after step %d" % k)
    torch.cuda.synchronize()
    # not a trivial path: the run dropped its velocities at least once after the start, and the time step grew
    states = [log[k][2] for k in range(steps)]
    resets = [k for k in range(1, steps) if states[k]["p"] <= 0.0 and states[k]["dt"] == states[k - 1]["dt"] * 0.5]
    grown = [k for k in range(1, steps) if states[k]["dt"] > states[k - 1]["dt"]]
    print("driven trajectory: %d resets, %d increases of DT, converged %r after %d advances"
          % (len(resets), len(grown), bool(states[-1]["converged"]), int(states[-1]["n_steps"])))
    assert resets and grown
    assert not np.any(p.d_image.cpu().numpy())
    assert np.abs(want[0]).max() < 0.01 * np.abs(p.pos).max()  # and it went downhill


# ---------------------------------------------------------------------------------------------------------------------
# 5. through Simulation.run
# ---------------------------------------------------------------------------------------------------------------------
N_DIMERS = 128
DIMER_L = (48.0, 24.0, 24.0)
R_MIN = 2.0 ** (1.0 / 6.0)


def _dimer_positions(seed=128):
    """128 dimers along x on an 8 x 4 x 4 lattice of spacing 6 (more than 4 between any two dimers: beyond r_cut = 3),
    separations drawn from [1.0, 1.6]."""
    rng = np.random.default_rng(seed)
    L = np.asarray(DIMER_L)
    ix, iy, iz = np.meshgrid(np.arange(8), np.arange(4), np.arange(4), indexing="ij")
    c = (np.stack([ix.ravel(), iy.ravel(), iz.ravel()], axis=1) + 0.5) * 6.0 - 0.5 * L
    s = rng.uniform(1.0, 1.6, N_DIMERS)
    pos = np.repeat(c, 2, axis=0)
    pos[0::2, 0] -= 0.5 * s
    pos[1::2, 0] += 0.5 * s
    return pos


def _dimers(pos=None, sorter_period=None, dt=0.005, **kw):
    import azplugins_amd as azp

    snap = azp.Snapshot.from_arrays(_dimer_positions() if pos is None else pos, DIMER_L)
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(snap)
    if sorter_period is None:
        sim.operations.tuners.clear()
    else:
        assert len(sim.operations.tuners) == 1
        sim.operations.tuners[0].trigger_period = sorter_period
    plj = azp.pair.PerturbedLennardJones(nlist=azp.nlist.Cell(buffer=0.4), default_r_cut=3.0, mode="none")
    plj.params[("A", "A")] = dict(epsilon=1.0, sigma=1.0, attraction_scale_factor=1.0)
    args = dict(force_tol=1e-6, angmom_tol=1e-6, energy_tol=1e-10)
    args.update(kw)
    fire = azp.minimize.FIRE(dt=dt, forces=[plj], methods=[azp.ConstantVolume(azp.All())], **args)
    sim.operations.integrator = fire
    return sim, fire


def _by_tag(sim, name="pos"):
    st = sim.state
    tag = st.tag[: st.N].cpu().numpy().view(np.uint32).astype(np.int64)
    out = np.empty((st.N, 4))
    out[tag] = getattr(st, name)[: st.N].cpu().numpy()
    return out


@pytest.fixture(scope="module")
def minimized_dimers():
    """The dimers minimized ``while not converged`` in chunks of 100 steps, at most 3000 (tests/fire_ref.py with a numpy
    Lennard-Jones converges after 266 steps on the same start: well inside half the budget)."""
    sim, fire = _dimers(sorter_period=200)
    assert fire.converged is False
    while not fire.converged and sim.timestep < 3000:
        sim.run(100)
    return sim, fire


def test_dimers_reach_the_minimum(minimized_dimers):
    sim, fire = minimized_dimers
    print("dimers: converged %r after at most %d steps, energy %.12f, force_rms %.3g"
          % (fire.converged, sim.timestep, fire.energy, fire.force_rms))
    assert fire.converged and sim.timestep < 3000
    pos = _by_tag(sim)
    d = np.linalg.norm(pos[1::2, :3] - pos[0::2, :3], axis=1)
    assert np.abs(d - R_MIN).max() < 1e-5
    assert abs(fire.energy - (-0.5)) < 1e-9
    assert fire.force_rms < fire.force_tol


def test_nothing_moves_after_convergence(minimized_dimers):
    sim, fire = minimized_dimers
    assert fire.converged
    pos, vel, t0 = _by_tag(sim), _by_tag(sim, "vel"), sim.timestep
    state = fire._state.cpu().numpy().copy()
    sim.run(50)
    assert sim.timestep == t0 + 50
    np.testing.assert_array_equal(_bits(_by_tag(sim)), _bits(pos))
    np.testing.assert_array_equal(_bits(_by_tag(sim, "vel")), _bits(vel))
    np.testing.assert_array_equal(_bits(fire._state.cpu().numpy()), _bits(state))
    assert fire.converged


def test_reset(minimized_dimers):
    """(after the two tests above: it undoes the convergence they read)"""
    sim, fire = minimized_dimers
    assert fire.converged and np.abs(_by_tag(sim, "vel")[:, :3]).max() > 0.0
    fire.reset()
    want = ref.new_state(0.005)
    _assert_state(fire._state.cpu().numpy(), want, "after reset")
    vel = sim.state.vel[: sim.state.N].cpu().numpy()
    assert not np.any(vel[:, :3]) and np.all(vel[:, 3] == 1.0)
    assert fire.converged is False
    sim.run(30)  # at the minimum already: it converges again once min_steps_conv has passed
    assert fire.converged and int(fire._state[_lib.FIRE_N_STEPS].item()) == 10


@pytest.mark.parametrize("sorter_period", [None, 20])
def test_split_runs(sorter_period):
    import torch

    def final(chunks):
        sim, fire = _dimers(sorter_period=sorter_period)
        for n in chunks:
            sim.run(n)
        torch.cuda.synchronize()
        if sorter_period is not None:
            assert sim.operations.tuners[0].num_sorts >= 3
        return sim.state.pos.clone(), sim.state.vel.clone(), sim.state.image.clone(), fire._state.clone(), fire

    whole, split = final([60]), final([30, 30])
    for a, b in zip(whole[:4], split[:4]):
        assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), "run(30); run(30) differs from run(60)"
    s = whole[3].cpu().numpy()
    assert s[_lib.FIRE_N_STEPS] == 60 and s[_lib.FIRE_CONVERGED] == 0.0 and s[_lib.FIRE_VV] > 0.0  # it was under way
    assert whole[4].energy == split[4].energy and whole[4].force_rms == split[4].force_rms


def _chains(seed=64):
    """64 chains of 8 beads along x on an 8 x 8 grid of spacing 1.5 in (y, z), beads 1.05 apart, every coordinate
    jittered by up to 0.05: DoubleWell bonds (minima at 1 and 2), harmonic angles that want the chain straight and a
    purely repulsive PerturbedLJ (attraction_scale_factor = 0)."""
    import azplugins_amd as azp

    rng = np.random.default_rng(seed)
    L = np.array([12.0, 12.0, 12.0])
    iy, iz, ib = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")
    xyz = np.stack([(ib.ravel() + 0.5) * 1.05 - 4.2, (iy.ravel() + 0.5) * 1.5 - 6.0, (iz.ravel() + 0.5) * 1.5 - 6.0], axis=1)
    xyz += rng.uniform(-0.05, 0.05, xyz.shape)
    n = xyz.shape[0]
    d = xyz[:, None, :] - xyz[None, :, :]
    d -= L * np.rint(d / L)
    r = np.sqrt((d * d).sum(axis=2)) + 10.0 * np.eye(n)
    assert r.min() >= 0.9, r.min()  # no pair closer than 0.9
    first = np.arange(n)[ib.ravel() != 7]
    bonds = np.stack([first, first + 1], axis=1).astype(np.uint32)
    mid = np.arange(n)[(ib.ravel() != 0) & (ib.ravel() != 7)]
    angles = np.stack([mid - 1, mid, mid + 1], axis=1).astype(np.uint32)
    snap = azp.Snapshot.from_arrays(xyz, L, bonds=bonds, angles=angles)
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(snap)
    plj = azp.pair.PerturbedLennardJones(nlist=azp.nlist.Cell(buffer=0.4), default_r_cut=3.0, mode="none")
    plj.params[("A", "A")] = dict(epsilon=1.0, sigma=1.0, attraction_scale_factor=0.0)
    dw = azp.bond.DoubleWell()
    dw.params["A-A"] = dict(r_0=1.0, r_1=1.5, U_1=1.0, U_tilt=0.0)
    ha = azp.angle.Harmonic()
    ha.params["A-A-A"] = dict(k=5.0, t0=math.pi)
    fire = azp.minimize.FIRE(dt=0.005, force_tol=1e-4, angmom_tol=1e-4, energy_tol=1e-9, forces=[plj, dw, ha],
                             methods=[azp.ConstantVolume()])
    sim.operations.integrator = fire
    thermo = azp.compute.ThermodynamicQuantities(azp.All())
    sim.operations.add(thermo)
    return sim, fire, thermo


def test_chains_relax():
    sim, fire, thermo = _chains()
    N = sim.state.N
    assert N == 512 and len(sim.operations.tuners) == 1  # (the particle sorter stays on)
    sim.run(1)  # the first advance saw the configuration as built
    e0, f0 = fire.energy, fire.force_rms
    assert e0 == pytest.approx(thermo_energy_at_start(), rel=1e-12)
    sim.run(499)
    e500 = fire.energy
    assert e500 < e0
    while not fire.converged and sim.timestep < 3000:
        sim.run(100)
    print("chains: energy per particle %.6f -> %.6f (500 steps) -> %.6f, force_rms %.3g -> %.3g, converged %r after at most %d steps"
          % (e0, e500, fire.energy, f0, fire.force_rms, fire.converged, sim.timestep))
    assert fire.force_rms <= f0 / 100.0
    assert fire.energy <= e500
    # the recorder of thermodynamic quantities sees the energy the minimizer sees: once converged nothing moves, and
    # the last advance summed the forces of the configuration that is still there
    assert fire.converged
    assert thermo.potential_energy / N == pytest.approx(fire.energy, rel=1e-12)


def thermo_energy_at_start():
    """U / N of the chains as built, through compute.ThermodynamicQuantities on a second, equal system."""
    sim, fire, thermo = _chains()
    sim.run(0)
    return thermo.potential_energy / sim.state.N


def test_refusals_on_the_device():
    import azplugins_amd as azp
    from azplugins_amd import flow, thermostats

    sim, fire = _dimers()
    fire.methods = [azp.ConstantVolume(thermostat=thermostats.Bussi(kT=1.0, tau=0.5))]
    with pytest.raises(azp.AzpError, match="exactly one ConstantVolume"):
        sim.run(1)
    fire.methods = [flow.Langevin(azp.All(), kT=1.0, flow_field=flow.ConstantFlow((0.0, 0.0, 0.0)))]
    with pytest.raises(azp.AzpError, match="exactly one ConstantVolume"):
        sim.run(1)
    fire.methods = [azp.ConstantVolume(azp.All())]
    fire.integrate_rotational_dof = True
    with pytest.raises(azp.AzpError, match="rotational"):
        sim.run(1)
    fire.integrate_rotational_dof = False
    assert sim.timestep == 0 and fire.converged is False
    sim.run(2)
    assert sim.timestep == 2
    # a partials buffer that is too small, through the C ABI: refused ahead of the launch
    p = _Particles(257, seed=9)
    a = p.args()
    a.partials_bytes = 4 * 8 * 2 - 8  # (N = 257: two workgroups, four slots)
    for name in ("azp_fire_measure", "azp_fire_step_two", "azp_fire_advance"):
        assert getattr(_lib.lib(), name)(C.byref(a), _stream()) == -1
    a.partials_bytes = 4 * 8 * 2
    _call("azp_fire_measure", a)
    assert bool(p.d_partials.isfinite().all())


def test_nonfinite_forces_are_reported():
    """Two particles of one dimer at the same position: their force is not finite. That is an input error reported
    cleanly: the kernels only do arithmetic on it, the flag stops every later step, and nobody else's position suffers."""
    import azplugins_amd as azp

    pos = _dimer_positions()
    pos[11] = pos[10]
    sim, fire = _dimers(pos=pos)
    sim.run(20)
    assert sim.timestep == 20
    with pytest.raises(azp.AzpError, match="non-finite"):
        fire.converged
    with pytest.raises(azp.AzpError, match="non-finite"):
        fire.energy
    got = _by_tag(sim)
    others = np.ones(2 * N_DIMERS, dtype=bool)
    others[10:12] = False
    assert np.all(np.isfinite(got[others, :3]))
    np.testing.assert_array_equal(_bits(got[:, :3]), _bits(pos))  # the flag was raised by the first advance: nothing moved
    assert fire._state[_lib.FIRE_NONFINITE].item() == 1.0 and fire._state[_lib.FIRE_N_STEPS].item() == 0.0
