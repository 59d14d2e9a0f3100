"""The thermostats of ConstantVolume on the GPU (csrc/thermostat.hip) against tests/thermostat_ref.py: the kinetic pass,
step two with partials and the scaled step one bit for bit through the C ABI, the advance over a grid of parameters
within ``ALPHA_REL``, and runs of an ideal gas and of the PerturbedLJ liquid through ``Simulation.run``.

Deviations of the advance are taken relative to the sum of the magnitudes of the terms a quantity is made of (alpha:
alpha itself; xi: |xi_0| + (dt / tau^2)(2 K / (Nf kT) + 1); eta: |eta_0| + |xi| dt; energy: |energy_0| + K + alpha^2 K,
for MTTK Nf kT (tau^2 xi^2 / 2 + |eta|)): a quantity that cancels to zero has no relative error of its own."""

import ctypes as C
import itertools
import math

import numpy as np
import pytest

import thermostat_ref as ref
from azplugins_amd import _lib

pytestmark = pytest.mark.gpu

# 63 * 256 to 64 * 256 + 1: 63, 64 and 65 partials, the fold's step from one round of a wave to two; the last: two
# particles per lane, 1025 partials
SIZES = [2, 63, 64, 65, 255, 256, 257, 1000, 63 * 256, 64 * 256, 64 * 256 + 1, 2048 * 256 + 1]
L_BOX = (6.0, 7.0, 8.0)


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _stream():
    return _lib.raw_stream("cuda:0")


class _Particles:
    """Host arrays and their device copies behind one azp_thermostat_args."""

    def __init__(self, N, seed, v_scale=1.0):
        import torch

        rng = np.random.default_rng(seed)
        L = np.asarray(L_BOX)
        self.N = N
        self.pos = rng.uniform(-0.5, 0.5, (N, 3)) * L
        self.vel = rng.normal(0.0, v_scale, (N, 3))
        self.mass = rng.uniform(0.5, 2.0, N)
        self.force = rng.normal(0.0, 5.0, (N, 3))
        self.image = rng.integers(-3, 4, (N, 3)).astype(np.int32)
        self.type_w = rng.integers(0, 3, N).astype(np.int64).view(np.float64)
        self.d_pos = _dev(np.c_[self.pos, self.type_w])
        self.d_vel = _dev(np.c_[self.vel, self.mass])
        self.d_force = _dev(np.c_[self.force, rng.normal(size=N)])
        self.d_image = _dev(self.image)
        need = C.c_uint64(0)
        _lib.check(_lib.lib().azp_thermostat_partials_size(N, C.byref(need)))
        self.d_partials = torch.full((need.value // 8,), float("nan"), dtype=torch.float64, device="cuda:0")
        self.d_state = torch.zeros(_lib.THERMOSTAT_NSTATE, dtype=torch.float64, device="cuda:0")

    def args(self, dt=0.005, kind=_lib.THERMOSTAT_BERENDSEN, kT=1.0, tau=1.0):
        a = _lib.ThermostatArgs()
        a.d_pos, a.d_vel, a.d_net_force = self.d_pos.data_ptr(), self.d_vel.data_ptr(), self.d_force.data_ptr()
        a.d_image = self.d_image.data_ptr()
        a.d_partials, a.partials_bytes = self.d_partials.data_ptr(), self.d_partials.numel() * 8
        a.d_state = self.d_state.data_ptr()
        a.box = _lib.make_box(L_BOX)
        a.dt, a.kT, a.tau, a.ndof = dt, kT, tau, float(max(3 * self.N - 3, 3))
        a.kind, a.N = kind, self.N
        return a


def _call(name, a):
    _lib.check(getattr(_lib.lib(), name)(C.byref(a), _stream()), name)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kinetic pass and step two with partials, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
def test_kinetic_pass_and_step_two(N):
    p = _Particles(N, seed=1000 + N % 97)
    dt = 0.01
    a = p.args(dt=dt, kind=_lib.THERMOSTAT_MTTK)
    _call("azp_thermostat_kinetic", a)
    _call("azp_thermostat_advance", a)  # (the fold: K lands in the state)
    K0 = p.d_state.cpu().numpy()[_lib.THERMOSTAT_K]
    np.testing.assert_array_equal(_bits(p.d_vel.cpu().numpy()[:, :3]), _bits(p.vel))  # the kinetic pass writes no velocity
    want0 = ref.kinetic_energy(p.vel, p.mass)
    assert _bits(K0) == _bits(want0), (K0, want0)
    _call("azp_thermostat_step_two", a)
    _call("azp_thermostat_advance", a)
    K1 = p.d_state.cpu().numpy()[_lib.THERMOSTAT_K]
    got = p.d_vel.cpu().numpy()
    v1 = ref.step_two(p.vel, p.mass, p.force, dt)
    np.testing.assert_array_equal(_bits(got[:, :3]), _bits(v1))
    np.testing.assert_array_equal(_bits(got[:, 3]), _bits(p.mass))
    want1 = ref.kinetic_energy(v1, p.mass)
    assert _bits(K1) == _bits(want1), (K1, want1)
    assert K1 != K0


# ---------------------------------------------------------------------------------------------------------------------
# 2. the scaled step one, bit for bit, with the alpha the device wrote
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
def test_scaled_step_one(N):
    p = _Particles(N, seed=2000 + N % 97, v_scale=8.0)
    dt = 0.05  # |v| dt ~ 0.4 in a box of edges 6 to 8: a few percent of the particles cross a periodic face per axis
    a = p.args(dt=dt, kind=_lib.THERMOSTAT_BERENDSEN, kT=0.7, tau=0.2)
    _call("azp_thermostat_kinetic", a)
    _call("azp_thermostat_advance", a)
    _call("azp_thermostat_step_one", a)
    state = p.d_state.cpu().numpy()
    alpha = float(state[_lib.THERMOSTAT_ALPHA])
    assert 0.0 < alpha < 1.0  # (the gas is far hotter than kT)
    pos, vel, image = ref.step_one(p.pos, p.vel, p.mass, p.force, p.image, L_BOX, dt, alpha)
    got_v, got_p, got_i = p.d_vel.cpu().numpy(), p.d_pos.cpu().numpy(), p.d_image.cpu().numpy()
    np.testing.assert_array_equal(_bits(got_v[:, :3]), _bits(vel))
    np.testing.assert_array_equal(_bits(got_v[:, 3]), _bits(p.mass))
    np.testing.assert_array_equal(_bits(got_p[:, :3]), _bits(pos))
    np.testing.assert_array_equal(_bits(got_p[:, 3]), _bits(p.type_w))
    np.testing.assert_array_equal(got_i, image)
    L = np.asarray(L_BOX)
    assert np.all(got_p[:, :3] >= -0.5 * L) and np.all(got_p[:, :3] < 0.5 * L)
    if N >= 63:
        assert (image != p.image).any()  # some did cross


# ---------------------------------------------------------------------------------------------------------------------
# 3. the advance over a grid
# ---------------------------------------------------------------------------------------------------------------------
def advance_grid():
    """(kind, kT, tau, dt, ndof, timestep, seed, K, state0) of every case: kT, dt, tau (Bussi's 0 and Berendsen's
    tau = dt included), Nf from 3 to 3 * 2^20 - 3, K from 0 to 3 Kbar, a fresh and a used state and, for Bussi, sixteen
    (timestep, seed) pairs up to 40-bit timesteps and the largest seed."""
    cases = []
    states = [ref.new_state(), dict(energy=-3.25, xi=0.3, eta=-0.2)]
    rng = np.random.default_rng(204)
    draws = [(0, 0), (12345, 7), (2**32 + 7, 65535), ((0xAB << 32) | 99, 4242)]
    draws += [(int(t), int(sd)) for t, sd in zip(rng.integers(0, 2**40, 12), rng.integers(0, 2**16, 12))]
    for kind, kT, dt, ndof in itertools.product((ref.BERENDSEN, ref.BUSSI, ref.MTTK), (0.5, 1.0, 1.5, 2.7), (0.001, 0.0037, 0.01),
                                                (3.0, 93.0, 2997.0, 3.0 * 2**20 - 3.0)):
        taus = {ref.BERENDSEN: (dt, 0.1, 0.73, 2.0), ref.BUSSI: (0.0, dt, 0.1, 0.73, 2.0), ref.MTTK: (0.05, 0.1, 0.73, 2.0)}[kind]
        Kbar = 0.5 * ndof * kT
        for tau, (t, seed), x, s0 in itertools.product(taus, draws if kind == ref.BUSSI else draws[:1],
                                                       (0.0, 0.1, 0.5, 1.0, 1.7, 3.0), states):
            cases.append((kind, kT, tau, dt, ndof, t, seed, x * Kbar, s0))
    return cases


def advance_deviations(cases):
    """Runs every case on the device (one launch each, one readback for all) and returns per case the deviations of
    (alpha, xi, eta, energy) from the reference, each relative to its scale, and the Gamma attempts (device, host)."""
    import torch

    n = len(cases)
    state = np.zeros((n, _lib.THERMOSTAT_NSTATE))
    partial = np.zeros(n)
    for i, (kind, kT, tau, dt, ndof, t, seed, K, s0) in enumerate(cases):
        state[i, _lib.THERMOSTAT_ENERGY], state[i, _lib.THERMOSTAT_XI], state[i, _lib.THERMOSTAT_ETA] = s0["energy"], s0["xi"], s0["eta"]
        state[i, _lib.THERMOSTAT_ALPHA] = state[i, _lib.THERMOSTAT_K] = np.nan
        partial[i] = K
    d_state, d_partial = _dev(state), _dev(partial)
    lib, stream = _lib.lib(), _stream()
    a = _lib.ThermostatArgs()
    a.N, a.partials_bytes = 2, 8  # (N = 2: one workgroup, one partial, which holds K)
    for i, (kind, kT, tau, dt, ndof, t, seed, K, s0) in enumerate(cases):
        a.d_state = d_state.data_ptr() + i * 8 * _lib.THERMOSTAT_NSTATE
        a.d_partials = d_partial.data_ptr() + i * 8
        a.kind, a.kT, a.tau, a.dt, a.ndof, a.timestep, a.seed = kind, kT, tau, dt, ndof, t, seed
        _lib.check(lib.azp_thermostat_advance(C.byref(a), stream), "azp_thermostat_advance")
    torch.cuda.synchronize()
    got = d_state.cpu().numpy()
    dev = np.zeros((n, 4))
    attempts = np.zeros((n, 2), dtype=np.int64)
    for i, (kind, kT, tau, dt, ndof, t, seed, K, s0) in enumerate(cases):
        alpha, s, tries = ref.advance(kind, K, s0, kT, tau, dt, ndof, seed, t)
        g = got[i]
        assert _bits(g[_lib.THERMOSTAT_K]) == _bits(K)
        attempts[i] = (int(g[_lib.THERMOSTAT_ATTEMPTS]), tries)
        dev[i, 0] = abs(g[_lib.THERMOSTAT_ALPHA] - alpha) / alpha
        if kind == ref.MTTK:
            xi_scale = abs(s0["xi"]) + (dt / (tau * tau)) * (2.0 * K / (ndof * kT) + 1.0)
            eta_scale = abs(s0["eta"]) + abs(s["xi"]) * dt
            e_scale = ndof * kT * (0.5 * tau * tau * s["xi"] ** 2 + abs(s["eta"]))
        else:
            xi_scale = eta_scale = 1.0
            e_scale = abs(s0["energy"]) + K + alpha * alpha * K
        # (a scale of zero: every term is zero, and so must the difference be)
        dev[i, 1] = abs(g[_lib.THERMOSTAT_XI] - s["xi"]) / (xi_scale or 1.0)
        dev[i, 2] = abs(g[_lib.THERMOSTAT_ETA] - s["eta"]) / (eta_scale or 1.0)
        dev[i, 3] = abs(g[_lib.THERMOSTAT_ENERGY] - s["energy"]) / (e_scale or 1.0)
    return dev, attempts, got


def test_advance_over_the_grid():
    cases = advance_grid()
    dev, attempts, got = advance_deviations(cases)
    kinds = np.array([c[0] for c in cases])
    for kind, name in ((ref.BERENDSEN, "Berendsen"), (ref.BUSSI, "Bussi"), (ref.MTTK, "MTTK")):
        print("%s: %d cases, largest deviation of alpha %.3g, xi %.3g, eta %.3g, energy %.3g"
              % ((name, int((kinds == kind).sum())) + tuple(dev[kinds == kind].max(axis=0))))
    print("largest deviation over the grid: %.3g (ALPHA_REL = %.3g)" % (dev.max(), ref.ALPHA_REL))
    assert np.all(np.isfinite(got[:, :6]))
    # the device's sampler takes the attempts the host's takes, and neither reaches the cap
    np.testing.assert_array_equal(attempts[:, 0], attempts[:, 1])
    assert attempts.max() <= ref.GAMMA_MAX_ATTEMPTS
    for i, c in enumerate(cases):
        kind, K, s0 = c[0], c[7], c[8]
        if K == 0.0 and kind != ref.MTTK:
            # alpha = 1 and the state unchanged, in every bit
            assert got[i, _lib.THERMOSTAT_ALPHA] == 1.0
            assert (got[i, _lib.THERMOSTAT_ENERGY], got[i, _lib.THERMOSTAT_XI], got[i, _lib.THERMOSTAT_ETA]) == (s0["energy"], s0["xi"], s0["eta"])
        if kind != ref.MTTK:
            assert (got[i, _lib.THERMOSTAT_XI], got[i, _lib.THERMOSTAT_ETA]) == (s0["xi"], s0["eta"])
    assert dev.max() <= 1e-10, "a deviation of this size is a bug, not a tolerance"
    worst = int(np.argmax(dev.max(axis=1)))
    assert dev.max() <= ref.ALPHA_REL, (cases[worst], dev[worst])


# ---------------------------------------------------------------------------------------------------------------------
# 4. runs of an ideal gas
# ---------------------------------------------------------------------------------------------------------------------
GAS_N, GAS_DT = 32, 0.005
GAS_NDOF = 3.0 * GAS_N - 3.0


def _ramp(t):
    return 1.0 + 0.002 * t


def _thermostat(kind, kT=None):
    from azplugins_amd import thermostats

    if kind == "berendsen":
        return thermostats.Berendsen(kT=1.5 if kT is None else kT, tau=0.25), ref.BERENDSEN
    if kind == "bussi":
        return thermostats.Bussi(kT=_ramp if kT is None else kT, tau=0.1), ref.BUSSI
    if kind == "bussi0":
        return thermostats.Bussi(kT=1.5 if kT is None else kT), ref.BUSSI
    return thermostats.MTTK(kT=1.5 if kT is None else kT, tau=0.2), ref.MTTK


def _gas(kind, seed=5, recorder=True):
    import azplugins_amd as azp
    from azplugins_amd import compute

    rng = np.random.default_rng(77)
    L = 10.0
    snap = azp.Snapshot.from_arrays(rng.uniform(-0.5 * L, 0.5 * L, (GAS_N, 3)), [L, L, L], velocity=rng.normal(size=(GAS_N, 3)))
    snap.particles.mass[:] = rng.uniform(0.5, 2.0, GAS_N)
    sim = azp.Simulation(device="cuda:0", seed=seed)
    sim.create_state_from_snapshot(snap)
    sim.operations.tuners.clear()  # (the reference sums K in the snapshot's order; the liquid below keeps the sorter)
    th, ref_kind = _thermostat(kind)
    sim.operations.integrator = azp.Integrator(dt=GAS_DT, forces=[], methods=[azp.ConstantVolume(azp.All(), th)])
    rec = None
    if recorder:
        thermo = compute.ThermodynamicQuantities(azp.All())
        sim.operations.add(thermo)
        rec = compute.ThermodynamicRecorder(thermo, azp.Periodic(1))
        sim.operations.add(rec)
    return sim, th, ref_kind, rec


def _host_K(sim):
    v = sim.state.vel[: sim.state.N].cpu().numpy()
    return ref.kinetic_energy(v[:, :3], v[:, 3])


def _host_vel(sim):
    v = sim.state.vel[: sim.state.N].cpu().numpy()
    return v[:, :3].copy(), v[:, 3].copy()


@pytest.mark.parametrize("kind", ["berendsen", "bussi", "bussi0", "mttk"])
def test_ideal_gas_follows_the_recurrence(kind):
    """200 steps without forces, K read through the recorder at every step, against the reference recurrence within
    2 * steps * ALPHA_REL. ALPHA_REL measured 0 (tests/thermostat_ref.py), so that is bit equality, and the recurrence is
    the one that can be met to the bit: ``ideal_gas_particles`` carries it in the arithmetic the kernels define (every
    velocity scaled, K re-summed in the device's order). The scalar form K_(n+1) = alpha_n^2 K_n replaces N rounded
    products and a sum by one product; it is held within ``recurrence_rounding``, a bound from the number format
    (measured: 7.5e-16 to 3.1e-15 over the 200 steps)."""
    steps = 200
    sim, th, ref_kind, rec = _gas(kind)
    v0, mass = _host_vel(sim)
    x0 = sim.state.pos[:GAS_N, :3].cpu().numpy().copy()
    sim.run(steps)
    assert sim.timestep == steps and rec.timesteps.tolist() == list(range(1, steps + 1))
    got = rec.table["kinetic_energy"]
    Ks, alphas, want, v_end, state, worst = ref.ideal_gas_particles(ref_kind, v0, mass, steps, th.kT, th.tau, GAS_DT, GAS_NDOF,
                                                                    seed=sim.seed)
    assert worst <= ref.GAMMA_MAX_ATTEMPTS
    rel = np.abs(got - want) / want
    tol = 2 * steps * ref.ALPHA_REL
    print("%s: K follows the recurrence within %.3g (allowed %.3g)" % (kind, rel.max(), tol))
    assert rel.max() <= tol
    assert np.abs(alphas - 1.0).max() > 1e-4  # the thermostat acted
    # the scalar recurrence, and for Berendsen its closed form, up to rounding
    scalar = ref.ideal_gas(ref_kind, Ks[0], steps, th.kT, th.tau, GAS_DT, GAS_NDOF, seed=sim.seed)[0]
    rel_scalar = np.abs(got - scalar[1:]) / scalar[1:]
    print("%s: and the scalar recurrence within %.3g (allowed %.3g)" % (kind, rel_scalar.max(), ref.recurrence_rounding(steps)))
    assert rel_scalar.max() <= ref.recurrence_rounding(steps)
    if kind == "berendsen":
        closed = ref.berendsen_closed(Ks[0], steps, 1.5, th.tau, GAS_DT, GAS_NDOF)
        # (the closed form adds a power of up to 200 and a few operations of its own: as much again)
        assert np.abs(got - closed[1:]).max() <= 2 * ref.recurrence_rounding(steps) * closed.max()
    assert abs(th.energy - state["energy"]) <= tol * (abs(state["energy"]) + Ks[0] + want[-1])
    if kind == "mttk":
        xi, eta = th.translational_dof
        assert abs(xi - state["xi"]) <= tol * max(abs(state["xi"]), GAS_DT / th.tau**2)
        assert abs(eta - state["eta"]) <= tol * max(abs(state["eta"]), abs(state["xi"]) * GAS_DT)
    got_v, _ = _host_vel(sim)
    assert np.abs(got_v - v_end).max() <= tol * np.abs(v_end).max()
    assert not np.array_equal(sim.state.pos[:GAS_N, :3].cpu().numpy(), x0)  # the particles moved


@pytest.mark.parametrize("kind", ["berendsen", "bussi", "mttk"])
def test_split_runs_and_seeds(kind):
    import torch

    def final(seed, chunks):
        sim, th, _, _ = _gas(kind, seed=seed, recorder=False)
        for n in chunks:
            sim.run(n)
        torch.cuda.synchronize()
        return sim.state.vel.clone(), sim.state.pos.clone(), th._state.clone()

    whole = final(5, [20])
    split = final(5, [10, 10])
    again = final(5, [20])
    for a, b, c in zip(whole, split, again):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64)), "run(10); run(10) differs from run(20)"
        assert torch.equal(a.view(torch.int64), c.view(torch.int64)), "the same seed twice differs"
    other = final(6, [20])
    if kind == "bussi":
        assert not torch.equal(whole[0], other[0])
    else:
        assert torch.equal(whole[0].view(torch.int64), other[0].view(torch.int64))  # (no random numbers)


def test_mttk_translational_dof_between_runs():
    """The step after ``translational_dof`` is set starts from the new (xi, eta): K of the scaled velocities, xi, eta
    and the energy against the reference within 2 * ALPHA_REL (bit equality, as in
    test_ideal_gas_follows_the_recurrence)."""
    sim, th, _, _ = _gas("mttk", recorder=False)
    sim.run(5)
    assert th.translational_dof != (0.0, 0.0)
    th.translational_dof = (0.5, 0.1)
    assert th.translational_dof == (0.5, 0.1)
    assert th.energy == ref.mttk_energy(0.5, 0.1, GAS_NDOF, 1.5, th.tau)
    K = _host_K(sim)
    v, mass = _host_vel(sim)
    sim.run(1)
    alpha, state, _ = ref.advance(ref.MTTK, K, dict(energy=0.0, xi=0.5, eta=0.1), 1.5, th.tau, GAS_DT, GAS_NDOF)
    assert alpha < 1.0
    tol = 2 * ref.ALPHA_REL
    K1 = ref.kinetic_energy(alpha * v, mass)
    assert abs(_host_K(sim) - K1) <= tol * K1
    assert abs(K1 - alpha * alpha * K) <= ref.recurrence_rounding(1) * K
    xi, eta = th.translational_dof
    assert abs(xi - state["xi"]) <= tol * abs(state["xi"]) and abs(eta - state["eta"]) <= tol * abs(state["eta"])
    assert abs(th.energy - state["energy"]) <= tol * abs(state["energy"])
    # Berendsen and Bussi: the energy can be set
    sim, th, _, _ = _gas("berendsen", recorder=False)
    sim.run(3)
    e = th.energy
    assert e != 0.0
    th.energy = 0.0
    K = _host_K(sim)
    sim.run(1)
    alpha, state, _ = ref.advance(ref.BERENDSEN, K, ref.new_state(), 1.5, th.tau, GAS_DT, GAS_NDOF)
    assert abs(th.energy - state["energy"]) <= tol * (K + alpha * alpha * K)


def test_driver_rejections_on_the_device():
    import azplugins_amd as azp
    from azplugins_amd import thermostats

    sim, th, _, _ = _gas("bussi", recorder=False)
    integ = sim.operations.integrator
    other = azp.ConstantVolume(thermostat=th)  # a second method with the same thermostat
    with pytest.raises(azp.AzpError, match="two methods"):
        sim.run(1)
    other.thermostat = None
    integ.methods[0].thermostat = thermostats.Berendsen(kT=1.0, tau=0.5 * GAS_DT)
    with pytest.raises(azp.AzpError, match="below dt"):
        sim.run(1)
    integ.methods[0].thermostat = th
    integ.integrate_rotational_dof = True
    with pytest.raises(azp.AzpError, match="rotational"):
        sim.run(1)
    integ.integrate_rotational_dof = False
    sim.run(2)
    assert sim.timestep == 2


# ---------------------------------------------------------------------------------------------------------------------
# 5. the liquid
# ---------------------------------------------------------------------------------------------------------------------
LIQ_DT, LIQ_STEPS, LIQ_EVERY = 0.005, 2000, 100


def _liquid(thermostat, **kw):
    import azplugins_amd as azp

    sim = azp.Simulation(device="cuda:0", seed=9)
    sim.create_state_from_snapshot(azp.lattice_snapshot(n=10, a=0.8 ** (-1.0 / 3.0)))  # N = 1000, rho* = 0.8
    sim.thermalize_particle_momenta(kT=1.0, seed=17)
    assert len(sim.operations.tuners) == 1  # (the particle sorter stays on)
    nl = azp.nlist.Cell(buffer=0.4)
    plj = azp.pair.PerturbedLennardJones(nlist=nl, default_r_cut=3.0, mode="shift")
    plj.params[("A", "A")] = dict(epsilon=1.0, sigma=1.0, attraction_scale_factor=0.5)
    sim.operations.integrator = azp.Integrator(dt=LIQ_DT, forces=[plj], methods=[azp.ConstantVolume(thermostat=thermostat, **kw)])
    return sim


@pytest.fixture(scope="module")
def liquid_runs():
    """NVE and the three thermostats on the same liquid: K + U (+ the thermostat's energy) every LIQ_EVERY steps, the
    kinetic temperature and the total momentum at every step."""
    import azplugins_amd as azp
    from azplugins_amd import compute, thermostats

    tau = 100 * LIQ_DT
    out = {}
    for name, th in (("nve", None), ("mttk", thermostats.MTTK(kT=1.0, tau=tau)), ("bussi", thermostats.Bussi(kT=1.5, tau=tau)),
                     ("berendsen", thermostats.Berendsen(kT=1.5, tau=tau))):
        sim = _liquid(th)
        thermo = compute.ThermodynamicQuantities(azp.All())
        sim.operations.add(thermo)
        rec = compute.ThermodynamicRecorder(thermo, azp.Periodic(1))
        sim.operations.add(rec)
        sim.run(0)
        N = sim.state.N
        E = [thermo.kinetic_energy + thermo.potential_energy + (th.energy if th is not None else 0.0)]
        P0 = np.asarray(thermo.linear_momentum)
        extra = [0.0]
        for _ in range(LIQ_STEPS // LIQ_EVERY):
            sim.run(LIQ_EVERY)
            extra.append(th.energy if th is not None else 0.0)
        table = rec.table
        total = table["kinetic_energy"] + table["potential_energy"]
        E += [total[k * LIQ_EVERY - 1] + extra[k] for k in range(1, len(extra))]
        E = np.array(E)
        out[name] = dict(N=N, drift=np.abs(E - E[0]).max() / N, temperature=table["kinetic_temperature"],
                         momentum=np.linalg.norm(table["linear_momentum"] - P0, axis=1).max(),
                         sorts=sim.operations.tuners[0].num_sorts)
        print("%s: drift of the conserved energy per particle %.4g, mean kT of the last 1000 steps %.4f, momentum growth %.3g, "
              "%d sorts" % (name, out[name]["drift"], table["kinetic_temperature"][-1000:].mean(), out[name]["momentum"],
                            out[name]["sorts"]))
    return out


@pytest.mark.parametrize("name", ["mttk", "bussi", "berendsen"])
def test_liquid_conserved_energy(liquid_runs, name):
    nve, run = liquid_runs["nve"], liquid_runs[name]
    assert run["N"] == 1000 and run["sorts"] >= 1 and nve["drift"] > 0.0
    assert run["drift"] <= 4.0 * nve["drift"], (run["drift"], nve["drift"])


@pytest.mark.parametrize("name", ["bussi", "berendsen"])
def test_liquid_reaches_the_temperature(liquid_runs, name):
    ndof = 3.0 * 1000 - 3.0
    T = liquid_runs[name]["temperature"]
    assert len(T) == LIQ_STEPS
    assert abs(T[-1000:].mean() - 1.5) <= 5.0 * 1.5 * math.sqrt(2.0 / ndof), T[-1000:].mean()


@pytest.mark.parametrize("name", ["mttk", "bussi", "berendsen"])
def test_liquid_momentum(liquid_runs, name):
    assert liquid_runs[name]["momentum"] <= 4.0 * liquid_runs["nve"]["momentum"], (liquid_runs[name]["momentum"], liquid_runs["nve"]["momentum"])


def test_unthermostatted_path_is_unchanged():
    import torch

    import azplugins_amd as azp

    finals = []
    for bare in (True, False):
        sim = _liquid(None)  # ConstantVolume(thermostat=None)
        if bare:
            sim.operations.integrator.methods[0] = azp.ConstantVolume()
        assert sim.operations.integrator.methods[0].thermostat is None
        sim.run(50)
        torch.cuda.synchronize()
        finals.append((sim.state.pos.clone(), sim.state.vel.clone()))
    for a, b in zip(*finals):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))
