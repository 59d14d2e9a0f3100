"""ConstantPressure on the GPU (csrc/barostat.hip) against tests/barostat_ref.py: step one and step two bit for bit
through the C ABI, the advance over a grid of parameters within ``BARO_REL``, and runs of an ideal gas and of the
PerturbedLJ liquid through ``Simulation.run``.

Deviations of the advance are taken relative to the sum of the magnitudes of the terms a quantity is made of (nu:
|nu_0| + halves (dt / 2)(|K_aa| + |W_aa| + |V S_a| + 2 K / Nf) / W, the largest over the axes; alpha, lambda, b, alpha_T
and the energy: the quantity itself, a product or a sum of positive terms)."""

import ctypes as C
import itertools
import math

import numpy as np
import pytest

import barostat_ref as ref
import thermostat_ref
from azplugins_amd import _lib

pytestmark = pytest.mark.gpu

L_BOX = (6.0, 7.0, 8.0)
NS = _lib.BAROSTAT_NSTATE
NU, ALPHA, LAMBDA, B = _lib.BAROSTAT_NU, _lib.BAROSTAT_ALPHA, _lib.BAROSTAT_LAMBDA, _lib.BAROSTAT_B


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _stream():
    return _lib.raw_stream("cuda:0")


def _call(name, a):
    _lib.check(getattr(_lib.lib(), name)(C.byref(a), _stream()), name)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# 1. step one and step two, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 255, 256, 257, 1000, 64 * 256 + 1])
def test_step_one_and_step_two(N):
    import torch

    rng = np.random.default_rng(3000 + N % 97)
    L = np.asarray(L_BOX)
    dt = 0.05  # |v| dt ~ 0.4 in a box of edges 6 to 8: a few percent of the particles cross a periodic face per axis
    pos = rng.uniform(-0.5, 0.5, (N, 3)) * L
    vel = rng.normal(0.0, 8.0, (N, 3))
    # (row 0 sits at the +x face and moves outwards: it crosses whatever N is)
    pos[0, 0], vel[0, 0] = 0.499 * L[0], 8.0
    mass = rng.uniform(0.5, 2.0, N)
    force = rng.normal(0.0, 5.0, (N, 3))
    image = rng.integers(-3, 4, (N, 3)).astype(np.int32)
    type_w = rng.integers(0, 3, N).astype(np.int64).view(np.float64)
    d_pos, d_vel, d_force, d_image = _dev(np.c_[pos, type_w]), _dev(np.c_[vel, mass]), _dev(np.c_[force, rng.normal(size=N)]), _dev(image)
    state = np.zeros(NS)
    state[NU:NU + 3] = (0.3, -0.2, 0.25)
    state[_lib.BAROSTAT_REF_KT] = 1.0
    d_state = _dev(state)
    d_sums = torch.zeros(_lib.THERMO_NSUMS, dtype=torch.float64, device="cuda:0")  # (no kinetic energy, no virial, S = 0: G = 0)
    a = _lib.BarostatArgs()
    a.d_pos, a.d_vel, a.d_net_force, a.d_image = d_pos.data_ptr(), d_vel.data_ptr(), d_force.data_ptr(), d_image.data_ptr()
    a.d_state, a.d_sums = d_state.data_ptr(), d_sums.data_ptr()
    a.box = _lib.make_box(L_BOX)
    a.dt, a.tauS, a.ndof, a.box_dof, a.phase, a.N = dt, 1.0, float(max(3 * N - 3, 3)), 7, _lib.BAROSTAT_OPEN, N
    _call("azp_barostat_advance", a)
    d_state[_lib.BAROSTAT_ALPHA_T] = 0.9375  # (as a thermostat's advance would have left it)
    s = d_state.cpu().numpy()
    assert s[_lib.BAROSTAT_NONFINITE] == 0.0
    np.testing.assert_array_equal(s[NU:NU + 3], (0.3, -0.2, 0.25))
    alpha, lam, b, alpha_T = s[ALPHA:ALPHA + 3], s[LAMBDA:LAMBDA + 3], s[B:B + 3], float(s[_lib.BAROSTAT_ALPHA_T])
    assert len(set(alpha)) == 3 and len(set(lam)) == 3 and len(set(b)) == 3 and np.all(np.abs(lam - 1.0) > 5e-3)
    L_new = lam * L
    a.box = _lib.make_box(tuple(L_new))
    _call("azp_barostat_step_one", a)
    want_p, want_v, want_i = ref.step_one(pos, vel, mass, force, image, L_new, dt, alpha, lam, b, alpha_T)
    got_v, got_p, got_i = d_vel.cpu().numpy(), d_pos.cpu().numpy(), d_image.cpu().numpy()
    np.testing.assert_array_equal(_bits(got_v[:, :3]), _bits(want_v))
    np.testing.assert_array_equal(_bits(got_v[:, 3]), _bits(mass))
    np.testing.assert_array_equal(_bits(got_p[:, :3]), _bits(want_p))
    np.testing.assert_array_equal(_bits(got_p[:, 3]), _bits(type_w))
    np.testing.assert_array_equal(got_i, want_i)
    assert np.all(got_p[:, :3] >= -0.5 * L_new) and np.all(got_p[:, :3] < 0.5 * L_new)
    assert (want_i != image).any()  # some did cross
    assert want_i[0, 0] == image[0, 0] + 1
    # step two with a force of its own
    force2 = rng.normal(0.0, 5.0, (N, 3))
    d_force2 = _dev(np.c_[force2, rng.normal(size=N)])
    a.d_net_force = d_force2.data_ptr()
    _call("azp_barostat_step_two", a)
    got_v2 = d_vel.cpu().numpy()
    np.testing.assert_array_equal(_bits(got_v2[:, :3]), _bits(ref.step_two(want_v, mass, force2, dt, alpha)))
    np.testing.assert_array_equal(_bits(got_v2[:, 3]), _bits(mass))
    np.testing.assert_array_equal(_bits(d_pos.cpu().numpy()), _bits(got_p))  # step two moves nothing
    del d_force, d_force2


# ---------------------------------------------------------------------------------------------------------------------
# 2. the advance over a grid
# ---------------------------------------------------------------------------------------------------------------------
THERMOSTATS = (None, (thermostat_ref.BERENDSEN, 0.25), (thermostat_ref.BUSSI, 0.1), (thermostat_ref.MTTK, 0.2))
S_GRID = (1.0, 2.0, 3.0)


def advance_grid():
    """(phase, couple, mask, kT, tauS, dt, ndof, x, used, thermostat) of every case: the three phases, the five couples,
    three box_dof masks, kT, tauS, dt, Nf from 3 to 3 * 2^20 - 3, sums rows whose P_aa is x S_a (below, at, above), a fresh
    and a used state, each thermostat kind and none."""
    return list(itertools.product((ref.CLOSE, ref.OPEN, ref.CLOSE | ref.OPEN), ("none", "xy", "xz", "yz", "xyz"), (7, 5, 2),
                                  (0.5, 1.5), (0.1, 1.0), (0.001, 0.01), (3.0, 93.0, 3.0 * 2**20 - 3.0), (0.5, 1.0, 1.5),
                                  (False, True), THERMOSTATS))


def _case_inputs(case):
    phase, couple, mask, kT, tauS, dt, ndof, x, used, th = case
    V = (L_BOX[0] * L_BOX[1]) * L_BOX[2]
    row = np.zeros(_lib.THERMO_NSUMS)
    row[0] = (ndof + 3.0) / 3.0
    for a, (k, w) in enumerate(zip(ref.KAA, ref.WAA)):
        row[k] = ndof * kT / 3.0 * (1.0 + 0.01 * (a - 1))  # K = Nf kT / 2
        row[w] = x * S_GRID[a] * V - row[k]
    s0 = ref.new_state(nu=(0.3, -0.2, 0.1), ref_kT=kT) if used else ref.new_state()
    ts0 = None
    if th is not None:
        ts0 = dict(energy=-3.25, xi=0.3, eta=-0.2) if used else thermostat_ref.new_state()
    # (timestep, seed): the key of Bussi's draws, a function of the case
    return row, s0, ts0, 1000 + 37 * phase + int(round(dt * 1e4)) + (mask << 8) + int(ndof) % 1000, 7 + int(2 * kT) + 3 * ref.COUPLE[couple]


def _run_grid(cases, split=False):
    """Every case on the device, one launch each (``split``: a phase of close|open as two launches), one readback for
    all: (barostat states, thermostat states)."""
    import torch

    n = len(cases)
    state, rows, tstate = np.zeros((n, NS)), np.zeros((n, _lib.THERMO_NSUMS)), np.zeros((n, _lib.THERMOSTAT_NSTATE))
    for i, case in enumerate(cases):
        row, s0, ts0, _, _ = _case_inputs(case)
        rows[i] = row
        state[i, NU:NU + 3], state[i, _lib.BAROSTAT_REF_KT] = s0["nu"], s0["ref_kT"]
        if ts0 is not None:
            tstate[i, _lib.THERMOSTAT_ENERGY], tstate[i, _lib.THERMOSTAT_XI], tstate[i, _lib.THERMOSTAT_ETA] = ts0["energy"], ts0["xi"], ts0["eta"]
    d_state, d_rows, d_tstate = _dev(state), _dev(rows), _dev(tstate)
    lib, stream = _lib.lib(), _stream()
    a = _lib.BarostatArgs()
    a.N = 2
    a.box = _lib.make_box(L_BOX)
    a.S[:] = S_GRID
    for i, case in enumerate(cases):
        phase, couple, mask, kT, tauS, dt, ndof, x, used, th = case
        _, _, _, t, seed = _case_inputs(case)
        a.d_state = d_state.data_ptr() + i * 8 * NS
        a.d_sums = d_rows.data_ptr() + i * 8 * _lib.THERMO_NSUMS
        a.d_thermostat_state = d_tstate.data_ptr() + i * 8 * _lib.THERMOSTAT_NSTATE if th is not None else None
        a.dt, a.tauS, a.ndof, a.couple, a.box_dof, a.timestep = dt, tauS, ndof, ref.COUPLE[couple], mask, t
        if th is not None:
            a.thermostat_kind, a.thermostat_tau, a.thermostat_kT, a.thermostat_seed = th[0], th[1], kT, seed
        for ph in ((ref.CLOSE, ref.OPEN) if split and phase == (ref.CLOSE | ref.OPEN) else (phase,)):
            a.phase = ph
            _lib.check(lib.azp_barostat_advance(C.byref(a), stream), "azp_barostat_advance")
    torch.cuda.synchronize()
    return d_state.cpu().numpy(), d_tstate.cpu().numpy()


def advance_deviations(cases, got):
    """Per case the deviations of (nu, alpha, lambda, b, alpha_T, energy) from the reference, each relative to its scale."""
    dev = np.zeros((len(cases), 6))
    for i, case in enumerate(cases):
        phase, couple, mask, kT, tauS, dt, ndof, x, used, th = case
        row, s0, ts0, t, seed = _case_inputs(case)
        thermostat = None if th is None else dict(kind=th[0], kT=kT, tau=th[1], seed=seed, timestep=t, state=ts0)
        dof = tuple(bool(mask >> a & 1) for a in range(3))
        want = ref.advance(row, L_BOX, S_GRID, dt, tauS, ndof, couple, dof, phase, s0, thermostat)
        g = got[i]
        halves = bin(phase).count("1")
        g_mag = max((abs(row[k]) + abs(row[w]) + abs(want["V"] * S_GRID[a]) + 2.0 * want["K"] / ndof) / want["W"]
                    for a, (k, w) in enumerate(zip(ref.KAA, ref.WAA)))
        nu_scale = max(abs(v) for v in s0["nu"]) + halves * 0.5 * dt * g_mag
        dev[i, 0] = np.abs(g[NU:NU + 3] - want["nu"]).max() / nu_scale
        if phase & ref.OPEN:
            dev[i, 1] = (np.abs(g[ALPHA:ALPHA + 3] - want["alpha"]) / want["alpha"]).max()
            dev[i, 2] = (np.abs(g[LAMBDA:LAMBDA + 3] - want["lam"]) / want["lam"]).max()
            dev[i, 3] = (np.abs(g[B:B + 3] - want["b"]) / want["b"]).max()
            dev[i, 4] = abs(g[_lib.BAROSTAT_ALPHA_T] - want["alpha_T"]) / want["alpha_T"]
        dev[i, 5] = abs(g[_lib.BAROSTAT_ENERGY] - want["energy"]) / (want["energy"] or 1.0)
        # what goes through no library function is equal in every bit
        assert _bits(g[_lib.BAROSTAT_K]) == _bits(want["K"]) and _bits(g[_lib.BAROSTAT_V]) == _bits(want["V"])
        assert _bits(g[_lib.BAROSTAT_W]) == _bits(want["W"]) and _bits(g[_lib.BAROSTAT_REF_KT]) == _bits(want["ref_kT"])
        np.testing.assert_array_equal(_bits(g[_lib.BAROSTAT_P:_lib.BAROSTAT_P + 3]), _bits(want["P"]))
        for a in range(3):
            if not dof[a]:
                assert _bits(g[NU + a]) == _bits(0.0)
                if phase & ref.OPEN:
                    assert g[LAMBDA + a] == 1.0 and g[B + a] == dt
    return dev


def test_advance_over_the_grid():
    cases = advance_grid()
    got, got_ts = _run_grid(cases)
    assert np.all(np.isfinite(got)) and np.all(got[:, _lib.BAROSTAT_NONFINITE] == 0.0)
    dev = advance_deviations(cases, got)
    names = ("nu", "alpha", "lambda", "b", "alpha_T", "energy")
    print("%d cases, largest deviations: %s" % (len(cases), ", ".join("%s %.3g" % (n, d) for n, d in zip(names, dev.max(axis=0)))))
    print("largest deviation over the grid: %.3g (BARO_REL = %.3g)" % (dev.max(), ref.BARO_REL))
    # the couplings, in every bit
    for i, case in enumerate(cases):
        couple, mask = case[1], case[2]
        axes = [a for a in ref._COUPLED_AXES[couple] if mask >> a & 1]
        if len(axes) > 1 and not case[8]:  # (a fresh state: the coupled rates start equal)
            assert len({int(_bits(got[i, NU:NU + 3])[a]) for a in axes}) == 1, case
    # close|open in one launch is close then open
    both = [k for k, c in enumerate(cases) if c[0] == (ref.CLOSE | ref.OPEN)]
    two, two_ts = _run_grid([cases[k] for k in both], split=True)
    np.testing.assert_array_equal(_bits(two), _bits(got[both]))
    np.testing.assert_array_equal(_bits(two_ts), _bits(got_ts[both]))
    assert dev.max() <= 1e-10, "a deviation of this size is a bug, not a tolerance"
    worst = int(np.argmax(dev.max(axis=1)))
    assert dev.max() <= ref.BARO_REL, (cases[worst], dev[worst])


# ---------------------------------------------------------------------------------------------------------------------
# 3. runs of an ideal gas
# ---------------------------------------------------------------------------------------------------------------------
GAS_N, GAS_DT, GAS_L, GAS_TAUS = 32, 0.005, 10.0, 0.5
GAS_THERMOSTATS = {"nph": None, "berendsen": (thermostat_ref.BERENDSEN, 0.25), "bussi": (thermostat_ref.BUSSI, 0.1),
                   "mttk": (thermostat_ref.MTTK, 0.2)}
GAS_KT = 1.5


def _gas_start():
    rng = np.random.default_rng(77)
    pos = rng.uniform(-0.5 * GAS_L, 0.5 * GAS_L, (GAS_N, 3))
    vel = rng.normal(size=(GAS_N, 3))
    mass = rng.uniform(0.5, 2.0, GAS_N)
    K = 0.5 * float((mass[:, None] * vel * vel).sum())
    return pos, vel, mass, 0.5 * (2.0 * K / (3.0 * GAS_L**3))  # S = P(0) / 2


def _gas(kind, seed=5, recorder=True, couple="none"):
    import azplugins_amd as azp
    from azplugins_amd import compute, thermostats

    pos, vel, mass, S = _gas_start()
    snap = azp.Snapshot.from_arrays(pos, [GAS_L] * 3, velocity=vel)
    snap.particles.mass[:] = mass
    sim = azp.Simulation(device="cuda:0", seed=seed)
    sim.create_state_from_snapshot(snap)
    sim.operations.tuners.clear()  # (the reference sums in the snapshot's order)
    th = GAS_THERMOSTATS[kind]
    if th is not None:
        cls = {thermostat_ref.BERENDSEN: thermostats.Berendsen, thermostat_ref.BUSSI: thermostats.Bussi, thermostat_ref.MTTK: thermostats.MTTK}[th[0]]
        th = cls(kT=GAS_KT, tau=th[1])
    method = azp.ConstantPressure(azp.All(), S=S, tauS=GAS_TAUS, couple=couple, thermostat=th)
    sim.operations.integrator = azp.Integrator(dt=GAS_DT, forces=[], methods=[method])
    rec = None
    if recorder:
        thermo = compute.ThermodynamicQuantities(azp.All())
        sim.operations.add(thermo)
        rec = compute.ThermodynamicRecorder(thermo, azp.Periodic(1))
        sim.operations.add(rec)
    return sim, method, rec


def _ref_thermostat(kind):
    th = GAS_THERMOSTATS[kind]
    return None if th is None else dict(kind=th[0], kT=GAS_KT, tau=th[1])


def _host_vel(sim):
    v = sim.state.vel[: sim.state.N].cpu().numpy()
    return v[:, :3].copy(), v[:, 3].copy()


def _box_L(sim):
    b = sim.state.box
    return [b.Lx, b.Ly, b.Lz]


@pytest.mark.parametrize("kind", ["nph", "berendsen", "bussi", "mttk"])
def test_ideal_gas_follows_the_recurrence(kind):
    """200 steps without forces at S = P(0) / 2: K and V of every step through the recorder, nu, the box and the velocities
    of the end state, against the reference recurrence carried in the device's arithmetic, within 2 * steps * BARO_REL."""
    steps = 200
    sim, method, rec = _gas(kind)
    v0, mass = _host_vel(sim)
    S = method._S_at(0)
    sim.run(steps)
    assert sim.timestep == steps and rec.timesteps.tolist() == list(range(1, steps + 1))
    Ks, Vs, v_end, L_end, state, ts = ref.ideal_gas(v0, mass, [GAS_L] * 3, steps, S, GAS_DT, GAS_TAUS, thermostat=_ref_thermostat(kind),
                                                    seed=sim.seed)
    tol = 2 * steps * ref.BARO_REL
    table = rec.table
    rel_K = np.abs(table["kinetic_energy"] - Ks) / Ks
    rel_V = np.abs(table["volume"] - Vs) / Vs
    L = _box_L(sim)
    rel_L = max(abs(a - b) / b for a, b in zip(L, L_end))
    nu = method.barostat_dof
    rel_nu = max(abs(a - b) for a, b in zip(nu, state["nu"])) / max(abs(x) for x in state["nu"])
    got_v, _ = _host_vel(sim)
    rel_v = np.abs(got_v - v_end).max() / np.abs(v_end).max()
    print("%s: K within %.3g, V within %.3g, L within %.3g, nu within %.3g, v within %.3g (allowed %.3g); V grew by %.3f"
          % (kind, rel_K.max(), rel_V.max(), rel_L, rel_nu, rel_v, tol, Vs[-1] / GAS_L**3))
    assert max(rel_K.max(), rel_V.max(), rel_L, rel_nu, rel_v) <= tol
    assert abs(method.barostat_energy - state["energy"]) <= tol * state["energy"]
    if kind == "nph":
        assert method.reference_kT == state["ref_kT"] > 0.0
    else:
        assert method.reference_kT == 0.0
        assert abs(method.thermostat.energy - ts["energy"]) <= tol * (abs(ts["energy"]) + Ks[0]) + 0.0
    # the box did change, every axis, and the pressure above S pushed it outwards
    assert all(x > GAS_L * 1.001 for x in L) and table["volume"][-1] > table["volume"][0]


@pytest.mark.parametrize("kind", ["nph", "bussi", "mttk"])
def test_split_runs_and_seeds(kind):
    import torch

    def final(seed, chunks):
        sim, method, _ = _gas(kind, seed=seed, recorder=False)
        for n in chunks:
            sim.run(n)
        torch.cuda.synchronize()
        th = method.thermostat
        box = torch.tensor(_box_L(sim), dtype=torch.float64)
        return (sim.state.pos.clone(), sim.state.vel.clone(), sim.state.image.clone().to(torch.int64), box, method._state.clone(),
                th._state.clone() if th is not None else torch.zeros(1, dtype=torch.float64))

    def same(x, y):
        return all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip(x, y))

    whole = final(5, [20])
    assert same(whole, final(5, [10, 10])), "run(10); run(10) differs from run(20)"
    assert same(whole, final(5, [20])), "the same seed twice differs"
    assert same(whole, final(5, [1, 18, 1]))
    other = final(6, [20])
    assert same(whole, other) == (kind != "bussi")  # (only Bussi draws random numbers)


def test_barostat_dof_between_runs():
    """The step after ``barostat_dof`` is set starts from the new rates."""
    sim, method, _ = _gas("nph", recorder=False)
    sim.run(5)
    assert all(x != 0.0 for x in method.barostat_dof)
    method.barostat_dof = (0.1, -0.1, 0.05)
    assert method.barostat_dof == (0.1, -0.1, 0.05)
    v, mass = _host_vel(sim)
    L0 = _box_L(sim)
    start = ref.new_state(nu=(0.1, -0.1, 0.05), ref_kT=method.reference_kT)
    sim.run(1)
    _, _, v_end, L_end, state, _ = ref.ideal_gas(v, mass, L0, 1, method._S_at(0), GAS_DT, GAS_TAUS, state=start)
    tol = 2 * ref.BARO_REL
    L = _box_L(sim)
    assert L[1] < L0[1] and L[0] > L0[0]  # (nu_y < 0 shrinks y)
    assert max(abs(a - b) / b for a, b in zip(L, L_end)) <= tol
    assert max(abs(a - b) / abs(b) for a, b in zip(method.barostat_dof, state["nu"])) <= tol
    got_v, _ = _host_vel(sim)
    assert np.abs(got_v - v_end).max() <= tol * np.abs(v_end).max()
    # reference_kT can be set too: the mass of the next step's barostat follows it
    method.reference_kT = 2.0 * method.reference_kT
    sim.run(1)
    assert method._slots(_lib.BAROSTAT_W)[0] == ((3.0 * GAS_N) * method.reference_kT) * (GAS_TAUS * GAS_TAUS)


def test_a_gas_at_rest_is_refused():
    """Without kinetic energy and without a thermostat there is nothing to take reference_kT from: W = 0."""
    import azplugins_amd as azp

    sim, method, _ = _gas("nph", recorder=False)
    sim.state.vel[:, :3] = 0.0
    with pytest.raises(azp.AzpError, match="not finite"):
        sim.run(1)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the liquid
# ---------------------------------------------------------------------------------------------------------------------
LIQ_DT, LIQ_EVERY = 0.005, 100
# The barostat's time constant of the NPT runs. The mean of G_a over a window of duration T is (nu_end - nu_start) / T,
# so the window's mean pressure misses S by (W / V)(delta nu) / T (and by kT / V = 8e-4, the 2 K / Nf term): W grows with
# tauS^2, and 0.5 keeps the miss of a window of 10 time units below a hundredth for rates of a few hundredths.
LIQ_TAUS_NPT = 0.5


def _liquid(method):
    import azplugins_amd as azp
    from azplugins_amd import compute

    sim = azp.Simulation(device="cuda:0", seed=9)
    sim.create_state_from_snapshot(azp.lattice_snapshot(n=10, a=0.8 ** (-1.0 / 3.0)))  # N = 1000, rho* = 0.8
    sim.thermalize_particle_momenta(kT=1.0, seed=17)
    assert len(sim.operations.tuners) == 1  # (the particle sorter stays on)
    nl = azp.nlist.Cell(buffer=0.4)
    plj = azp.pair.PerturbedLennardJones(nlist=nl, default_r_cut=3.0, mode="shift")
    plj.params[("A", "A")] = dict(epsilon=1.0, sigma=1.0, attraction_scale_factor=0.5)
    sim.operations.integrator = azp.Integrator(dt=LIQ_DT, forces=[plj], methods=[method])
    thermo = compute.ThermodynamicQuantities(azp.All())
    sim.operations.add(thermo)
    rec = compute.ThermodynamicRecorder(thermo, azp.Periodic(1))
    sim.operations.add(rec)
    return sim, thermo, rec


def _run_liquid(method, steps, S=None):
    """``steps`` steps; the conserved quantity every LIQ_EVERY steps (K + U, + S V + the barostat's energy, + the
    thermostat's), the recorder's table, the growth of the total momentum."""
    import azplugins_amd as azp

    sim, thermo, rec = _liquid(method)
    baro = isinstance(method, azp.ConstantPressure)
    th = method.thermostat

    def extra():
        e = th.energy if th is not None else 0.0
        if baro:
            e += S * sim.state.box.volume + method.barostat_energy
        return e

    sim.run(0)
    E = [thermo.kinetic_energy + thermo.potential_energy + extra()]
    P0 = np.asarray(thermo.linear_momentum)
    V0 = sim.state.box.volume
    extras = []
    for _ in range(steps // LIQ_EVERY):
        sim.run(LIQ_EVERY)
        extras.append(extra())
    table = rec.table
    total = table["kinetic_energy"] + table["potential_energy"]
    E = np.array(E + [total[(k + 1) * LIQ_EVERY - 1] + extras[k] for k in range(len(extras))])
    return dict(N=sim.state.N, V0=V0, drift=np.abs(E - E[0]).max() / sim.state.N, table=table,
                momentum=np.linalg.norm(table["linear_momentum"] - P0, axis=1).max(), sorts=sim.operations.tuners[0].num_sorts,
                box=sim.state.box)


def _block_se(x, blocks_in_window):
    """The standard deviation of the means of LIQ_EVERY-step blocks of x, divided by sqrt(blocks in the NPT window)."""
    means = x.reshape(-1, LIQ_EVERY).mean(axis=1)
    return means.std(ddof=1) / math.sqrt(blocks_in_window)


@pytest.fixture(scope="module")
def liquid_runs():
    """The yardsticks, which run code that exists without the barostat (NVE: the drift and the momentum growth; NVT with
    Bussi at kT = 1: P0 and the standard errors), then NPH at S = P0 and NPT at S = P0 + 1, coupled and uncoupled."""
    import azplugins_amd as azp
    from azplugins_amd import thermostats

    out = {}
    out["nve"] = _run_liquid(azp.ConstantVolume(), 2000)
    nvt = out["nvt"] = _run_liquid(azp.ConstantVolume(thermostat=thermostats.Bussi(kT=1.0, tau=100 * LIQ_DT)), 2000)
    P = nvt["table"]["pressure"][-1000:]
    Paa = nvt["table"]["pressure_tensor"][-1000:][:, [0, 3, 5]]
    window_blocks = 2000 // LIQ_EVERY
    P0 = out["P0"] = float(P.mean())
    out["se"] = float(_block_se(P, window_blocks))
    out["se_aa"] = [float(_block_se(Paa[:, a], window_blocks)) for a in range(3)]
    print("NVT: P0 = %.4f, se = %.4g, se_aa = %s" % (P0, out["se"], out["se_aa"]))
    out["nph"] = _run_liquid(azp.ConstantPressure(azp.All(), S=P0, tauS=1.0, couple="xyz"), 2000, S=P0)
    for name, couple in (("npt", "xyz"), ("npt_none", "none")):
        th = thermostats.Bussi(kT=1.0, tau=100 * LIQ_DT)
        out[name] = _run_liquid(azp.ConstantPressure(azp.All(), S=P0 + 1.0, tauS=LIQ_TAUS_NPT, couple=couple, thermostat=th), 3000, S=P0 + 1.0)
    for name in ("nve", "nvt", "nph", "npt", "npt_none"):
        r = out[name]
        print("%s: drift per particle %.4g, momentum growth %.3g, mean P of the last 1000 steps %.4f, V / V0 at the end %.4f, %d sorts"
              % (name, r["drift"], r["momentum"], r["table"]["pressure"][-1000:].mean(), r["box"].volume / r["V0"], r["sorts"]))
    return out


def test_liquid_nph_conserves_its_energy(liquid_runs):
    nve, nph = liquid_runs["nve"], liquid_runs["nph"]
    assert nph["N"] == 1000 and nph["sorts"] >= 1 and nve["drift"] > 0.0
    assert np.ptp(nph["table"]["volume"]) > 1e-3 * nph["V0"]  # the box did move
    assert nph["drift"] <= 4.0 * nve["drift"], (nph["drift"], nve["drift"])


def test_liquid_npt_reaches_the_pressure(liquid_runs):
    S, se = liquid_runs["P0"] + 1.0, liquid_runs["se"]
    t = liquid_runs["npt"]["table"]
    assert len(t["pressure"]) == 3000 and se > 0.0
    P, V = t["pressure"][-2000:].mean(), t["volume"][-2000:].mean()
    print("NPT: mean P %.4f against S = %.4f (5 se = %.4g), mean V / V0 = %.4f" % (P, S, 5.0 * se, V / liquid_runs["npt"]["V0"]))
    assert abs(P - S) <= 5.0 * se, (P, S, se)
    assert 0.5 * liquid_runs["npt"]["V0"] < V < liquid_runs["npt"]["V0"]
    b = liquid_runs["npt"]["box"]
    assert b.Lx == b.Ly == b.Lz  # couple "xyz": a cube stays a cube, in every bit


def test_liquid_uncoupled_axes_reach_the_pressure(liquid_runs):
    S = liquid_runs["P0"] + 1.0
    Paa = liquid_runs["npt_none"]["table"]["pressure_tensor"][-2000:][:, [0, 3, 5]].mean(axis=0)
    print("NPT, couple none: mean P_aa %s against S = %.4f (5 se_aa = %s)" % (Paa, S, [5.0 * x for x in liquid_runs["se_aa"]]))
    for a in range(3):
        assert abs(Paa[a] - S) <= 5.0 * liquid_runs["se_aa"][a], (a, Paa[a], S, liquid_runs["se_aa"][a])
    b = liquid_runs["npt_none"]["box"]
    assert len({b.Lx, b.Ly, b.Lz}) == 3  # each axis went its own way


@pytest.mark.parametrize("name", ["nph", "npt", "npt_none"])
def test_liquid_momentum(liquid_runs, name):
    assert liquid_runs[name]["momentum"] <= 4.0 * liquid_runs["nve"]["momentum"], (liquid_runs[name]["momentum"], liquid_runs["nve"]["momentum"])


# ---------------------------------------------------------------------------------------------------------------------
# 5. ConstantVolume is what it was
# ---------------------------------------------------------------------------------------------------------------------
def test_constant_volume_is_unchanged():
    import torch

    import azplugins_amd as azp

    finals = []
    keep = None
    for with_barostat in (False, True):
        if with_barostat:
            keep = azp.ConstantPressure(azp.All(), S=1.0, tauS=1.0, couple="xyz")  # exists, in no integrator
        sim, thermo, rec = _liquid(azp.ConstantVolume())
        sim.operations.remove(rec)
        sim.operations.remove(thermo)
        sim.run(50)
        torch.cuda.synchronize()
        # without a barostat or a thermo compute no virial pass runs
        assert sim.operations.integrator.forces[0].compute_virial is False
        finals.append((sim.state.pos.clone(), sim.state.vel.clone(), sim.state.image.clone().to(torch.int64)))
    assert keep is not None
    for a, b in zip(*finals):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    # and with a barostat it does
    sim, thermo, rec = _liquid(azp.ConstantPressure(azp.All(), S=1.0, tauS=1.0, couple="xyz"))
    sim.operations.remove(rec)
    sim.operations.remove(thermo)
    sim.run(2)
    assert sim.operations.integrator.forces[0].compute_virial is True
