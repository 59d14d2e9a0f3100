"""methods.Langevin / methods.Brownian without a GPU: constructor validation, the gamma and gamma_r tables, every refusal
of the driver (on the stand-ins of tests/test_step_loop.py), the order of the launches with rotation, the C ABI, and the
numpy restatement (tests/langevin_ref.py) on its own: against the oracle's NO_SQUISH step, and against the two statistical
bounds that the GPU tests put on the kernels (so that the bounds are the scheme's, not only the kernel's)."""

import ctypes as C
import os
import subprocess
import tempfile
import warnings

import numpy as np
import pytest

import langevin_ref as ref
import test_step_loop as loop
from azplugins_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------
# the classes
# ---------------------------------------------------------------------------
def test_exports_and_defaults():
    import azplugins_amd as azp
    from azplugins_amd import methods

    assert azp.Langevin is methods.Langevin and azp.Brownian is methods.Brownian
    assert azp.methods.ConstantVolume is azp.ConstantVolume
    for cls in (methods.Langevin, methods.Brownian):
        m = cls(filter=azp.All(), kT=1.5)
        assert m.gamma.default == 1.0 and m.gamma_r.default == (1.0, 1.0, 1.0)
        assert m._fusable and m._updaters_split
        assert m._kT(7) == 1.5
    m = methods.Langevin(azp.Type("A"), kT=lambda t: 1.0 + t, tally_reservoir_energy=False)
    assert m._kT(3) == 4.0 and m.tally_reservoir_energy is False


def test_constructor_validation():
    from azplugins_amd import All, Type, methods

    with pytest.raises(_lib.AzpError, match="tally_reservoir_energy.*reduction"):
        methods.Langevin(All(), kT=1.0, tally_reservoir_energy=True)
    for cls in (methods.Langevin, methods.Brownian):
        with pytest.raises(_lib.AzpError, match="filter"):
            cls(filter="all", kT=1.0)
        for bad_kT in (-1.0, np.nan, np.inf):
            with pytest.raises(_lib.AzpError, match="kT"):
                cls(All(), kT=bad_kT)
        cls(All(), kT=0.0)  # the noiseless run
        for bad in (-0.5, np.nan, np.inf):
            with pytest.raises(_lib.AzpError):
                cls(All(), kT=1.0, default_gamma=bad)
            with pytest.raises(_lib.AzpError):
                cls(All(), kT=1.0, default_gamma_r=(1.0, bad, 1.0))
        for malformed in (1.0, (1.0, 2.0), (1.0, 2.0, 3.0, 4.0)):
            with pytest.raises(_lib.AzpError, match="three values"):
                cls(All(), kT=1.0, default_gamma_r=malformed)
        assert not hasattr(cls(All(), kT=1.0), "noiseless")  # kT = 0 is the noiseless run
    # Langevin takes 0, Brownian divides by its coefficients
    lan = methods.Langevin(Type("A"), kT=1.0, default_gamma=0.0, default_gamma_r=(0.0, 0.0, 0.0))
    lan.gamma["A"] = 0.0
    lan.gamma_r["A"] = (0.0, 1.0, 0.0)
    bro = methods.Brownian(All(), kT=1.0)
    with pytest.raises(_lib.AzpError, match="> 0"):
        methods.Brownian(All(), kT=1.0, default_gamma=0.0)
    with pytest.raises(_lib.AzpError, match="> 0"):
        methods.Brownian(All(), kT=1.0, default_gamma_r=(1.0, 1.0, 0.0))
    with pytest.raises(_lib.AzpError, match="> 0"):
        bro.gamma["A"] = 0.0
    with pytest.raises(_lib.AzpError, match="> 0"):
        bro.gamma_r["A"] = (2.0, 0.0, 2.0)
    assert bro.gamma_r["A"] == (1.0, 1.0, 1.0)  # a refused value is not stored


def test_gamma_tables():
    from azplugins_amd import All, methods

    m = methods.Langevin(All(), kT=1.0, default_gamma=0.5, default_gamma_r=(0.1, 0.2, 0.3))
    m.gamma["B"] = 2.0
    m.gamma_r[["A", "C"]] = (1, 2, 3)
    types = ["A", "B", "C", "D"]
    np.testing.assert_array_equal(m.gamma.table(types), [0.5, 2.0, 0.5, 0.5])
    want = np.array([[1, 2, 3], [0.1, 0.2, 0.3], [1, 2, 3], [0.1, 0.2, 0.3]], dtype=np.float64)
    np.testing.assert_array_equal(m.gamma_r.table(types), want)
    g, g_r = m._gamma_tables(types)
    assert g.dtype == np.float64 and g.shape == (4,) and g_r.dtype == np.float64 and g_r.shape == (4, 3) and g_r.flags.c_contiguous
    assert m.gamma["Z"] == 0.5 and m.gamma_r["Z"] == (0.1, 0.2, 0.3)


# ---------------------------------------------------------------------------
# the driver, on the stand-ins of test_step_loop
# ---------------------------------------------------------------------------
def _sim(methods, monkeypatch, rot=False, seed=1, **kw):
    sim, log = loop.make_sim("nve", monkeypatch, seed=seed, **kw)
    sim.state.langevin_torque = None
    integ = sim.operations.integrator
    integ.methods = methods
    integ.integrate_rotational_dof = rot
    return sim, log


def test_refusals_come_ahead_of_the_forces_at_zero_steps(monkeypatch):
    import azplugins_amd as azp
    from azplugins_amd import All, Type, flow, methods, minimize, thermostats

    u = flow.ConstantFlow(velocity=(0, 0, 0))

    def lan(f):
        return methods.Langevin(f, kT=1.0)

    def bro(f):
        return methods.Brownian(f, kT=1.0)

    same = lan(All())
    cases = [
        ([lan(All()), azp.ConstantVolume()], {}, "cannot be mixed"),
        ([azp.ConstantVolume(thermostat=thermostats.Bussi(kT=1.0, tau=0.5)), bro(Type("A"))], {}, "cannot be mixed"),
        ([lan(Type("A")), azp.ConstantPressure(All(), S=1.0, tauS=1.0, couple="xyz")], {}, "only method|cannot be mixed"),
        ([lan(Type(["A", "B"])), bro(Type("B"))], {}, "overlap"),
        ([lan(Type("A")), flow.Brownian(Type("A"), kT=1.0, flow_field=u)], {}, "overlap"),
        ([lan(All()), bro(Type("A"))], {}, r"All\(\) must be the only"),
        ([flow.Langevin(Type("A"), kT=1.0, flow_field=u), lan(All())], {}, r"All\(\) must be the only"),
        ([same, same], {}, "twice"),
        ([lan(Type("Z"))], {}, "Z"),
        ([lan(Type("A")), flow.Langevin(Type("B"), kT=1.0, flow_field=u)], dict(rot=True), "flow.*rotational"),
    ]
    for ms, kw, match in cases:
        sim, log = _sim(ms, monkeypatch, **kw)
        with pytest.raises(_lib.AzpError, match=match):
            sim.run(0)
        assert log == [], ms
    # decomposed runs: the stored accelerations and torques do not migrate
    for m in (lan(All()), bro(All())):
        sim, log = _sim([m], monkeypatch)
        sim.domain = loop._Domain(log)
        with pytest.raises(_lib.AzpError, match="decomposed.*do not migrate"):
            sim.run(0)
        assert log == []
    # the minimizer takes ConstantVolume only
    sim, log = _sim([], monkeypatch)
    forces = sim.operations.integrator.forces
    sim.operations.integrator = minimize.FIRE(dt=loop.DT, force_tol=1e-3, angmom_tol=1e-3, energy_tol=1e-7, forces=forces,
                                              methods=[lan(All())])
    with pytest.raises(_lib.AzpError):
        sim.run(0)
    assert log == []
    # what can run together, with and without rotation (flow methods: without)
    ok = [([lan(All())], True), ([bro(All())], True), ([lan(Type("A")), bro(Type("B"))], True),
          ([lan(Type("A")), flow.Langevin(Type("B"), kT=1.0, flow_field=u)], False),
          ([flow.Brownian(Type("A"), kT=1.0, flow_field=u), bro(Type("B"))], False)]
    for ms, rot in ok:
        sim, log = _sim(ms, monkeypatch, rot=rot)
        assert sim._check_flow_methods(sim.operations.integrator) == ms
        sim.run(0)
        assert len([e for e in log if ".compute(" in e and not e.startswith("nlist")]) == 2


def _launches(log):
    return [e for e in log if e.startswith("azp_integrate")]


def test_launch_order_with_rotation(monkeypatch):
    """One launch per half step moves and rotates (no azp_integrate_nve_rot_* next to it); step two of step t - 1 and step
    one of step t are one launch with the kT and the random numbers of t - 1, split where a writer is due (3, 6) or an
    updater that changes types (4); langevin_torque starts as zeros and stays the same tensor over the runs."""
    from azplugins_amd import All, methods

    kT_log = []
    m = methods.Langevin(All(), kT=loop._kT(kT_log))
    sim, log = _sim([m], monkeypatch, rot=True)
    sim.run(7)
    assert not any(e.endswith("STALE") for e in log)
    one, two, two_one = ("azp_integrate_langevin_step_%s timestep=%%d kT=%%r dt=0.005 N=6" % s for s in ("one", "two", "two_one"))
    kT = lambda t: 1.0 + 0.125 * t  # noqa: E731
    want = [one % (0, kT(0)), two_one % (0, kT(0)), two_one % (1, kT(1)), two % (2, kT(2)), one % (3, kT(3)),
            two % (3, kT(3)), one % (4, kT(4)), two_one % (4, kT(4)), two % (5, kT(5)), one % (6, kT(6)), two % (6, kT(6))]
    assert _launches(log) == want
    st = sim.state
    assert m._args.rotational == 1 and m._args.d_langevin_torque == st.langevin_torque.data_ptr()
    assert m._args.d_orientation == st.orientation.data_ptr() and m._args.d_inertia == st.inertia.data_ptr()
    assert st.langevin_torque.shape == (loop.N, 4) and not st.langevin_torque.any()
    assert st.accel is not None and st.accel.shape == (loop.N, 4)
    # (the two forces of the stand-in: the net torque is their sum, a tensor of its own)
    assert m._args.d_net_torque not in (f.torque_tensor.data_ptr() for f in sim.operations.integrator.forces)
    torque = st.langevin_torque
    sim.run(1)
    assert st.langevin_torque is torque


def test_brownian_and_no_rotation_launches(monkeypatch):
    from azplugins_amd import Type, methods

    lan, bro = methods.Langevin(Type("A"), kT=1.0), methods.Brownian(Type("B"), kT=2.0)
    sim, log = _sim([lan, bro], monkeypatch, rot=False, writer=0, updater=0)
    sim.run(2)
    assert [e.split()[0] for e in _launches(log)] == [
        "azp_integrate_langevin_step_one", "azp_integrate_brownian_step", "azp_integrate_langevin_step_two_one",
        "azp_integrate_brownian_step", "azp_integrate_langevin_step_two"]
    for m in (lan, bro):  # without integrate_rotational_dof the rotational arrays are not handed over
        a = m._args
        assert a.rotational == 0 and not any((a.d_orientation, a.d_angmom, a.d_inertia, a.d_net_torque, a.d_langevin_torque))
    assert sim.state.langevin_torque is None
    # Brownian with rotation: no angular momenta, no stored torques
    sim, log = _sim([methods.Brownian(Type("B"), kT=2.0)], monkeypatch, rot=True, writer=0, updater=0)
    sim.run(1)
    a = sim.operations.integrator.methods[0]._args
    assert a.rotational == 1 and a.d_orientation and a.d_langevin_torque is None and sim.state.langevin_torque is None
    assert sim.state.accel is None


def test_seed_warning_follows_the_first_forces(monkeypatch):
    from azplugins_amd import All, methods

    sim, log = _sim([methods.Langevin(All(), kT=1.0)], monkeypatch, rot=True, seed=None)
    with warnings.catch_warnings():
        warnings.simplefilter("always")
        monkeypatch.setattr(warnings, "showwarning", lambda message, *a, **k: log.append("warning: %s" % message))
        sim.run(0)
        assert not any(e.startswith("warning") for e in log)
        sim.run(1)
    k = [i for i, e in enumerate(log) if e.startswith("warning")]
    assert len(k) == 1 and "seed" in log[k[0]] and sim.seed == 0 and log[k[0] - 1].startswith("azp_sum_forces")
    assert not _launches(log[: k[0]]) and _launches(log[k[0]:])


# ---------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------
def test_abi_struct_layout():
    fields = [name for name, _ in _lib.LangevinArgs._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "azp.h"\nint main(){printf("%zu\\n", sizeof(azp_langevin_args));' + "".join(
        'printf("%%zu\\n", offsetof(azp_langevin_args, %s));' % f for f in fields) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "s.c"), "w") as f:
            f.write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    assert got[0] == C.sizeof(_lib.LangevinArgs)
    for k, f in enumerate(fields):
        assert got[1 + k] == getattr(_lib.LangevinArgs, f).offset, f


ENTRIES = ("azp_integrate_langevin_step_one", "azp_integrate_langevin_step_two", "azp_integrate_langevin_step_two_one",
           "azp_integrate_brownian_step")


def test_abi_entries_check_their_arguments():
    """Every refusal is made on the host, ahead of any launch: null struct, missing arrays, dt, block size; N = 0 succeeds."""
    lib = _lib.lib()
    buf = (C.c_double * 64)()  # (never read: every call below is refused, or has nothing to do)
    p = C.addressof(buf)

    def full(rot):
        a = _lib.LangevinArgs()
        for name in ("d_pos", "d_vel", "d_accel", "d_net_force", "d_tag", "d_gamma"):
            setattr(a, name, p)
        if rot:
            for name in ("d_orientation", "d_angmom", "d_inertia", "d_net_torque", "d_langevin_torque", "d_gamma_r"):
                setattr(a, name, p)
        a.rotational, a.N, a.ntypes, a.dt = int(rot), 4, 1, 0.005
        return a

    for name in ENTRIES:
        fn = getattr(lib, name)
        brownian, one = name.endswith("brownian_step"), name.endswith("step_one")
        assert fn(None, None) == -1
        assert fn(C.byref(_lib.LangevinArgs()), None) == 0  # N = 0: nothing to do
        for rot in (False, True):
            needed = ["d_pos"]
            if not one:
                needed += ["d_net_force", "d_tag", "d_gamma"]
            if not brownian:
                needed += ["d_vel", "d_accel"]
            if rot:
                needed += ["d_orientation", "d_inertia", "d_net_torque"] + ([] if one else ["d_gamma_r"])
                if not brownian:
                    needed += ["d_angmom", "d_langevin_torque"]
            for missing in needed:
                a = full(rot)
                setattr(a, missing, None)
                assert fn(C.byref(a), None) == -1, (name, rot, missing)
            for field, bad in (("dt", 0.0), ("dt", -0.005), ("dt", float("nan")), ("ntypes", 0), ("block_size", 32),
                               ("block_size", 96), ("block_size", 320), ("block_size", 512)):
                a = full(rot)
                setattr(a, field, bad)
                assert fn(C.byref(a), None) == -1, (name, rot, field, bad)
            a = full(rot)
            a.N = 0
            assert fn(C.byref(a), None) == 0


# ---------------------------------------------------------------------------
# the numpy restatement on its own
# ---------------------------------------------------------------------------
def _tops(n, seed):
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    p = rng.normal(size=(n, 4))
    I = rng.uniform(0.2, 1.5, size=(n, 3))
    I[::7, 2] = 0.0
    I[::11, 0] = 0.0
    tau = rng.normal(size=(n, 3))
    return q, p, I, tau


def test_quaternion_algebra():
    q, p, _, tau = _tops(64, 1)
    # rotate() against the rotation matrix of q, and body() as its inverse
    s, x, y, z = q.T
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - s * z), 2 * (x * z + s * y)],
                  [2 * (x * y + s * z), 1 - 2 * (x * x + z * z), 2 * (y * z - s * x)],
                  [2 * (x * z - s * y), 2 * (y * z + s * x), 1 - 2 * (x * x + y * y)]]).transpose(2, 0, 1)
    np.testing.assert_allclose(ref.rotate(q, tau), np.einsum("nij,nj->ni", R, tau), atol=1e-14)
    np.testing.assert_allclose(ref.body(q, ref.rotate(q, tau)), tau, atol=1e-14)
    # a kick by T changes the body angular momentum by dt T / 2: the half kick
    T = np.random.default_rng(2).normal(size=(64, 3))
    np.testing.assert_allclose(ref.body_angmom(q, ref.kick(q, p, T, 0.01)) - ref.body_angmom(q, p), 0.005 * T, atol=1e-14)


def test_reference_rotation_is_the_oracle_step_with_the_effective_torque(oracle):
    """One Langevin step of the restatement equals oracle.nve_rot_step fed the space-frame torque tau + rotate(q, b): in
    step one with the stored b, in step two with the b that step two computes."""
    n, dt, kT, seed = 1000, 0.004, 1.3, 9
    q, p, I, tau = _tops(n, 3)
    rng = np.random.default_rng(4)
    b = np.where(I != 0.0, rng.normal(size=(n, 3)), 0.0)
    gamma_r = rng.uniform(0.0, 3.0, size=(n, 3))
    tag = rng.permutation(n).astype(np.uint32)
    sel = np.ones(n, bool)

    def t4(t):
        return np.concatenate([t, np.zeros((n, 1))], axis=1)

    for t in range(3):
        q1, p1 = ref.langevin_rot_step_one(q, p, I, tau, b, dt, sel)
        qo, po = oracle.nve_rot_step(True, q, p, I, t4(tau + ref.rotate(q, b)), dt)
        assert np.abs(q1 - qo).max() < 1e-12 and np.abs(p1 - po).max() < 1e-12 * max(1.0, np.abs(po).max())
        q, p = q1, p1
        tau = rng.normal(size=(n, 3))
        p2, b = ref.langevin_rot_step_two(q, p, I, tau, tag, gamma_r, kT, dt, seed, t, sel)
        assert np.all(b[I == 0.0] == 0.0) and np.abs(b).max() > 1.0
        qo, po = oracle.nve_rot_step(False, q, p, I, t4(tau + ref.rotate(q, b)), dt)
        assert np.array_equal(qo, q) and np.abs(p2 - po).max() < 1e-12 * max(1.0, np.abs(po).max())
        p = p2
    # gamma_r = 0: b = 0 whatever kT, and the step is the oracle's NVE step
    p2, b = ref.langevin_rot_step_two(q, p, I, tau, tag, np.zeros((n, 3)), kT, dt, seed, 5, sel)
    assert not b.any()
    assert np.abs(p2 - oracle.nve_rot_step(False, q, p, I, t4(tau), dt)[1]).max() < 1e-12 * np.abs(p2).max()


def test_reference_leaves_unselected_rows_alone():
    n = 64
    q, p, I, tau = _tops(n, 5)
    sel = np.arange(n) % 3 != 1
    tag = np.arange(n, dtype=np.uint32)
    g = np.full((n, 3), 2.0)
    b0 = np.full((n, 3), 0.25)
    q1, p1 = ref.langevin_rot_step_one(q, p, I, tau, b0, 0.01, sel)
    p2, _ = ref.langevin_rot_step_two(q, p, I, tau, tag, g, 1.0, 0.01, 1, 0, sel)
    q3 = ref.brownian_rot_step(q, I, tau, tag, g, 1.0, 0.01, 1, 0, sel)
    for got, was in ((q1, q), (p1, p), (p2, p), (q3, q)):
        assert np.array_equal(got[~sel], was[~sel]) and not np.array_equal(got[sel], was[sel])
    # Brownian, nothing to turn a particle: q keeps its bits
    still = ref.brownian_rot_step(q, I, np.zeros((n, 3)), tag, g, 0.0, 0.01, 1, 0, np.ones(n, bool))
    assert np.array_equal(still, q)


def planar_rotors(n):
    """q = identity, p = 0, I = (0, 0, 1), no torque."""
    q = np.tile([1.0, 0.0, 0.0, 0.0], (n, 1))
    return q, np.zeros((n, 4)), np.tile([0.0, 0.0, 1.0], (n, 1)), np.zeros((n, 3))


def test_reference_langevin_rotor_statistics():
    """Planar rotors: the half-step S_z is AR(1) with factor 1 - g dt / I, and the full-step variance is exactly kT I_z
    (DESIGN 4.25), so the mean of S_z^2 / I_z over 4 samples 10 relaxation times apart lies within 5 sigma of a chi-square
    with 4 N degrees of freedom: the bound of the GPU test, met by the scheme itself."""
    N, kT, g, dt = 4096, 1.5, 2.0, 0.01
    q, p, I, tau = planar_rotors(N)
    b = np.zeros((N, 3))
    tag, sel, gamma_r = np.arange(N, dtype=np.uint32), np.ones(N, bool), np.tile([0.0, 0.0, g], (N, 1))
    samples = []
    for t in range(1000 + 4 * 500):
        q, p = ref.langevin_rot_step_one(q, p, I, tau, b, dt, sel)
        p, b = ref.langevin_rot_step_two(q, p, I, tau, tag, gamma_r, kT, dt, 5, t, sel)
        if t + 1 > 1000 and (t + 1 - 1000) % 500 == 0:
            samples.append(np.mean(ref.body_angmom(q, p)[:, 2] ** 2 / I[:, 2]))
    assert len(samples) == 4
    assert abs(np.mean(samples) - kT) < 5 * kT * np.sqrt(2.0 / (4 * N)), samples
    assert not b[:, :2].any() and not ref.body_angmom(q, p)[:, :2].any()  # the axes without inertia stay out of it
    np.testing.assert_allclose(np.linalg.norm(q, axis=1), 1.0, atol=1e-14)


def test_reference_brownian_rotor_statistics():
    """Planar rotors: theta = 2 atan2(q_z, q_s) after time t has the variance 2 kT t / gamma_r = 0.25 (within 5 sqrt(2 / N)
    relative) and the mean 0 (within 5 sqrt(var / N)); 5 sigma = 2.5 < pi, nothing to unwrap."""
    N, kT, g, dt, steps = 4096, 1.0, 2.0, 0.005, 50
    q, _, I, tau = planar_rotors(N)
    tag, sel, gamma_r = np.arange(N, dtype=np.uint32), np.ones(N, bool), np.tile([1.0, 1.0, g], (N, 1))
    for t in range(steps):
        q = ref.brownian_rot_step(q, I, tau, tag, gamma_r, kT, dt, 5, t, sel)
    theta = 2.0 * np.arctan2(q[:, 3], q[:, 0])
    var = 2.0 * kT * steps * dt / g
    assert var == 0.25
    assert abs(np.var(theta) / var - 1.0) < 5 * np.sqrt(2.0 / N), np.var(theta)
    assert abs(np.mean(theta)) < 5 * np.sqrt(var / N), np.mean(theta)
    assert not q[:, 1:3].any()
