"""methods.Langevin / methods.Brownian on the GPU (csrc/langevin.hip): the four entry points against the numpy restatement
(tests/langevin_ref.py); the translation pinned bit for bit to flow.Langevin / flow.Brownian at zero flow and the rotation
to the NVE kernels; one step through Simulation.run with TwoPatchMorse forces and torques; split, repeated and sorted runs;
type filters; a recorder due mid-run; a flow method next to a methods one; the statistics of both schemes on planar rotors;
and one full-size C5 run."""

import ctypes as C

import numpy as np
import pytest

import langevin_ref as ref
from azplugins_amd import synthetic as syn

pytestmark = pytest.mark.gpu

TOL = 1e-12
TPM_SOFT = dict(M_d=1.0, M_r=0.25, r_eq=1.1, omega=5.0, alpha=0.4, repulsion=True)  # (the well of the NVE energy test)


def _close(got, want, what, tol=TOL):
    scale = max(np.abs(want).max(), 1e-300)
    err = np.abs(got - want).max()
    assert err <= tol * scale, "%s differs by %g (scale %g)" % (what, err, scale)


# ---------------------------------------------------------------------------
# the entry points, called directly
# ---------------------------------------------------------------------------
N_K, L_K, DT_K, KT_K, SEED_K = 1000, 9.0, 0.004, 1.3, 0x1234
MASK_K = np.array([1, 0, 1], dtype=np.uint8)
GAMMA_K = np.array([0.7, 5.0, 2.5])
GAMMA_R_K = np.array([[0.3, 0.6, 0.9], [5.0, 5.0, 5.0], [1.1, 0.0, 2.2]])
GAMMA_R_BROWNIAN = np.array([[0.3, 0.6, 0.9], [5.0, 5.0, 5.0], [1.1, 0.4, 2.2]])


def _kernel_state():
    """Random particles near and across the faces of a box, with masses, orientations, angular momenta, forces, torques,
    stored accelerations and Langevin torques; every 7th / 11th row without a z / x moment; three types."""
    rng = np.random.default_rng(21)
    n = N_K
    h = dict(pos=rng.uniform(-0.5 * L_K, 0.5 * L_K, (n, 3)), vel=3.0 * rng.normal(size=(n, 3)), mass=rng.uniform(0.5, 2.0, n),
             accel=rng.normal(size=(n, 3)), image=rng.integers(-2, 3, (n, 3)).astype(np.int32),
             tag=rng.permutation(n).astype(np.uint32), typeid=rng.integers(0, 3, n), p=rng.normal(size=(n, 4)))
    q = rng.normal(size=(n, 4))
    h["q"] = q / np.linalg.norm(q, axis=1)[:, None]
    I = rng.uniform(0.2, 1.5, size=(n, 3))
    I[::7, 2] = 0.0
    I[::11, 0] = 0.0
    h["I"] = I
    h["b"] = np.where(I != 0.0, rng.normal(size=(n, 3)), 0.0)
    h["force"] = 20.0 * rng.normal(size=(n, 3))
    h["torque"] = rng.normal(size=(n, 3))
    return h


def _pad4(x, w=0.0):
    return np.ascontiguousarray(np.c_[x, np.broadcast_to(w, x.shape[0])], dtype=np.float64)


class _Device:
    """The arrays of a host state on the device, and an argument struct pointed at them."""

    def __init__(self, h, gamma_r, rot=True, block_size=0):
        import torch

        from azplugins_amd import _lib

        dev = "cuda:0"
        t = self.t = dict(
            pos=torch.from_numpy(syn.pos4(h["pos"], h["typeid"])), vel=torch.from_numpy(_pad4(h["vel"], h["mass"])),
            accel=torch.from_numpy(_pad4(h["accel"])), force=torch.from_numpy(_pad4(h["force"], 7.0)),
            image=torch.from_numpy(h["image"].copy()), tag=torch.from_numpy(h["tag"].view(np.int32).copy()),
            q=torch.from_numpy(h["q"].copy()), p=torch.from_numpy(h["p"].copy()), I=torch.from_numpy(h["I"].copy()),
            torque=torch.from_numpy(_pad4(h["torque"])), b=torch.from_numpy(_pad4(h["b"])),
            gamma=torch.from_numpy(GAMMA_K.copy()), gamma_r=torch.from_numpy(np.ascontiguousarray(gamma_r)),
            mask=torch.from_numpy(MASK_K.copy()))
        for k in t:
            t[k] = t[k].to(dev)
        a = self.a = _lib.LangevinArgs()
        a.d_pos, a.d_vel, a.d_accel, a.d_net_force = (t[k].data_ptr() for k in ("pos", "vel", "accel", "force"))
        a.d_image, a.d_tag, a.d_gamma, a.d_type_mask = (t[k].data_ptr() for k in ("image", "tag", "gamma", "mask"))
        if rot:
            a.d_orientation, a.d_angmom, a.d_inertia = (t[k].data_ptr() for k in ("q", "p", "I"))
            a.d_net_torque, a.d_langevin_torque, a.d_gamma_r = (t[k].data_ptr() for k in ("torque", "b", "gamma_r"))
        a.box = _lib.make_box(L_K)
        a.dt, a.kT, a.seed, a.rotational, a.N, a.ntypes, a.block_size = DT_K, KT_K, SEED_K, int(rot), N_K, 3, block_size
        self.stream = torch.cuda.current_stream().cuda_stream

    def call(self, name, timestep):
        from azplugins_amd import _lib

        self.a.timestep = timestep
        _lib.check(getattr(_lib.lib(), "azp_integrate_" + name)(C.byref(self.a), self.stream), name)

    def host(self):
        import torch

        torch.cuda.synchronize()
        g = {k: v.cpu().numpy() for k, v in self.t.items()}
        return dict(pos=g["pos"][:, :3], posw=g["pos"][:, 3], vel=g["vel"][:, :3], mass=g["vel"][:, 3], accel=g["accel"][:, :3],
                    accelw=g["accel"][:, 3], image=g["image"], q=g["q"], p=g["p"], b=g["b"][:, :3], bw=g["b"][:, 3])


FIELDS = ("pos", "vel", "accel", "image", "q", "p", "b")


def _compare_kernel(got, want, sel, start, fields=FIELDS):
    for k in fields:
        if k == "image":
            np.testing.assert_array_equal(got[k], want[k])
        elif k == "q":
            assert np.abs(got[k] - want[k]).max() < 1e-13, "q differs by %g" % np.abs(got[k] - want[k]).max()
        else:
            _close(got[k], want[k], k)
        assert np.array_equal(got[k][~sel], start[k][~sel]), "%s of a masked row changed" % k  # bit for bit
        assert not np.array_equal(got[k][sel], start[k][sel]) or k == "image", k
    assert np.array_equal(got["posw"].view(np.int64), syn.pos4(start["pos"], start["typeid"])[:, 3].view(np.int64))  # the types
    assert np.array_equal(got["mass"], start["mass"]) and not got["accelw"][sel].any() and not got["bw"][sel].any()


@pytest.mark.parametrize("block_size", [0, 64])
def test_langevin_kernels_match_the_reference(block_size):
    """azp_integrate_langevin_step_one / _two with rotation against tests/langevin_ref.py over 5 steps: N = 1000 (no
    multiple of a block), the default block of 256 and blocks of 64."""
    h0 = _kernel_state()
    sel = MASK_K[h0["typeid"]].astype(bool)
    gamma, gamma_r = GAMMA_K[h0["typeid"]], GAMMA_R_K[h0["typeid"]]
    d = _Device(h0, GAMMA_R_K, block_size=block_size)
    h = h0
    for t in range(5):
        d.call("langevin_step_one", 100 + t)
        h = ref.langevin_step_one(h, h0["torque"], [L_K] * 3, DT_K, sel, True)
        d.call("langevin_step_two", 100 + t)
        h = ref.langevin_step_two(h, h0["force"], h0["torque"], gamma, gamma_r, KT_K, DT_K, SEED_K, 100 + t, sel, True)
    got = d.host()
    _compare_kernel(got, h, sel, h0)
    assert np.abs(got["image"] - h0["image"]).sum() > 0  # some particles did cross a face
    assert np.all(got["b"][h0["I"] == 0.0] == 0.0)


@pytest.mark.parametrize("block_size", [0, 64])
def test_brownian_kernel_matches_the_reference(block_size):
    h0 = _kernel_state()
    sel = MASK_K[h0["typeid"]].astype(bool)
    gamma, gamma_r = GAMMA_K[h0["typeid"]], GAMMA_R_BROWNIAN[h0["typeid"]]
    d = _Device(h0, GAMMA_R_BROWNIAN, block_size=block_size)
    h = h0
    for t in range(5):
        d.call("brownian_step", 7 + t)
        h = ref.brownian_step(h, h0["force"], h0["torque"], gamma, gamma_r, KT_K, DT_K, SEED_K, 7 + t, [L_K] * 3, sel, True)
    got = d.host()
    _compare_kernel(got, h, sel, h0, fields=("pos", "image", "q"))
    for k in ("vel", "accel", "p", "b"):  # not touched, whatever the mask
        assert np.array_equal(got[k], h0[k]), k


@pytest.mark.parametrize("rot", [True, False])
def test_two_one_is_two_then_one(rot):
    """The fused launch leaves exactly the bits of step two followed by step one; without `rotational` the rotational
    arrays are not touched (and need not exist)."""
    h0 = _kernel_state()
    out = []
    for fused in (False, True):
        d = _Device(h0, GAMMA_R_K, rot=rot, block_size=128)
        if fused:
            d.call("langevin_step_two_one", 41)
        else:
            d.call("langevin_step_two", 41)
            d.call("langevin_step_one", 41)
        out.append(d.host())
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), k
    sel = MASK_K[h0["typeid"]].astype(bool)
    for k in ("q", "p", "b"):
        assert np.array_equal(out[0][k][sel], h0[k][sel]) == (not rot), k
    assert not np.array_equal(out[0]["pos"][sel], h0["pos"][sel])


# ---------------------------------------------------------------------------
# through Simulation.run
# ---------------------------------------------------------------------------
def _ideal_gas(N=4096, L=16.0, seed=1, types=("A",), typeid=None, sim_seed=5, inertia=None, spin=0.0):
    """An ideal gas with masses 0.5 .. 2; ``inertia``: random orientations and body angular momenta of scale ``spin``."""
    import azplugins_amd as azp

    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-0.5 * L, 0.5 * L, (N, 3))
    kw = {}
    if inertia is not None:
        q = rng.normal(size=(N, 4))
        q /= np.linalg.norm(q, axis=1)[:, None]
        S = spin * rng.normal(size=(N, 3)) * (np.asarray(inertia) != 0.0)
        kw = dict(orientation=q, moment_inertia=np.broadcast_to(inertia, (N, 3)), angmom=2.0 * ref.qmul(q, ref.pure(S)))
    snap = azp.Snapshot.from_arrays(xyz, [L, L, L], typeid=typeid, types=types, velocity=rng.normal(size=(N, 3)), **kw)
    snap.particles.mass[:] = rng.uniform(0.5, 2.0, N)
    sim = azp.Simulation(device="cuda:0", seed=sim_seed)
    sim.create_state_from_snapshot(snap)
    sim.operations.tuners.clear()
    return sim


def _host(sim):
    st = sim.state
    N = st.N
    out = dict(pos=st.pos[:N, :3].cpu().numpy(), vel=st.vel[:N, :3].cpu().numpy(), mass=st.vel[:N, 3].cpu().numpy(),
               image=st.image[:N].cpu().numpy(), tag=st.tag[:N].cpu().numpy().view(np.uint32), typeid=st.typeid_host.copy(),
               force=st.net_force[:N, :3].cpu().numpy(), q=st.orientation[:N].cpu().numpy(), p=st.angmom[:N].cpu().numpy(),
               I=st.inertia[:N].cpu().numpy())
    out["accel"] = st.accel[:N, :3].cpu().numpy() if st.accel is not None else np.zeros((N, 3))
    out["b"] = st.langevin_torque[:N, :3].cpu().numpy() if st.langevin_torque is not None else np.zeros((N, 3))
    return out


def _by_tag(sim):
    g = _host(sim)
    order = np.argsort(g["tag"])
    return {k: v[order] for k, v in g.items()}


STATE = ("pos", "vel", "image", "accel", "q", "p", "b")


@pytest.mark.parametrize("kind", ["langevin", "brownian"])
def test_translation_is_the_flow_method_at_zero_flow(kind):
    """Without integrate_rotational_dof, 20 steps of methods.Langevin / methods.Brownian leave exactly the bits that
    flow.Langevin / flow.Brownian leave with ConstantFlow((0, 0, 0)): N = 4096, a callable kT, two types with their own gamma."""
    import azplugins_amd as azp
    from azplugins_amd import All, flow, methods

    out = []
    for family in ("flow", "methods"):
        sim = _ideal_gas(types=("A", "B"), typeid=np.arange(4096) % 2, inertia=(0.3, 0.4, 0.5), spin=1.0)
        kT = lambda t: 1.0 + 0.01 * t  # noqa: E731
        if family == "flow":
            cls = flow.Langevin if kind == "langevin" else flow.Brownian
            m = cls(All(), kT=kT, flow_field=flow.ConstantFlow((0, 0, 0)), default_gamma=1.5)
        else:
            m = (methods.Langevin if kind == "langevin" else methods.Brownian)(All(), kT=kT, default_gamma=1.5)
        m.gamma["B"] = 0.25
        sim.operations.integrator = azp.Integrator(dt=0.01, methods=[m])
        start = _host(sim)
        sim.run(20)
        out.append(_host(sim))
        assert sim.state.langevin_torque is None
    for k in STATE:
        assert np.array_equal(out[0][k], out[1][k]), k
    assert not np.array_equal(out[1]["pos"], start["pos"])
    for k in ("q", "p"):  # rotation off: not read, not written
        assert np.array_equal(out[1][k], start[k])


def test_rotation_without_friction_is_the_nve_rotation():
    """Free tops, gamma = gamma_r = 0: after 20 steps q and p hold the bits that ConstantVolume with
    integrate_rotational_dof leaves (kT > 0 changes nothing: every noise amplitude is sqrt(0))."""
    import azplugins_amd as azp
    from azplugins_amd import All, methods

    out = []
    for method in (azp.ConstantVolume(), methods.Langevin(All(), kT=1.5, default_gamma=0.0, default_gamma_r=(0.0, 0.0, 0.0))):
        sim = _ideal_gas(N=1000, inertia=(0.3, 0.4, 0.5), spin=1.0)
        sim.operations.integrator = azp.Integrator(dt=0.01, methods=[method], integrate_rotational_dof=True)
        start = _host(sim)
        sim.run(20)
        out.append(_host(sim))
    for k in ("q", "p"):
        assert np.array_equal(out[0][k], out[1][k]), k
        assert not np.array_equal(out[1][k], start[k]), k
    assert not out[1]["b"].any()


def _tpm_sim(method, n=6, dt=0.002):
    """TwoPatchMorse colloids on config_tpm(n, n, n) with the soft well of the NVE energy test (its cutoff of 4.0 does not fit
    this box of 7.2: 3.0 here), thermal velocities, random body angular momenta, unequal moments of inertia."""
    import azplugins_amd as azp

    cfg = syn.config_tpm(n, n, n)
    N = cfg["xyz"].shape[0]
    rng = np.random.default_rng(8)
    S = 0.2 * rng.normal(size=(N, 3))
    snap = azp.Snapshot.from_arrays(cfg["xyz"], cfg["L"], velocity=0.5 * rng.normal(size=(N, 3)), orientation=cfg["orientation"],
                                    moment_inertia=np.tile([0.1, 0.12, 0.14], (N, 1)),
                                    angmom=2.0 * ref.qmul(cfg["orientation"], ref.pure(S)))
    snap.particles.mass[:] = rng.uniform(0.5, 2.0, N)
    sim = azp.Simulation(device="cuda:0", seed=77)
    sim.create_state_from_snapshot(snap)
    sim.operations.tuners.clear()
    tpm = azp.pair.TwoPatchMorse(nlist=azp.nlist.Cell(buffer=0.4), default_r_cut=3.0, mode="none")
    tpm.params[("A", "A")] = TPM_SOFT
    sim.operations.integrator = azp.Integrator(dt=dt, forces=[tpm], methods=[method], integrate_rotational_dof=True)
    return sim, tpm


@pytest.mark.parametrize("kind", ["langevin", "brownian"])
def test_one_step_with_forces_and_torques(kind):
    """One step through Simulation.run against the restatement fed the device's own forces and torques (at t for step one and
    the Brownian step, at t + 1 for step two)."""
    from azplugins_amd import All, methods

    if kind == "langevin":
        m = methods.Langevin(All(), kT=0.8, default_gamma=2.0, default_gamma_r=(0.5, 1.0, 1.5))
    else:
        m = methods.Brownian(All(), kT=0.8, default_gamma=40.0, default_gamma_r=(5.0, 10.0, 15.0))
    sim, tpm = _tpm_sim(m)
    sim.run(0)
    h = _host(sim)
    N = h["tag"].size
    h["accel"] = h["force"] / h["mass"][:, None]  # a = F(t) / m at the first run
    torque0 = tpm.torques.copy()
    assert np.abs(h["force"]).max() > 0.1 and np.abs(torque0).max() > 0.01  # forces and torques that matter
    sim.run(1)
    g = _host(sim)
    sel, L, dt, seed = np.ones(N, bool), sim.state.box.L, 0.002, 77
    gamma, gamma_r = np.full(N, m.gamma["A"]), np.tile(m.gamma_r["A"], (N, 1))
    if kind == "langevin":
        want = ref.langevin_step_one(h, torque0, L, dt, sel, True)
        want = ref.langevin_step_two(want, g["force"], tpm.torques, gamma, gamma_r, 0.8, dt, seed, 0, sel, True)
        fields = STATE
    else:
        want = ref.brownian_step(h, h["force"], torque0, gamma, gamma_r, 0.8, dt, seed, 0, L, sel, True)
        fields = ("pos", "image", "q")
        assert np.array_equal(g["vel"], h["vel"]) and np.array_equal(g["p"], h["p"]) and sim.state.accel is None
    for k in fields:
        if k == "image":
            np.testing.assert_array_equal(g[k], want[k])
        elif k == "q":
            assert np.abs(g[k] - want[k]).max() < 1e-13
        else:
            _close(g[k], want[k], k)
    assert not np.array_equal(g["q"], h["q"])


def _two_type_rotors(sim_seed=5, N=4096, sorter=0):
    """Types A (methods.Langevin), B (methods.Brownian), C (no method): an ideal gas of spinning tops, rotation on."""
    import azplugins_amd as azp
    from azplugins_amd import Type, methods

    sim = _ideal_gas(N=N, L=20.0, types=("A", "B", "C"), typeid=np.arange(N) % 3, sim_seed=sim_seed, inertia=(0.3, 0.0, 0.5), spin=0.5)
    if sorter:
        sim.operations.tuners.append(azp.ParticleSorter(trigger_period=sorter))
    lan = methods.Langevin(Type("A"), kT=0.8, default_gamma=0.5, default_gamma_r=(0.4, 0.8, 1.2))
    bro = methods.Brownian(Type(["B"]), kT=1.3, default_gamma=3.0, default_gamma_r=(2.0, 3.0, 4.0))
    sim.operations.integrator = azp.Integrator(dt=0.02, methods=[lan, bro], integrate_rotational_dof=True)
    return sim


def _run_rotors(splits, **kw):
    sim = _two_type_rotors(**kw)
    for n in splits:
        sim.run(n)
    return sim, _by_tag(sim)


def test_split_and_repeated_runs_are_bit_identical():
    _, a = _run_rotors([20])
    _, b = _run_rotors([10, 10])
    _, c = _run_rotors([20])
    _, d = _run_rotors([20], sim_seed=6)
    for k in STATE:
        assert np.array_equal(a[k], b[k]), k
        assert np.array_equal(a[k], c[k]), k
    for k in ("pos", "vel", "q", "p", "b"):
        assert not np.array_equal(a[k], d[k]), k  # another seed, another trajectory


def test_type_filter_leaves_the_other_types_untouched():
    sim = _two_type_rotors()
    start = _by_tag(sim)
    sim.run(15)
    g = _by_tag(sim)
    a, b, c = (start["typeid"] == k for k in range(3))
    for k in STATE:
        assert np.array_equal(g[k][c], start[k][c]), k  # no method selects C: every bit where it was
    for k in ("vel", "p", "accel", "b"):  # Brownian leaves velocities and angular momenta alone, stores nothing
        assert np.array_equal(g[k][b], start[k][b]), k
    for k in ("pos", "q"):
        assert not np.array_equal(g[k][a], start[k][a]) and not np.array_equal(g[k][b], start[k][b]), k
    assert not np.array_equal(g["p"][a], start["p"][a]) and g["b"][a].any()


def test_particle_sort_keeps_the_trajectory():
    """accel and langevin_torque travel with the particles: a sorted run equals the unsorted one, particle by tag."""
    s_sorted, a = _run_rotors([120], N=8192, sorter=50)
    _, b = _run_rotors([120], N=8192)
    assert s_sorted.operations.tuners[0].num_sorts == 2
    assert not np.array_equal(_host(s_sorted)["tag"], np.arange(8192, dtype=np.uint32))  # the order did change
    for k in STATE:
        assert np.array_equal(a[k], b[k]), k


def test_recorder_due_mid_run_leaves_the_trajectory():
    """A ThermodynamicRecorder due every 7 steps splits the fused launch there (step two on its own, then step one): the same
    bits as the run without it."""
    from azplugins_amd import All, compute, trigger

    def run(record):
        sim = _two_type_rotors()
        if record:
            thermo = compute.ThermodynamicQuantities(All())
            sim.operations.add(thermo)
            rec = compute.ThermodynamicRecorder(thermo, trigger.Periodic(7))
            sim.operations.add(rec)
        sim.run(30)
        return _by_tag(sim)

    a, b = run(True), run(False)
    for k in STATE:
        assert np.array_equal(a[k], b[k]), k


def test_flow_method_next_to_a_methods_one():
    """flow.Langevin on type A (a constant flow) next to methods.Langevin on type B, 20 steps against the restatements."""
    import azplugins_amd as azp
    import flow_ref
    from azplugins_amd import Type, flow, methods

    N, dt, L = 4096, 0.01, 16.0
    sim = _ideal_gas(N=N, L=L, types=("A", "B"), typeid=np.arange(N) % 2)
    U = (0.7, -0.3, 0.2)
    fl = flow.Langevin(Type("A"), kT=1.2, flow_field=flow.ConstantFlow(U), default_gamma=1.5)
    me = methods.Langevin(Type("B"), kT=0.6, default_gamma=0.8)
    sim.operations.integrator = azp.Integrator(dt=dt, methods=[fl, me])
    h = _host(sim)
    sim.run(20)
    g = _host(sim)
    a, b = h["typeid"] == 0, h["typeid"] == 1
    zero = np.zeros((N, 3))
    for t in range(20):
        h["pos"], h["vel"], h["image"] = flow_ref.langevin_step_one(h["pos"], h["vel"], h["accel"], h["image"], [L] * 3, dt, a)
        h = ref.langevin_step_one(h, zero, [L] * 3, dt, b, False)
        h["vel"], h["accel"] = flow_ref.langevin_step_two(h["pos"], h["vel"], h["mass"], h["accel"], zero, h["tag"], np.full(N, 1.5),
                                                          1.2, dt, 5, t, ("constant", U), False, a)
        h = ref.langevin_step_two(h, zero, zero, np.full(N, 0.8), None, 0.6, dt, 5, t, b, False)
    for k in ("pos", "vel", "accel"):
        _close(g[k], h[k], k)
    np.testing.assert_array_equal(g["image"], h["image"])
    assert abs(g["vel"][a].mean(axis=0)[0] - g["vel"][b].mean(axis=0)[0]) > 0.05  # A is dragged along by its flow


# ---------------------------------------------------------------------------
# statistics: planar rotors, I = (0, 0, 1), no forces
# ---------------------------------------------------------------------------
def _planar_rotors(method, dt, N=4096):
    import azplugins_amd as azp

    rng = np.random.default_rng(3)
    snap = azp.Snapshot.from_arrays(rng.uniform(-8.0, 8.0, (N, 3)), [16.0] * 3, moment_inertia=np.tile([0.0, 0.0, 1.0], (N, 1)))
    sim = azp.Simulation(device="cuda:0", seed=9)
    sim.create_state_from_snapshot(snap)
    sim.operations.tuners.clear()
    sim.operations.integrator = azp.Integrator(dt=dt, methods=[method], integrate_rotational_dof=True)
    return sim


def test_langevin_rotor_statistics():
    """The full-step variance of S_z is exactly kT I_z (the half-step S_z is AR(1) with factor 1 - g dt / I; no
    dt bias): after 1000 steps, the mean of S_z^2 / I_z over 4 samples 500 steps (10 relaxation times) apart lies within
    5 sigma of a chi-square with 4 N degrees of freedom. ThermodynamicQuantities sums the same rotational energy."""
    from azplugins_amd import All, compute, methods

    N, kT, g, dt = 4096, 1.5, 2.0, 0.01
    sim = _planar_rotors(methods.Langevin(All(), kT=kT, default_gamma_r=(1.0, 1.0, g)), dt)
    thermo = compute.ThermodynamicQuantities(All())
    sim.operations.add(thermo)
    sim.run(1000)
    samples = []
    for _ in range(4):
        sim.run(500)
        h = _host(sim)
        s2 = ref.body_angmom(h["q"], h["p"])[:, 2] ** 2 / h["I"][:, 2]
        samples.append(s2.mean())
        assert abs(thermo.rotational_kinetic_energy - 0.5 * s2.sum()) < 1e-10 * s2.sum()
    assert thermo.rotational_degrees_of_freedom == N
    assert abs(np.mean(samples) - kT) < 5 * kT * np.sqrt(2.0 / (4 * N)), samples
    assert not ref.body_angmom(h["q"], h["p"])[:, :2].any() and not h["q"][:, 1:3].any()  # planar it stays
    np.testing.assert_allclose(np.linalg.norm(h["q"], axis=1), 1.0, atol=1e-12)


def test_brownian_rotor_statistics():
    """theta = 2 atan2(q_z, q_s) after t = 50 dt has the variance 2 kT t / gamma_r = 0.25 within 5 sqrt(2 / N) relative and
    the mean 0 within 5 sqrt(var / N) (5 sigma = 2.5 < pi: nothing to unwrap); angmom is not touched."""
    from azplugins_amd import All, methods

    N, kT, g, dt, steps = 4096, 1.0, 2.0, 0.005, 50
    sim = _planar_rotors(methods.Brownian(All(), kT=kT, default_gamma_r=(1.0, 1.0, g)), dt)
    h0 = _host(sim)
    sim.run(steps)
    h = _host(sim)
    theta = 2.0 * np.arctan2(h["q"][:, 3], h["q"][:, 0]) - 2.0 * np.arctan2(h0["q"][:, 3], h0["q"][:, 0])
    var = 2.0 * kT * steps * dt / g
    assert abs(np.var(theta) / var - 1.0) < 5 * np.sqrt(2.0 / N), np.var(theta)
    assert abs(np.mean(theta)) < 5 * np.sqrt(var / N), np.mean(theta)
    assert np.array_equal(h["p"], h0["p"]) and np.array_equal(h["vel"], h0["vel"])


# ---------------------------------------------------------------------------
# one full-size run
# ---------------------------------------------------------------------------
C5_KT, C5_DT, C5_GAMMA, C5_GAMMA_R, C5_INERTIA, C5_STEPS = 1.0, 0.004, 5.0, (1.0, 1.0, 1.0), (0.1, 0.12, 0.14), 200
# T_trans, T_rot of tests/langevin_ref.py on config_tpm(6, 6, 6) with the oracle's forces after C5_STEPS steps, mean over 16
# seeds, and the standard error of each mean (tools/langevin_probe.py --reference prints them)
C5_REF = dict(T_trans=(1.0169, 0.0183), T_rot=(0.9765, 0.0134))


def c5_temperatures(vel, mass, q, p, I):
    """kT of the translation, 2 K / (3 N - 3), and of the rotation, 2 K_rot / (3 N)."""
    N = mass.size
    S = ref.body_angmom(q, p)
    return float((mass[:, None] * vel ** 2).sum() / (3 * N - 3)), float((S ** 2 / I).sum() / (3 * N))


def test_c5_full_size_langevin():
    """C5 at the benchmark's size (64 x 64 x 128 TwoPatchMorse colloids) under methods.Langevin with rotation and the sorter,
    200 steps: everything finite, |q| = 1, and both temperatures where the restatement puts them on a 6 x 6 x 6 copy of the
    system at the same dt: within 5 sigma, sigma^2 = (standard error of the 16-seed reference mean)^2 + kT^2 2 / (3 N).
    Reference: T_trans = 1.0169 +- 0.0183, T_rot = 0.9765 +- 0.0134 (bands +-0.092 and +-0.068); measured on the MI355X:
    T_trans = 1.0211, T_rot = 1.0048."""
    import torch

    import azplugins_amd as azp
    from azplugins_amd import All, methods

    cfg = syn.config_tpm()
    N = cfg["xyz"].shape[0]
    assert N == 64 * 64 * 128
    snap = azp.Snapshot.from_arrays(cfg["xyz"], cfg["L"], orientation=cfg["orientation"])
    snap.particles.moment_inertia[:] = C5_INERTIA
    sim = azp.Simulation(device="cuda:0", seed=11)
    sim.create_state_from_snapshot(snap)
    sim.operations.tuners[:] = [azp.ParticleSorter(trigger_period=50)]
    tpm = azp.pair.TwoPatchMorse(nlist=azp.nlist.Cell(buffer=cfg["r_buff"]), default_r_cut=cfg["r_cut"], mode="shift")
    tpm.params[("A", "A")] = cfg["params"]
    m = methods.Langevin(All(), kT=C5_KT, default_gamma=C5_GAMMA, default_gamma_r=C5_GAMMA_R)
    sim.operations.integrator = azp.Integrator(dt=C5_DT, forces=[tpm], methods=[m], integrate_rotational_dof=True)
    sim.thermalize_particle_momenta(C5_KT, seed=5)
    sim.run(C5_STEPS)
    st = sim.state
    for name in ("pos", "vel", "accel", "net_force", "orientation", "angmom", "langevin_torque"):
        assert bool(torch.isfinite(getattr(st, name)[:N]).all()), name
    assert sim.operations.tuners[0].num_sorts >= 3
    h = _host(sim)
    assert np.abs(np.linalg.norm(h["q"], axis=1) - 1.0).max() < 1e-12
    T = dict(zip(("T_trans", "T_rot"), c5_temperatures(h["vel"], h["mass"], h["q"], h["p"], h["I"])))
    print("C5 under Langevin after %d steps: %r; reference %r" % (C5_STEPS, T, C5_REF))
    for name, (mean, stderr) in C5_REF.items():
        sigma = np.sqrt(stderr ** 2 + C5_KT ** 2 * 2.0 / (3 * N))
        assert abs(T[name] - mean) < 5 * sigma, (name, T[name], mean, sigma)
