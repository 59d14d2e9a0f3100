"""Type updates on the GPU (csrc/type_update.hip, azplugins_amd.update / .evaporate): the kernels against the numpy
restatement (tests/evaporate_ref.py) with no tolerance -- the results are integers -- invariance of the picked tags
under re-indexing, bit-identical repeats, the force path after a type change (list mode, fused-plan mode, a step at
which a speculative launch would otherwise have run), a type-filtered flow method, a small drying run end to end, a
decomposed run against the single-domain run, and that an updater disturbs nothing else."""

import ctypes as C
import os
import socket

import numpy as np
import pytest

import evaporate_ref as ref
import flow_ref
from azplugins_amd import _lib
from azplugins_amd import synthetic as syn

pytestmark = pytest.mark.gpu

PLJ = "PerturbedLennardJones"
TOL = 1e-10  # tests/test_gpu_parity.py: PerturbedLennardJones forces against the oracle


# -- the kernels through the C ABI ---------------------------------------------------------------------------------
def _dev(a):
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to("cuda:0")


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _system(N, seed, Lz=20.0, lo=-1.0, hi=0.5):
    """Three types, random tags; for N >= 8 two solvent (type 1) particles sit exactly on z = lo and z = hi."""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-0.5, 0.5, (N, 3)) * np.array([12.0, 12.0, Lz])
    typeid = rng.integers(0, 3, N)
    if N >= 8:
        xyz[1, 2], xyz[5, 2] = lo, hi
        typeid[1] = typeid[5] = 1
    if N == 1:
        xyz[0, 2], typeid[0] = 0.0, 1
    tag = (rng.permutation(N) + 7).astype(np.uint32)
    return syn.pos4(xyz, typeid), typeid, tag


def _check_only_types_changed(before, after):
    b, a = before.view(np.uint64), after.view(np.uint64)
    np.testing.assert_array_equal(a[:, :3], b[:, :3])  # x, y, z: the same bits
    np.testing.assert_array_equal(a[:, 3] >> np.uint64(32), b[:, 3] >> np.uint64(32))
    return (a[:, 3] & np.uint64(0xFFFFFFFF)).astype(np.int64)


def gpu_type_update(pos_dev, N, inside, outside, lo, hi):
    a = _lib.TypeUpdateArgs()
    a.d_pos, a.N = pos_dev.data_ptr(), N
    a.inside_type, a.outside_type, a.z_lo, a.z_hi = inside, outside, lo, hi
    _lib.check(_lib.lib().azp_type_update_region(C.byref(a), _stream()), "azp_type_update_region")


class _Evap:
    """One evaporator's device buffers for a system of N rows."""

    def __init__(self, N, tag):
        import torch

        self.N = N
        self.tag = _dev(tag)
        self.scratch = torch.empty(int(_lib.lib().azp_evaporate_scratch_size(N)), dtype=torch.uint8, device="cuda:0")
        self.counts = torch.full((2,), -1, dtype=torch.int32, device="cuda:0")

    def args(self, pos_dev, solvent, evaporated, lo, hi, Nmax, seed, timestep):
        a = _lib.EvaporateArgs()
        a.d_pos, a.d_tag, a.N = pos_dev.data_ptr(), self.tag.data_ptr(), self.N
        a.solvent_type, a.evaporated_type = solvent, evaporated
        a.Nmax = _lib.EVAPORATE_NO_LIMIT if Nmax is None else Nmax
        a.z_lo, a.z_hi, a.timestep, a.seed = lo, hi, timestep, seed
        a.d_scratch, a.scratch_bytes = self.scratch.data_ptr(), self.scratch.numel()
        a.d_counts = self.counts.data_ptr()
        return a

    def evaporate(self, pos_dev, *spec):
        self.counts.fill_(-1)
        _lib.check(_lib.lib().azp_evaporate(C.byref(self.args(pos_dev, *spec)), _stream()), "azp_evaporate")
        return self.counts.cpu().numpy().view(np.uint32).tolist()


SLABS = {"thin": (-1.0, 0.5), "empty": (0.123456789, 0.123456789), "whole": (-10.0, 10.0)}
T_LOW, T_HIGH = 4294967290, (5 << 32) + 4294967290  # both sides of 2^32: the key's high byte


@pytest.mark.parametrize("N", [1, 63, 64, 65, 4096, 2**20])
def test_type_update_region_exact(N):
    pos, typeid, _ = _system(N, seed=N)
    for name, (lo, hi) in SLABS.items():
        for inside, outside in ((0, 1), (2, 0)):
            d = _dev(pos)
            gpu_type_update(d, N, inside, outside, lo, hi)
            got = _check_only_types_changed(pos, d.cpu().numpy())
            np.testing.assert_array_equal(got, ref.type_update_region(pos[:, 2], typeid, inside, outside, lo, hi), err_msg=name)
    if N >= 8:  # the particles on the faces are inside
        d = _dev(pos)
        gpu_type_update(d, N, 2, 1, *SLABS["thin"])
        got = _check_only_types_changed(pos, d.cpu().numpy())
        assert got[1] == 2 and got[5] == 2


@pytest.mark.parametrize("N", [1, 63, 64, 65, 4096, 2**20])
def test_evaporate_exact(N):
    pos, typeid, tag = _system(N, seed=100 + N)
    ev = _Evap(N, tag)
    pos_dev = _dev(pos)
    for name, (lo, hi) in SLABS.items():
        M = int(ref.candidates(pos[:, 2], typeid, 1, lo, hi).sum())
        assert (M == 0) == (name == "empty")
        if N >= 4096:
            assert (name != "thin") or 0 < M < N // 10
        for Nmax in sorted({1, 7, max(M - 1, 0), M, M + 1}) + [None]:
            for timestep in (T_LOW, T_HIGH):
                d = pos_dev.clone()
                counts = ev.evaporate(d, 1, 2, lo, hi, Nmax, 5, timestep)
                got = _check_only_types_changed(pos, d.cpu().numpy())
                want, M_ref, n_ref = ref.evaporate(pos[:, 2], typeid, tag, 1, 2, lo, hi, Nmax, 5, timestep)
                what = "%s slab, Nmax %r, timestep %d" % (name, Nmax, timestep)
                assert counts == [M_ref, n_ref], what
                # the new type of every row; with it the set of changed tags
                np.testing.assert_array_equal(got, want, err_msg=what)
                assert set(tag[got != typeid].tolist()) == set(tag[want != typeid].tolist())
    if N >= 8:
        # the particles on the two faces are candidates: with no limit they go
        d = pos_dev.clone()
        ev.evaporate(d, 1, 2, *SLABS["thin"], None, 5, 0)
        got = _check_only_types_changed(pos, d.cpu().numpy())
        assert got[1] == 2 and got[5] == 2
    # the two sides of 2^32 draw different keys (N = 1 has nothing to choose from)
    if N >= 4096:
        a = ref.evaporate(pos[:, 2], typeid, tag, 1, 2, -10.0, 10.0, 7, 5, T_LOW)[0]
        b = ref.evaporate(pos[:, 2], typeid, tag, 1, 2, -10.0, 10.0, 7, 5, T_HIGH)[0]
        assert not np.array_equal(a, b)


@pytest.mark.parametrize("N,Nmax", [(65, 3), (4096, 100), (20000, 4096), (20000, 5000), (20000, 30000)])
def test_two_phase_calls_exact(N, Nmax):
    """azp_evaporate_local_keys and azp_evaporate_apply_below against the numpy two-phase form: the keys a rank offers
    (ascending; the single-workgroup sort up to 4096 keys, the stepwise one beyond) and the rows flipped below a
    threshold."""
    import torch

    pos, typeid, tag = _system(N, seed=300 + N)
    ev = _Evap(N, tag)
    lo, hi, seed, timestep = -10.0, 10.0, 9, 1234
    cand = np.flatnonzero(ref.candidates(pos[:, 2], typeid, 1, lo, hi))
    want_keys = ref.local_keys(tag[cand], seed, timestep, Nmax)
    d = _dev(pos)
    keys_out = torch.full((min(Nmax, N),), -1, dtype=torch.int64, device="cuda:0")
    n_out = torch.full((1,), -1, dtype=torch.int32, device="cuda:0")
    a = ev.args(d, 1, 2, lo, hi, Nmax, seed, timestep)
    a.d_keys_out, a.d_n_keys_out = keys_out.data_ptr(), n_out.data_ptr()
    _lib.check(_lib.lib().azp_evaporate_local_keys(C.byref(a), _stream()), "azp_evaporate_local_keys")
    n = int(n_out.item())
    assert n == want_keys.size and ev.counts.cpu().numpy().view(np.uint32).tolist() == [cand.size, 0]
    np.testing.assert_array_equal(keys_out.cpu().numpy().view(np.uint64)[:n], want_keys)
    np.testing.assert_array_equal(d.cpu().numpy().view(np.uint64), pos.view(np.uint64))  # phase one changes nothing
    # phase two with a threshold in the middle of the offered keys, and with the largest key (everything)
    for thr in (int(want_keys[n // 2]), 0xFFFFFFFFFFFFFFFF, 0):
        d = _dev(pos)
        a = ev.args(d, 1, 2, lo, hi, Nmax, seed, timestep)
        _lib.check(_lib.lib().azp_evaporate_apply_below(C.byref(a), thr, _stream()), "azp_evaporate_apply_below")
        got = _check_only_types_changed(pos, d.cpu().numpy())
        want = typeid.copy()
        want[cand[ref.apply_below(tag[cand], seed, timestep, np.uint64(thr))]] = 2
        np.testing.assert_array_equal(got, want)
        assert ev.counts.cpu().numpy().view(np.uint32).tolist() == [cand.size, int((want != typeid).sum())]


# -- through the Python interface ------------------------------------------------------------------------------------
def _gas(N=4096, L=(12.0, 12.0, 20.0), seed=1, sim_seed=5, order=None):
    """An ideal gas of three types A, B, C with random tags; ``order``: a permutation of the rows."""
    import azplugins_amd as azp

    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-0.5, 0.5, (N, 3)) * np.asarray(L)
    typeid = rng.integers(0, 3, N)
    tag = rng.permutation(N).astype(np.uint32)
    vel = rng.normal(size=(N, 3))
    if order is not None:
        xyz, typeid, tag, vel = xyz[order], typeid[order], tag[order], vel[order]
    snap = azp.Snapshot.from_arrays(xyz, list(L), typeid=typeid, types=("A", "B", "C"), tag=tag, velocity=vel)
    sim = azp.Simulation(device="cuda:0", seed=sim_seed)
    sim.create_state_from_snapshot(snap)
    sim.operations.tuners.clear()
    return sim


def _types_by_tag(sim):
    st = sim.state
    tag = st.tag[: st.N].cpu().numpy().view(np.uint32).astype(np.int64)
    out = np.full(tag.max() + 1, -1, dtype=np.int64)
    out[tag] = st.typeid_host
    return out


def test_reindexing_invariance():
    import azplugins_amd as azp
    from azplugins_amd.evaporate import ParticleEvaporator

    N = 4096
    results = []
    for variant in ("plain", "permuted", "sorted"):
        order = np.random.default_rng(77).permutation(N) if variant == "permuted" else None
        sim = _gas(N, order=order)
        if variant == "sorted":
            before = sim.state.tag.cpu().numpy().copy()
            azp.ParticleSorter().sort(sim)
            assert not np.array_equal(sim.state.tag.cpu().numpy(), before)
        ev = ParticleEvaporator(trigger=1, solvent_type="B", evaporated_type="C", lo=-3.0, hi=2.0, Nmax=37)
        was = _types_by_tag(sim)
        for t in (0, 1, 2):
            ev._update(sim, t)
            assert ev.n_evaporated == 37 and ev.n_candidates > 37
        now = _types_by_tag(sim)
        assert (now != was).sum() == 3 * 37
        results.append(now)
    np.testing.assert_array_equal(results[0], results[1])
    np.testing.assert_array_equal(results[0], results[2])
    # and it is the numpy rule's pick
    sim = _gas(N)
    st = sim.state
    typeid, z = st.typeid_host.copy(), st.pos[:, 2].cpu().numpy()
    tag = st.tag.cpu().numpy().view(np.uint32)
    for t in (0, 1, 2):
        typeid = ref.evaporate(z, typeid, tag, 1, 2, -3.0, 2.0, 37, 5, t)[0]
    want = np.full(N, -1, dtype=np.int64)
    want[tag.astype(np.int64)] = typeid
    np.testing.assert_array_equal(results[0], want)


def _flow_run(n_steps, updaters, record_every=1):
    import azplugins_amd as azp
    from azplugins_amd import Type, flow

    sim = _gas(4096)
    m = flow.Langevin(filter=Type("B"), kT=1.0, flow_field=flow.ConstantFlow(velocity=(0.3, 0.0, 0.1)), default_gamma=1.0)
    sim.operations.integrator = azp.Integrator(dt=0.01, methods=[m])
    for u in updaters:
        sim.operations.add(u)
    return sim, m


def test_repeat_is_bit_identical():
    from azplugins_amd.evaporate import ParticleEvaporator
    from azplugins_amd.update import TypeUpdater

    def run():
        ev = ParticleEvaporator(trigger=3, solvent_type="B", evaporated_type="C", lo=-2.0, hi=2.0, Nmax=11)
        up = TypeUpdater(trigger=4, inside_type="A", outside_type="B", lo=5.0, hi=10.0)
        sim, _ = _flow_run(0, [ev, up])
        history = []
        for _ in range(13):
            sim.run(1)
            history.append(sim.state.pos[:, 3].cpu().numpy().view(np.int64).copy())
        return history

    a, b = run(), run()
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    assert not np.array_equal(a[0], a[-1])


def test_langevin_type_filter_follows_the_update():
    """flow.Langevin on the solvent type: from the step of the update on, an evaporated particle is no longer moved
    (HOOMD's order: the updater runs after step two of the previous step and ahead of step one), checked against the
    numpy schemes with the selection recomputed from the types at every step."""
    from azplugins_amd.evaporate import ParticleEvaporator

    ev = ParticleEvaporator(trigger=4, solvent_type="B", evaporated_type="C", lo=-4.0, hi=4.0, Nmax=100)
    sim, m = _flow_run(0, [ev])
    st = sim.state
    N = st.N
    L, dt, seed = st.box.L, 0.01, sim.seed & 0xFFFF
    h = dict(pos=st.pos[:N, :3].cpu().numpy().copy(), vel=st.vel[:N, :3].cpu().numpy().copy(), mass=st.vel[:N, 3].cpu().numpy().copy(),
             image=st.image[:N].cpu().numpy().copy(), tag=st.tag[:N].cpu().numpy().view(np.uint32).copy(), typeid=st.typeid_host.copy())
    h["accel"] = np.zeros((N, 3))
    gamma = np.ones(N)
    force = np.zeros((N, 3))
    start = h["pos"].copy()
    frozen_at = {}
    sim.run(8)  # updates at t = 0 and, inside the run, at t = 4
    pos_8 = st.pos[:N, :3].cpu().numpy().copy()
    sim.run(2)  # update at t = 8
    for t in range(10):
        if t % 4 == 0:
            new = ref.evaporate(h["pos"][:, 2], h["typeid"], h["tag"], 1, 2, -4.0, 4.0, 100, seed, t)[0]
            for i in np.flatnonzero(new != h["typeid"]):
                frozen_at[i] = t
            h["typeid"] = new
        sel = h["typeid"] == 1
        h["pos"], h["vel"], h["image"] = flow_ref.langevin_step_one(h["pos"], h["vel"], h["accel"], h["image"], L, dt, sel)
        h["vel"], h["accel"] = flow_ref.langevin_step_two(h["pos"], h["vel"], h["mass"], h["accel"], force, h["tag"], gamma, 1.0, dt,
                                                          seed, t, ("constant", (0.3, 0.0, 0.1)), False, sel)
    got_pos, got_vel = st.pos[:N, :3].cpu().numpy(), st.vel[:N, :3].cpu().numpy()
    np.testing.assert_array_equal(st.typeid_host, h["typeid"])
    assert len(frozen_at) == 300  # updates at t = 0, 4, 8
    assert np.abs(got_pos - h["pos"]).max() <= 1e-12 * np.abs(h["pos"]).max()
    assert np.abs(got_vel - h["vel"]).max() <= 1e-12 * np.abs(h["vel"]).max()
    # an evaporated particle stays where it was when it evaporated, bit for bit: all of them since t = 8 (those of
    # t = 8 were not moved by the step that began with their update), those of t = 0 since the start
    gone = np.array(sorted(frozen_at))
    np.testing.assert_array_equal(got_pos[gone], pos_8[gone])
    first = np.array([i for i, t in frozen_at.items() if t == 0])
    np.testing.assert_array_equal(got_pos[first], start[first])
    assert sorted(set(frozen_at.values())) == [0, 4, 8]
    moved = (h["typeid"] == 1)
    assert np.all(np.any(got_pos[moved] != start[moved], axis=1))


# -- forces see the new types ----------------------------------------------------------------------------------------
def _two_type_params(case):
    """case "eps0": the evaporated type B has epsilon = 0 with everything. case "rcut": B has the LARGER r_cut (a
    list built for the old types would miss pairs)."""
    eps = dict(AA=1.0, AB=0.0 if case == "eps0" else 0.8, BB=0.0 if case == "eps0" else 1.3)
    table = {k: dict(epsilon=e, sigma=1.0, attraction_scale_factor=0.5) for k, e in eps.items()}
    r_cut = dict(AA=2.0, AB=2.0 if case == "eps0" else 2.6, BB=2.0 if case == "eps0" else 3.0)
    return table, r_cut


@pytest.mark.parametrize("launch", ["list", "fused"])
@pytest.mark.parametrize("case", ["eps0", "rcut"])
def test_forces_follow_a_type_change(oracle, case, launch):
    import azplugins_amd as azp
    from azplugins_amd.evaporate import ParticleEvaporator
    from azplugins_amd.update import TypeUpdater

    cfg = syn.config_plj_sc(16)
    n = cfg["xyz"].shape[0]
    tagv = np.arange(n, dtype=np.uint64)
    vel = np.stack([syn.normal(41, tagv, c) for c in range(3)], axis=1) * 0.5
    typeid = (syn.hash64(9, tagv, 3) % np.uint64(8) == 0).astype(np.int64)  # 1/8 of type B to begin with
    snap = azp.Snapshot.from_arrays(cfg["xyz"], cfg["L"], typeid=typeid, types=("A", "B"), velocity=vel - vel.mean(axis=0))
    sim = azp.Simulation(device="cuda:0", seed=3)
    sim.create_state_from_snapshot(snap)
    sim.operations.tuners.clear()
    r_buff = 0.4
    nl = azp.nlist.Cell(buffer=r_buff)
    plj = azp.pair.PerturbedLennardJones(nlist=nl, default_r_cut=2.0, mode="shift")
    table, r_cut = _two_type_params(case)
    for pair in (("A", "A"), ("A", "B"), ("B", "B")):
        plj.params[pair] = table[pair[0] + pair[1]]
        plj.r_cut[pair] = r_cut[pair[0] + pair[1]]
    if launch == "list":
        nl.fused = False
    sim.operations.integrator = azp.Integrator(dt=0.002, forces=[plj], methods=[azp.ConstantVolume()])
    half = 0.5 * cfg["L"][2]
    if case == "eps0":
        up = ParticleEvaporator(trigger=azp.Periodic(100, phase=3), solvent_type="A", evaporated_type="B", lo=-0.5 * half, hi=half, Nmax=500)
    else:
        up = TypeUpdater(trigger=azp.Periodic(100, phase=3), inside_type="B", outside_type="A", lo=-0.25 * half, hi=0.25 * half)
    sim.operations.add(up)
    # how each force evaluation was launched: True = queued behind the distance check (speculative)
    launches = []
    inner = plj._compute_speculative

    def watched(timestep):
        launches.append(bool(inner(timestep)))
        return launches[-1]

    plj._compute_speculative = watched
    was = sim.state.typeid_host.copy()
    sim.run(5)  # forces at t = 0 .. 5; the updater runs at the top of the step that starts at t = 3
    now = sim.state.typeid_host.copy()
    assert ((now == 1) & (was == 0)).sum() >= 400  # many particles took the type with epsilon = 0 / the larger r_cut
    if case == "eps0":
        assert up.n_evaporated == 500 == (now != was).sum()
    # evaluations at t = 1, 2 were speculative launches, and so was t = 5; at t = 4, the first after the update,
    # the list was rebuilt instead although nothing had moved far
    assert launches == [False, True, True, True, False, True], launches
    assert nl.num_builds == 2
    assert nl.fused_active == (launch == "fused")
    assert plj.plan_info["valid"] == 1
    # the oracle on the final positions and the new types
    pos = sim.state.pos.cpu().numpy()
    box = oracle.make_box(cfg["L"])
    rc = np.array([[r_cut["AA"], r_cut["AB"]], [r_cut["AB"], r_cut["BB"]]])
    params = np.array([oracle.pack_pair_params(PLJ, table["".join(sorted("AB"[i] + "AB"[j]))]) for i in range(2) for j in range(2)])
    onl = oracle.build_nlist(pos, box, rc + r_buff, ntypes=2, half=True)
    f_ref = oracle.pair_forces(PLJ, pos, box, onl, params, rc, 0.0, "shift", ntypes=2, half=True)
    got = np.c_[plj.forces, plj.energies]
    scale = np.abs(f_ref).max()
    err = np.abs(got - f_ref).max()
    print("force error after the type change: %.3g of %.3g" % (err, scale))
    assert np.all(np.isfinite(got)) and err <= TOL * scale
    # and the forces of the old types would have failed this check by far: the change matters
    old = pos.copy()
    old[:, 3] = syn.pos4(pos[:, :3], was)[:, 3]
    f_old = oracle.pair_forces(PLJ, old, box, oracle.build_nlist(old, box, rc + r_buff, ntypes=2, half=True), params, rc, 0.0,
                               "shift", ntypes=2, half=True)
    assert np.abs(f_old - f_ref).max() > 1e-3 * scale


# -- a small drying run ----------------------------------------------------------------------------------------------
def test_drying_film_end_to_end():
    """N = 10,648 PerturbedLJ solvent particles under a planar harmonic barrier that moves down, an evaporator taking
    Nmax = 40 per period of 10 steps out of a slab: after n periods exactly n Nmax particles are evaporated, the slab
    held at least Nmax candidates at every update, and nothing that was never a candidate has been flipped."""
    import azplugins_amd as azp
    from azplugins_amd.evaporate import ParticleEvaporator

    cfg = syn.config_plj_sc(22)
    n = cfg["xyz"].shape[0]
    L = cfg["L"]
    tagv = np.arange(n, dtype=np.uint64)
    vel = np.stack([syn.normal(43, tagv, c) for c in range(3)], axis=1)
    snap = azp.Snapshot.from_arrays(cfg["xyz"], L, types=("S", "E"), velocity=vel - vel.mean(axis=0))
    sim = azp.Simulation(device="cuda:0", seed=12)
    sim.create_state_from_snapshot(snap)
    nl = azp.nlist.Cell(buffer=0.4)
    plj = azp.pair.PerturbedLennardJones(nlist=nl, default_r_cut=2.5, mode="shift")
    plj.params[("S", "S")] = cfg["params"]
    plj.params[("S", "E")] = dict(epsilon=0.0, sigma=1.0, attraction_scale_factor=0.0)
    plj.params[("E", "E")] = dict(epsilon=0.0, sigma=1.0, attraction_scale_factor=0.0)
    wall = azp.external.PlanarHarmonicBarrier(location=lambda t: 0.4 * L[1] - 0.002 * t)
    wall.params["S"] = dict(k=50.0, offset=0.0)
    wall.params["E"] = dict(k=0.0, offset=0.0)
    sim.operations.integrator = azp.Integrator(dt=0.002, forces=[plj, wall], methods=[azp.ConstantVolume()])
    Nmax, period, periods = 40, 10, 6
    lo, hi = 0.25 * L[2], 0.45 * L[2]
    ev = ParticleEvaporator(trigger=period, solvent_type="S", evaporated_type="E", lo=lo, hi=hi, Nmax=Nmax)
    sim.operations.add(ev)
    ever_candidate = np.zeros(n, dtype=bool)
    for k in range(periods):
        # the candidates of the update that the next run(period) starts with
        st = sim.state
        tag = st.tag[: st.N].cpu().numpy().view(np.uint32).astype(np.int64)
        ever_candidate[tag[ref.candidates(st.pos[: st.N, 2].cpu().numpy(), st.typeid_host, 0, lo, hi)]] = True
        assert sim.timestep == k * period
        sim.run(period)
        assert ev.n_candidates >= Nmax, "update %d had %d candidates" % (k, ev.n_candidates)
        assert ev.n_evaporated == Nmax
        assert int((sim.state.typeid_host == 1).sum()) == (k + 1) * Nmax
    types = _types_by_tag(sim)
    assert int((types == 1).sum()) == periods * Nmax
    assert not np.any((types == 1) & ~ever_candidate)
    assert nl.num_builds >= periods and np.all(np.isfinite(sim.state.pos.cpu().numpy()[:, :3]))


# -- nothing else is disturbed ---------------------------------------------------------------------------------------
def test_updater_without_particles_changes_nothing_else():
    """A TypeUpdater whose two types no particle has: positions and velocities after a run equal, bit for bit, those
    of the same run without it in which the lists are rebuilt at the same steps."""
    import azplugins_amd as azp
    from azplugins_amd.update import TypeUpdater

    def run(with_updater):
        cfg = syn.config_plj_sc(16)
        n = cfg["xyz"].shape[0]
        tagv = np.arange(n, dtype=np.uint64)
        vel = np.stack([syn.normal(45, tagv, c) for c in range(3)], axis=1)
        snap = azp.Snapshot.from_arrays(cfg["xyz"], cfg["L"], types=("A", "X", "Y"), velocity=vel - vel.mean(axis=0))
        sim = azp.Simulation(device="cuda:0", seed=2)
        sim.create_state_from_snapshot(snap)
        sim.operations.tuners.clear()
        nl = azp.nlist.Cell(buffer=0.4)
        plj = azp.pair.PerturbedLennardJones(nlist=nl, default_r_cut=2.5, mode="shift")
        for a_ in ("A", "X", "Y"):
            for b_ in ("A", "X", "Y"):
                plj.params[(a_, b_)] = cfg["params"]
        sim.operations.integrator = azp.Integrator(dt=0.004, forces=[plj], methods=[azp.ConstantVolume()])
        if with_updater:
            sim.operations.add(TypeUpdater(trigger=7, inside_type="X", outside_type="Y", lo=-3.0, hi=3.0))
        else:
            # no updater: the list is told to rebuild at the force evaluations that follow the steps at which the
            # updater runs (it runs at t = 0, 7, 14, 21, 28; the next evaluation is at t + 1)
            due, inner_compute, inner_allows = {1, 8, 15, 22, 29}, nl.compute, nl.allows_speculative_launch

            def compute(state, force=False, compact=False):
                if sim.timestep in due:
                    due.discard(sim.timestep)
                    force = True
                return inner_compute(state, force=force, compact=compact)

            nl.compute = compute
            nl.allows_speculative_launch = lambda state: sim.timestep not in due and inner_allows(state)
        sim.run(30)
        st = sim.state
        return st.pos.cpu().numpy().copy(), st.vel.cpu().numpy().copy(), nl.num_builds

    pos_a, vel_a, builds_a = run(True)
    pos_b, vel_b, builds_b = run(False)
    np.testing.assert_array_equal(pos_a.view(np.uint64), pos_b.view(np.uint64))
    np.testing.assert_array_equal(vel_a.view(np.uint64), vel_b.view(np.uint64))
    assert builds_a == builds_b >= 6


# -- decomposed ------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


DD = dict(steps=40, dt=0.005, period=5, Nmax=25, lo=-3.0, hi=2.5, margin=1e-6)


def _dd_config():
    cfg = syn.config_plj_sc(16)
    n = cfg["xyz"].shape[0]
    tagv = np.arange(n, dtype=np.uint64)
    v = np.stack([syn.normal(51, tagv, c) for c in range(3)], axis=1) * np.sqrt(1.5)
    cfg["vel"] = v - v.mean(axis=0)
    cfg["typeid"] = (syn.hash64(13, tagv, 5) % np.uint64(3)).astype(np.int64)
    cfg["types"] = ("A", "S", "E")
    return cfg


def _dd_setup(azp, sim, cfg):
    from azplugins_amd.evaporate import ParticleEvaporator

    nl = azp.nlist.Cell(buffer=cfg["r_buff"])
    plj = azp.pair.PerturbedLennardJones(nlist=nl, default_r_cut=cfg["r_cut"], mode="shift")
    for a_ in cfg["types"]:
        for b_ in cfg["types"]:
            gone = "E" in (a_, b_)
            plj.params[(a_, b_)] = dict(epsilon=0.0 if gone else 1.0, sigma=1.0, attraction_scale_factor=0.5)
    sim.operations.integrator = azp.Integrator(dt=DD["dt"], forces=[plj], methods=[azp.ConstantVolume()])
    ev = ParticleEvaporator(trigger=DD["period"], solvent_type="S", evaporated_type="E", lo=DD["lo"], hi=DD["hi"], Nmax=DD["Nmax"])
    sim.operations.add(ev)
    return nl, ev


def _dd_worker(rank, world, port, out_dir):
    import torch
    import torch.distributed as dist

    import azplugins_amd as azp
    from azplugins_amd import decomposition as dd

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    cfg = _dd_config()
    dec = dd.Decomposition(cfg["L"], world, cfg["r_cut"] + cfg["r_buff"])
    mine = np.flatnonzero(dec.owner(cfg["xyz"]) == rank)
    snap = azp.Snapshot.from_arrays(cfg["xyz"][mine], cfg["L"], typeid=cfg["typeid"][mine], types=cfg["types"],
                                    tag=mine.astype(np.uint32), velocity=cfg["vel"][mine])
    sim, dom = dd.rank_simulation_from_snapshot(snap, cfg["xyz"].shape[0], dec, rank, "cuda:0", seed=4)
    nl, ev = _dd_setup(azp, sim, cfg)
    counts = []
    for _ in range(DD["steps"] // DD["period"]):
        sim.run(DD["period"])
        counts.append((ev.n_candidates, ev.n_evaporated))
    torch.cuda.synchronize()
    st = sim.state
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), tag=st.tag[: st.N].cpu().numpy().view(np.uint32), typeid=st.typeid_host,
             rebuilds=np.array([dom.num_rebuilds]), migrated=np.array([dom.num_migrated]), counts=np.array(counts))
    dist.barrier()
    dist.destroy_process_group()


def test_decomposed_evaporation_matches_single_domain(tmp_path):
    import torch
    import torch.multiprocessing as mp

    import azplugins_amd as azp

    world = 2
    mp.spawn(_dd_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    cfg = _dd_config()
    n = cfg["xyz"].shape[0]
    snap = azp.Snapshot.from_arrays(cfg["xyz"], cfg["L"], typeid=cfg["typeid"], types=cfg["types"], velocity=cfg["vel"])
    sim = azp.Simulation(device="cuda:0", seed=4)
    sim.create_state_from_snapshot(snap)
    sim.operations.tuners.clear()
    nl, ev = _dd_setup(azp, sim, cfg)
    counts = []
    closest = np.inf
    for _ in range(DD["steps"] // DD["period"]):
        # the update at the start of this stretch sees these positions: no solvent particle may sit so close to a
        # face of the slab that round-off between the two runs could decide on which side it is
        st = sim.state
        z = st.pos[:, 2].cpu().numpy()[st.typeid_host == 1]
        closest = min(closest, np.abs(z - DD["lo"]).min(), np.abs(z - DD["hi"]).min())
        sim.run(DD["period"])
        counts.append((ev.n_candidates, ev.n_evaporated))
    torch.cuda.synchronize()
    print("closest approach of a solvent particle to a slab face at an update: %.3g" % closest)
    assert closest > DD["margin"]
    want = _types_by_tag(sim)
    got = np.full(n, -1, dtype=np.int64)
    migrated = 0
    for r in range(world):
        d = np.load(os.path.join(str(tmp_path), "rank%d.npz" % r))
        got[d["tag"].astype(np.int64)] = d["typeid"]
        assert int(d["rebuilds"][0]) >= DD["steps"] // DD["period"]  # every update re-selects the ghosts
        migrated += int(d["migrated"][0])
        np.testing.assert_array_equal(d["counts"], np.array(counts))  # the counts are global, and the same
    assert migrated > 0, "the run must move particles between the ranks"
    np.testing.assert_array_equal(got, want)
    assert int((want == 2).sum()) - int((cfg["typeid"] == 2).sum()) == DD["Nmax"] * (DD["steps"] // DD["period"])
