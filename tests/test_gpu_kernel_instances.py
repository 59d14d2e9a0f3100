"""Every instance of the pair kernels, pinned against the CPU oracle.

The LDS variant of a tile launch follows from the plan's largest staged set (pair_plan.hpp: plan_cap_for). The tests
build configurations whose fullest tile stages exactly K particles (staged_sets.staged_set_config), check the plan
compiler's per-tile counts against the numpy restatement, assert from the plan and from the launch record
(azp_last_launch: the dynamic LDS bytes restate the instance's layout) that the intended instance ran, and compare
forces, energies, virials and torques with the oracle at the suite's bars. The per-type-pair table shares the LDS with
the staged slots, so a tile instance runs out of room before the generic kernel does: the call then runs the generic
kernel, and fails only where that one cannot hold the table either."""

import ctypes as C
import functools

import numpy as np
import pytest

import helpers as H
import staged_sets as S
from azplugins_amd import _lib
from azplugins_amd import synthetic as syn
from test_gpu_parity import PAIR_LDS_BYTES, assert_close, assert_per_particle

pytestmark = pytest.mark.gpu

ISO = ["PerturbedLennardJones", "Hertz", "ExpandedYukawa", "Colloid", "DPDConservative"]
KINDS = ISO + ["dpd", "tpm"]
MODE = dict({n: "shift" for n in ISO}, dpd="none", tpm="shift")
CAPS = [1024, 1536, 1664, 2048, 2560]
R_BUFF = 0.3
LDS_LIMIT = 160 * 1024
DPD_KW = dict(kT=1.0, dt=0.01, seed=7, timestep=4242)
_PACK = {"dpd": "DPDGeneralWeight", "tpm": "TwoPatchMorse"}
_ENTRY = dict(H.ENTRY, dpd="azp_dpd_forces_general_weight", tpm="azp_aniso_forces_two_patch_morse")


def _radius(i):
    return 0.0 if i == 0 else 0.15 + 0.004 * i  # Colloid: type 0 solvent, the others colloids


def _pair_fn(name):
    """Parameters of type pair (i <= j), finite at the configurations' closest separations (~0.8) for any type count."""
    return {
        "PerturbedLennardJones": lambda i, j: dict(epsilon=1.0 + 0.01 * (i + j), sigma=0.9 - 0.003 * (i + j),
                                                   attraction_scale_factor=0.5 - 0.004 * i),
        "Hertz": lambda i, j: dict(epsilon=2.0 + 0.05 * (i + j)),
        "ExpandedYukawa": lambda i, j: dict(epsilon=1.0 + 0.02 * (i + j), kappa=1.2, delta=0.004 * (i + j)),
        "Colloid": lambda i, j: dict(A=40.0 + 0.5 * (i + j), a_1=_radius(i), a_2=_radius(j), sigma=0.35),
        "DPDConservative": lambda i, j: dict(A=25.0 - 0.2 * (i + j), gamma=4.5, s=0.5),
        "dpd": lambda i, j: dict(A=25.0 - 0.2 * (i + j), gamma=4.5 + 0.05 * (i + j), s=0.5 + 0.01 * (i + j)),
        "tpm": lambda i, j: dict(M_d=1.8341 + 0.01 * (i + j), M_r=0.0302, r_eq=1.0043, omega=5.0, alpha=0.40,
                                 repulsion=bool((i + j) % 2)),
    }[name]


@functools.lru_cache(maxsize=None)
def _params(name, T):
    import oracle

    fn = _pair_fn(name)
    return np.array([oracle.pack_pair_params(_PACK.get(name, name), fn(min(i, j), max(i, j)))
                     for i in range(T) for j in range(T)])


def _cutoffs(T, rc, mode):
    r_cut = np.full((T, T), rc)
    if T > 1:
        r_cut[0, 1] = r_cut[1, 0] = rc - 0.3
    r_on = 0.8 * r_cut
    if T > 2 and mode == "xplor":
        r_on[2, 2] = r_cut[2, 2] + 0.1  # r_on > r_cut: xplor degenerates to shift for this pair
    return r_cut, r_on


@functools.lru_cache(maxsize=None)
def _sys(key, T):
    """(pos, L, list, r_list) of a system: "small" (512 particles), or (K, tb, pad) for staged_set_config."""
    import oracle

    if key == "small":
        pos, L, _ = H.lattice_config(8, 1.0, 0.08, seed=5, ntypes=T)
        return pos, L, oracle.build_nlist(pos, oracle.make_box(L), 2.8, ntypes=T), 2.8
    cfg = S.staged_set_config(*key)
    pos = cfg["pos"]
    if T > 1:
        typeid = (syn.hash64(3, np.arange(cfg["N"], dtype=np.uint64), 7) % np.uint64(T)).astype(np.int64)
        pos = syn.pos4(pos[:, :3], typeid)
    return pos, cfg["L"], cfg["nl"], cfg["r_list"]


@functools.lru_cache(maxsize=None)
def _extras(n):
    """Velocities (mass 1), tags and orientations of n particles (DPD thermostat, TwoPatchMorse)."""
    tag = np.arange(n, dtype=np.uint64)
    vel = np.ones((n, 4))
    vel[:, :3] = np.stack([syn.normal(6, tag, c) for c in range(3)], axis=1)
    return vel, tag.astype(np.uint32), syn.random_quaternions(n, 9)


@functools.lru_cache(maxsize=None)
def _stages(key, tile):
    pos, L, nl, _ = _sys(key, 1)
    return S.stage_sizes(nl, pos.shape[0], pos.shape[0], tile)


@functools.lru_cache(maxsize=None)
def _ref(name, T, mode, key):
    """The oracle's (force, torque or None, virial); computed once per system, potential, type count and mode."""
    import oracle

    pos, L, nl, r_list = _sys(key, T)
    r_cut, r_on = _cutoffs(T, r_list - R_BUFF, mode)
    box = oracle.make_box(L)
    vel, tag, q = _extras(pos.shape[0])
    if name == "dpd":
        f, v = oracle.dpd_forces(pos, vel, tag, box, nl, _params(name, T), r_cut, ntypes=T, virial=True, **DPD_KW)
        return f, None, v
    if name == "tpm":
        return oracle.aniso_forces_tpm(pos, q, box, nl, _params(name, T), r_cut, mode, ntypes=T, virial=True)
    f, v = oracle.pair_forces(name, pos, box, nl, _params(name, T), r_cut, r_on, mode, ntypes=T, virial=True, nthreads=8)
    return f, None, v


def _run(name, T, mode, virial, tpp, key, how):
    """One call of the potential's entry point on NaN-prefilled outputs. how: "generic" (AZP_PAIR_FLAG_NO_AUTO_PLAN),
    "planned" (a plan compiled from the list, the *_planned entry), "auto" (the HOOMD-signature entry, libazp's plan
    cache). Returns a dict: status, force, torque, virial, plan info, launch record, plan, and again(prange, fill) that
    launches the same plan once more (rows [first, first + count) only when prange is given)."""
    import torch

    pos, L, nl, r_list = _sys(key, T)
    n = pos.shape[0]
    r_cut, r_on = _cutoffs(T, r_list - R_BUFF, mode)
    a, t = H.gpu_pair_args(pos, (L,), nl, T, r_cut, r_on, mode, virial, tpp=tpp,
                           r_list_max=r_list if how == "planned" else 0.0, auto_plan=(how == "auto"))
    p = H._dev(_params(name, T))
    vel, tag, q = _extras(n)
    keep = [p]
    tq = None
    if name == "dpd":
        s = _lib.DPDArgs()
        keep += [H._dev(vel, np.float64), H._dev(tag, np.uint32)]
        s.d_vel, s.d_tag = keep[1].data_ptr(), keep[2].data_ptr()
        s.timestep, s.deltaT, s.T, s.seed = DPD_KW["timestep"], DPD_KW["dt"], DPD_KW["kT"], DPD_KW["seed"]
    elif name == "tpm":
        s = _lib.AnisoArgs()
        keep.append(H._dev(q, np.float64))
        tq = torch.full((n, 4), float("nan"), dtype=torch.float64, device="cuda:0")
        s.d_orientation, s.d_torque = keep[1].data_ptr(), tq.data_ptr()
    else:
        s = None
    lib = _lib.lib()
    entry = _ENTRY[name]
    plan = info = None
    if how == "planned":
        plan = _lib.PairPlan()
        plan.build(a, H._stream())
        info = plan.info()
        entry = entry.replace("_forces_", "_forces_planned_")

    def again(prange=None, fill=float("nan")):
        assert keep  # (the payload buffers live as long as the launcher)
        a.range_first, a.range_count = prange if prange else (0, 0)
        t["force"].fill_(fill)
        t["virial"].fill_(fill)
        if tq is not None:
            tq.fill_(fill)
        if s is not None:
            s.pair = a
        st = C.byref(s if s is not None else a)
        rc = getattr(lib, entry)(*(([plan.handle] if plan else []) + [st, p.data_ptr(), H._stream()]))
        torch.cuda.synchronize()
        return dict(rc=rc, f=t["force"].cpu().numpy(), v=t["virial"].cpu().numpy(),
                    tq=tq.cpu().numpy() if tq is not None else None, launch=_lib.last_launch())

    out = again()
    out.update(info=info, plan=plan, again=again, key=key)
    return out


def _check(out, ref, virial, what):
    assert out["rc"] == 0, "%s: status %d" % (what, out["rc"])
    f_ref, t_ref, v_ref = ref
    assert_close(out["f"][:, :3], f_ref[:, :3], what=what + " force")
    assert_close(out["f"][:, 3], f_ref[:, 3], what=what + " energy")
    if virial:
        assert_close(out["v"], v_ref, what=what + " virial")
    if t_ref is not None:
        assert_close(out["tq"][:, :3], t_ref[:, :3], what=what + " torque")
    assert_per_particle(out["f"], f_ref)


def _check_stages(out):
    """The plan compiler's staged-set sizes equal the restatement (staged_sets.stage_sizes) tile by tile."""
    info = out["info"]
    if info["valid"]:
        assert np.array_equal(out["plan"].tile_stage(), _stages(out["key"], info["tile_size"]))
        assert info["max_stage"] == _stages(out["key"], info["tile_size"]).max()


def _tile_lds(cap, T, name):
    """Dynamic LDS of pair_forces_tiled_kernel (launch_tiled_instance2): x | y | z with a stride of CAP + 1 slots, and
    for several types the types of the slots, 8 bytes, and per type pair the coefficients and r_on^2."""
    lds = (cap + 1) * 24
    return lds if T == 1 else lds + cap * 4 + 8 + PAIR_LDS_BYTES[name] * T * T


def _xtiled_lds(name, cap, T):
    """Dynamic LDS of xtiled_kernel (xtiled_lds_slots + the coefficient table): x | y | z, three payload doubles, the
    tags (DPD), the types (several types)."""
    slot = 24 + 24 + (4 if name == "dpd" else 0) + (4 if T > 1 else 0)
    return cap * slot + (_generic_bytes(name) * T * T if T > 1 else 0)


@functools.lru_cache(maxsize=None)
def _generic_bytes(name):
    """Bytes per type pair of the generic kernel's LDS table, read from the launch records of two launches."""
    lds = [_run(name, T, MODE[name], False, 1, "small", "generic")["launch"]["lds_bytes"] for T in (2, 3)]
    per = (lds[1] - lds[0]) // 5
    assert per > 0 and lds == [4 * per, 9 * per], lds
    return per


def _largest_generic_T(name):
    per = _generic_bytes(name)
    T = 1
    while (T + 1) ** 2 * per <= LDS_LIMIT:
        T += 1
    return T


# ---------------------------------------------------------------------------
# pair_forces_tiled_kernel<E, TPP, CAP, VIRIAL, SINGLE, XPLOR>: one test per instance
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("virial", [False, True], ids=["plain", "virial"])
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("tpp", [1, 2, 4])
@pytest.mark.parametrize("T,mode", [(1, "none"), (1, "shift"), (1, "xplor"), (3, "shift"), (3, "xplor")])
@pytest.mark.parametrize("name", ISO)
def test_tile_instance(name, T, mode, tpp, cap, virial):
    """The fullest tile stages CAP - 1 particles: the variant's last slot is filled."""
    key = (cap - 1, 256 // tpp, 0)
    out = _run(name, T, mode, virial, tpp, key, "planned")
    info, launch = out["info"], out["launch"]
    assert info["valid"] == 1 and info["lds_slots"] == cap and info["threads_per_particle"] == tpp, info
    assert launch["threads_per_particle"] == tpp and launch["lds_bytes"] == _tile_lds(cap, T, name), launch
    _check_stages(out)
    _check(out, _ref(name, T, mode, key), virial, "%s T=%d %s tpp=%d cap=%d" % (name, T, mode, tpp, cap))


@pytest.mark.parametrize("K,cap", [(1023, 1024), (1024, 1536), (1535, 1536), (1536, 1664), (1663, 1664), (1664, 2048),
                                   (2047, 2048), (2048, 2560), (2559, 2560)])
@pytest.mark.parametrize("name", ["PerturbedLennardJones", "Colloid"])
def test_fill_boundary(name, K, cap):
    """A staged set of CAP - 1 takes the variant, one more takes the next."""
    assert S.cap_for(K) == cap
    key = (K, 256, 0)
    out = _run(name, 3, "xplor", True, 1, key, "planned")
    assert out["info"]["valid"] == 1 and out["info"]["max_stage"] == K and out["info"]["lds_slots"] == cap
    assert out["launch"]["lds_bytes"] == _tile_lds(cap, 3, name)
    _check_stages(out)
    _check(out, _ref(name, 3, "xplor", key), True, "%s K=%d" % (name, K))


def test_staged_set_over_budget():
    """2,560 staged particles do not fit beside the dummy slot: with a fixed lane count the plan is invalid (reason 2)
    and the planned entry runs the generic kernel; left to the compiler, the tile is halved and the plan is valid."""
    name, key = "PerturbedLennardJones", (2560, 256, 0)
    ref = _ref(name, 3, "shift", key)
    out = _run(name, 3, "shift", True, 1, key, "planned")
    assert out["info"]["valid"] == 0 and out["info"]["invalid_reason"] == 2
    assert out["launch"]["lds_bytes"] == PAIR_LDS_BYTES[name] * 9  # the generic kernel
    _check(out, ref, True, "invalid plan, generic kernel")
    out = _run(name, 3, "shift", True, 0, key, "planned")
    info = out["info"]
    assert info["valid"] == 1 and info["threads_per_particle"] == 2 and info["tile_size"] == 128, info
    assert out["launch"]["threads_per_particle"] == 2 and out["launch"]["lds_bytes"] == _tile_lds(info["lds_slots"], 3, name)
    _check_stages(out)
    _check(out, ref, True, "128-particle tiles")


@pytest.mark.parametrize("big", [2048, 2560])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("name", ISO)
def test_largest_lds_variants(name, T, big):
    """A plan in which most tiles would fit 1,664 slots and a few need `big`: one launch of the `big`-slot instance."""
    key = (big - 1, 256, S.LIQUID)  # as many isolated particles as liquid ones: half the tiles stage nothing
    stage = _stages(key, 256)
    large = int((stage + 1 > 1664).sum())
    assert 2 * (stage.size - large) >= stage.size and large > 0
    out = _run(name, T, "shift", True, 1, key, "planned")
    assert out["launch"]["lds_bytes"] == _tile_lds(big, T, name)
    assert out["launch"]["grid"] == (stage.size + 7) & ~7
    _check(out, _ref(name, T, "shift", key), True, "largest LDS variants")


def test_sub_range_launch_takes_the_smaller_instance():
    """A range whose tiles all fit a smaller variant than the plan's fullest tile runs that variant; its rows equal the
    full launch's bit for bit; rows outside the range, rounded outwards to whole tiles, keep their values."""
    name, T, key = "PerturbedLennardJones", 3, (2047, 256, 0)
    stage = _stages(key, 256)
    caps = np.array([S.cap_for(int(x)) for x in stage])
    t0 = int(np.flatnonzero((caps < 2048) & (stage > 0))[0])
    t1 = t0
    while t1 < stage.size and caps[t1] < 2048:
        t1 += 1
    cap = int(caps[t0:t1].max())
    full = _run(name, T, "shift", True, 1, key, "planned")
    assert full["info"]["lds_slots"] == 2048
    first, end = t0 * 256 + 5, t1 * 256 - 9
    part = full["again"]((first, end - first), fill=7.0)
    assert part["rc"] == 0 and part["launch"]["lds_bytes"] == _tile_lds(cap, T, name), (cap, part["launch"])
    rows = slice(t0 * 256, t1 * 256)
    assert np.array_equal(part["f"][rows], full["f"][rows]) and np.array_equal(part["v"][:, rows], full["v"][:, rows])
    outside = np.ones(full["f"].shape[0], dtype=bool)
    outside[rows] = False
    assert np.all(part["f"][outside] == 7.0) and np.all(part["v"][:, outside] == 7.0)


# ---------------------------------------------------------------------------
# xtiled_kernel<X, CAP, VIRIAL, SINGLE>: DPD thermostat and TwoPatchMorse
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("virial", [False, True], ids=["plain", "virial"])
@pytest.mark.parametrize("K,cap", [(1023, 1024), (1535, 1536), (1663, 2048), (2047, 2048), (2559, 2560)])
@pytest.mark.parametrize("T", [1, 2])
@pytest.mark.parametrize("name", ["dpd", "tpm"])
def test_xtiled_instance(name, T, K, cap, virial):
    """1,664 staged slots run the 2,048-slot instance."""
    key = (K, 256, 0)
    out = _run(name, T, MODE[name], virial, 1, key, "planned")
    assert out["info"]["valid"] == 1 and out["info"]["max_stage"] == K and out["info"]["threads_per_particle"] == 1
    assert out["launch"]["lds_bytes"] == _xtiled_lds(name, cap, T), out["launch"]
    _check_stages(out)
    _check(out, _ref(name, T, MODE[name], key), virial, "%s T=%d K=%d" % (name, T, K))


# ---------------------------------------------------------------------------
# pair_forces_kernel<X, TPP, VIRIAL, SINGLE>: every policy
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("virial", [False, True], ids=["plain", "virial"])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("tpp", [1, 2, 4, 8, 16, 32])
@pytest.mark.parametrize("name,mode", [(n, m) for n in ISO for m in ("shift", "xplor")] + [("dpd", "none"), ("tpm", "shift")])
def test_generic_instance(name, mode, tpp, T, virial):
    out = _run(name, T, mode, virial, tpp, "small", "generic")
    per = PAIR_LDS_BYTES[name] if name in PAIR_LDS_BYTES else _generic_bytes(name)
    assert out["launch"]["threads_per_particle"] == tpp and out["launch"]["lds_bytes"] == (per * T * T if T > 1 else 0)
    _check(out, _ref(name, T, mode, "small"), virial, "%s %s tpp=%d T=%d" % (name, mode, tpp, T))


# ---------------------------------------------------------------------------
# type counts: the generic kernel's limit holds on every path
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", KINDS)
def test_type_count_limit(name):
    """At the generic kernel's largest type count every entry gives the oracle's answer -- the tile instances cannot
    hold that table beside their staged slots and hand the call to the generic kernel; one type more fails everywhere
    with AZP_ERROR_TOO_MANY_TYPES and leaves the outputs alone."""
    Tg, mode = _largest_generic_T(name), MODE[name]
    big = (2047, 256, 0)
    lib = _lib.lib()
    lib.azp_pair_auto_plan_clear()
    s0 = _lib.auto_plan_stats()
    for key, how, tpp in (("small", "generic", 0), ("small", "planned", 1), (big, "planned", 1), ("small", "auto", 0)):
        out = _run(name, Tg, mode, True, tpp, key, how)
        if how == "planned":
            assert out["info"]["valid"] == 1
        assert out["launch"]["lds_bytes"] == _generic_bytes(name) * Tg * Tg  # the generic kernel ran
        _check(out, _ref(name, Tg, mode, key), True, "%s T=%d %s %s" % (name, Tg, how, key))
        bad = _run(name, Tg + 1, mode, True, tpp, key, how)
        assert bad["rc"] == _lib.ERROR_TOO_MANY_TYPES, bad["rc"]
        assert np.all(np.isnan(bad["f"])) and np.all(np.isnan(bad["v"]))
        if bad["tq"] is not None:
            assert np.all(np.isnan(bad["tq"]))
    s1 = _lib.auto_plan_stats()
    assert s1["generic_fallbacks"] - s0["generic_fallbacks"] >= 3
    lib.azp_pair_auto_plan_clear()


def _sim_potential(azp, name, nl, r_cut):
    if name == "dpd":
        return azp.pair.DPDGeneralWeight(nlist=nl, kT=0.0, default_r_cut=r_cut)  # kT = 0: drag + conservative only
    if name == "tpm":
        return azp.pair.TwoPatchMorse(nlist=nl, default_r_cut=r_cut, mode="shift")
    if name == "DPDConservative":
        return azp.pair.DPDConservativeGeneralWeight(nlist=nl, default_r_cut=r_cut)
    return getattr(azp.pair, name)(nlist=nl, default_r_cut=r_cut, mode="shift")


@pytest.mark.parametrize("name", KINDS)
def test_type_count_limit_simulation(name):
    """Simulation.run at the generic kernel's largest type count: the plan compiled from the cells cannot run, the list
    leaves fused mode and the step runs on the list; forces as the oracle's. One type more raises AzpError."""
    import oracle

    import azplugins_amd as azp

    Tg = _largest_generic_T(name)
    pos, L, _, _ = _sys("small", 1)
    n = pos.shape[0]
    r_cut = 2.5
    for T in (Tg, Tg + 1):
        typeid = (syn.hash64(3, np.arange(n, dtype=np.uint64), 7) % np.uint64(T)).astype(np.int64)
        types = tuple("t%d" % i for i in range(T))
        snap = azp.Snapshot.from_arrays(pos[:, :3], L, typeid=typeid, types=types,
                                        orientation=_extras(n)[2] if name == "tpm" else None)
        sim = azp.Simulation(device="cuda:0", seed=1)
        sim.create_state_from_snapshot(snap)
        nl = azp.nlist.Cell(buffer=R_BUFF)
        pot = _sim_potential(azp, name, nl, r_cut)
        fn = _pair_fn(name)
        for i in range(T):
            for j in range(i, T):
                pot.params[(types[i], types[j])] = fn(i, j)
        sim.operations.integrator = azp.Integrator(dt=0.001, forces=[pot], methods=[azp.ConstantVolume()])
        if T > Tg:
            with pytest.raises(_lib.AzpError, match="status -2"):
                sim.run(0)
            continue
        sim.run(0 if name == "tpm" else 3)
        pot.compute(sim.timestep)
        st = sim.state
        x = st.pos[: st.N].cpu().numpy()
        box = oracle.make_box(L)
        onl = oracle.build_nlist(x, box, r_cut + R_BUFF, ntypes=T)
        params = _params(name, T)
        rc = np.full((T, T), r_cut)
        if name == "dpd":
            vel = st.vel[: st.N].cpu().numpy()
            tag = st.tag[: st.N].cpu().numpy().view(np.uint32)
            f_ref = oracle.dpd_forces(x, vel, tag, box, onl, params, rc, 0.0, 0.001, 1, 0, ntypes=T)
        elif name == "tpm":
            f_ref, _ = oracle.aniso_forces_tpm(x, st.orientation[: st.N].cpu().numpy(), box, onl, params, rc, "shift", ntypes=T)
        else:
            f_ref = oracle.pair_forces(name, x, box, onl, params, rc, 0.0, "shift" if name != "DPDConservative" else "none",
                                       ntypes=T, nthreads=8)
        assert_close(np.c_[pot.forces, pot.energies], f_ref, what="%s T=%d" % (name, T))
