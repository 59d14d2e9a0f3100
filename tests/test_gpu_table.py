"""pair.Table and bond.Table on the GPU against the numpy restatement (tests/table_ref.py) at the suite's bars:
assert_close (TOL = 1e-10 of the largest component) and assert_per_particle.

Tables are smooth random curves with U and F drawn independently (a swapped column, or a force derived from U, shows),
r_min = 0.5 below the systems' closest separation (~0.8). Every comparison prints its error as a fraction of the bar
before it asserts."""

import ctypes as C
import functools

import numpy as np
import pytest

import helpers as H
import staged_sets as S
import table_ref as R
from azplugins_amd import _lib
from azplugins_amd import synthetic as syn
from test_gpu_parity import TOL, assert_close, assert_per_particle

pytestmark = pytest.mark.gpu

R_MIN = 0.5
R_BUFF = 0.3
COEFF_BYTES = 48  # LDS per type pair: EvalTable::Coeff (40 bytes) and r_on^2
WIDTHS = {(0, 0): 1000, (0, 1): 7, (0, 2): 1, (1, 1): 7, (1, 2): 1000, (2, 2): 1}


def _close(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    scale = np.abs(ref).max()
    print("%s: error %.3g of TOL" % (what, np.abs(got - ref).max() / (TOL * (scale if scale > 0 else 1.0))))
    assert_close(got, ref, what=what)


def _samples(i, j, width):
    return R.smooth_curve(100 + 10 * i + j, width, 2.0), R.smooth_curve(200 + 10 * i + j, width, 20.0)


def _cutoffs(T, rc):
    r_cut = np.full((T, T), rc)
    if T > 1:
        r_cut[0, 1] = r_cut[1, 0] = rc - 0.3
    return r_cut


@functools.lru_cache(maxsize=None)
def _tables(T, rc):
    """Restatement tables [i][j] of a T-type system with cutoff rc (r_cut[0, 1] shorter)."""
    r_cut = _cutoffs(T, rc)
    tabs = [[None] * T for _ in range(T)]
    for i in range(T):
        for j in range(i, T):
            U, F = _samples(i, j, WIDTHS[(i, j)])
            tabs[i][j] = tabs[j][i] = R.pair_table(R_MIN, r_cut[i, j], U, F)
    return tabs


def _device_tables(tabs, closed=False):
    """(parameter structs on the device, keepalive) for restatement tables: [i][j] for pairs, a list for bonds. The rows
    come from the library's own packer (bit-checked against the restatement in tests/test_table.py)."""
    flat = [t for row in tabs for t in row] if not closed else list(tabs)
    uniq = {}
    for t in flat:
        uniq.setdefault(id(t), t)
    first, at = {}, 0
    for k, t in uniq.items():
        first[k] = at
        at += t["rows"].shape[0]
    d_rows = H._dev(np.concatenate([t["rows"] for t in uniq.values()]))
    assert d_rows.data_ptr() % 32 == 0
    entries = [(t["r_min"], t["r_end"], d_rows.data_ptr() + 32 * first[id(t)], t["rows"].shape[0]) for t in flat]
    return H._dev(_lib.table_params_rows(entries)), d_rows


@functools.lru_cache(maxsize=None)
def _sys(key, T):
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
def _ref(key, T):
    pos, L, nl, r_list = _sys(key, T)
    rc = r_list - R_BUFF
    return R.pair_forces(pos, L, nl, _tables(T, rc), _cutoffs(T, rc), ntypes=T)


def _run(key, T, virial, tpp, planned):
    import torch

    pos, L, nl, r_list = _sys(key, T)
    rc = r_list - R_BUFF
    a, t = H.gpu_pair_args(pos, (L,), nl, T, _cutoffs(T, rc), 0.0, "none", virial, tpp=tpp, r_list_max=r_list if planned else 0.0)
    p, keep = _device_tables(_tables(T, rc))
    lib = _lib.lib()
    info = None
    if planned:
        plan = _lib.PairPlan()
        plan.build(a, H._stream())
        info = plan.info()
        rc_ = lib.azp_pair_forces_planned_table(plan.handle, C.byref(a), p.data_ptr(), H._stream())
    else:
        rc_ = lib.azp_pair_forces_table(C.byref(a), p.data_ptr(), H._stream())
    torch.cuda.synchronize()
    assert rc_ == 0 and keep is not None
    return t["force"].cpu().numpy(), t["virial"].cpu().numpy(), _lib.last_launch(), info


def _check(f, v, ref, virial, what):
    f_ref, v_ref = ref
    _close(f[:, :3], f_ref[:, :3], what + " force")
    _close(f[:, 3], f_ref[:, 3], what + " energy")
    if virial:
        _close(v, v_ref, what + " virial")
    assert_per_particle(f, f_ref)


@pytest.mark.parametrize("virial", [False, True], ids=["plain", "virial"])
@pytest.mark.parametrize("tpp", [1, 4, 32])
@pytest.mark.parametrize("T", [1, 3])
def test_generic_kernel(T, tpp, virial):
    """pair_forces_kernel<XIso<EvalTable>>: 512 particles, list radius 2.8; T = 3 with widths 1, 7 and 1000 and a
    shorter r_cut[0, 1]."""
    f, v, launch, _ = _run("small", T, virial, tpp, planned=False)
    assert launch["threads_per_particle"] == tpp and launch["lds_bytes"] == (COEFF_BYTES * T * T if T > 1 else 0)
    _check(f, v, _ref("small", T), virial, "generic T=%d tpp=%d" % (T, tpp))


@pytest.mark.parametrize("virial", [False, True], ids=["plain", "virial"])
@pytest.mark.parametrize("T", [1, 3])
def test_tile_kernel_planned(T, virial):
    """pair_forces_tiled_kernel<EvalTable> through azp_pair_forces_planned_table: the fullest tile stages 1023 particles
    (the 1024-slot instance, its last slot filled); the launch record restates the tile kernel's LDS layout."""
    key = (1023, 256, 0)
    f, v, launch, info = _run(key, T, virial, 1, planned=True)
    cap = 1024
    assert info["valid"] == 1 and info["lds_slots"] == cap and info["max_stage"] == 1023 and info["threads_per_particle"] == 1
    lds = (cap + 1) * 24
    assert launch["lds_bytes"] == (lds if T == 1 else lds + cap * 4 + 8 + COEFF_BYTES * T * T), launch
    _check(f, v, _ref(key, T), virial, "tile T=%d" % T)


def test_shift_mode_is_refused():
    """A table is tabulated as the user wants it: shift and xplor are invalid arguments, and nothing is written."""
    import torch

    pos, L, nl, r_list = _sys("small", 1)
    p, keep = _device_tables(_tables(1, 2.5))
    for mode in ("shift", "xplor"):
        a, t = H.gpu_pair_args(pos, (L,), nl, 1, 2.5, 2.0, mode, True, tpp=1)
        assert _lib.lib().azp_pair_forces_table(C.byref(a), p.data_ptr(), H._stream()) == -1
        torch.cuda.synchronize()
        assert np.all(np.isnan(t["force"].cpu().numpy()))


# ---------------------------------------------------------------------------
# edge cases, two particles
# ---------------------------------------------------------------------------
def _two(r, width, r_cut=2.5):
    """Two particles r apart along (1, 2, 2) / 3 listing each other, outputs prefilled with NaN: (force, virial,
    restatement force, restatement virial, samples U, F)."""
    import torch

    e = np.array([1.0, 2.0, 2.0]) / 3.0
    pos = syn.pos4(np.stack([-0.5 * r * e, 0.5 * r * e]))
    L = np.array([20.0, 20.0, 20.0])
    nl = (np.array([1, 1], dtype=np.uint32), np.array([0, 1], dtype=np.uint64), np.array([1, 0], dtype=np.uint32))
    U, F = _samples(0, 0, width)
    tab = R.pair_table(R_MIN, r_cut, U, F)
    a, t = H.gpu_pair_args(pos, (L,), nl, 1, r_cut, 0.0, "none", True, tpp=1)
    p, keep = _device_tables([[tab]])
    assert _lib.lib().azp_pair_forces_table(C.byref(a), p.data_ptr(), H._stream()) == 0
    torch.cuda.synchronize()
    assert keep is not None
    f_ref, v_ref = R.pair_forces(pos, L, nl, [[tab]], r_cut)
    return t["force"].cpu().numpy(), t["virial"].cpu().numpy(), f_ref, v_ref, U, F


@pytest.mark.parametrize("r", [R_MIN - 0.01, 2.5 + 0.01], ids=["below_r_min", "beyond_r_cut"])
def test_outside_the_table_is_exactly_zero(r):
    f, v, f_ref, v_ref, _, _ = _two(r, 8)
    assert np.all(f == 0.0) and np.all(v == 0.0)
    assert np.all(f_ref == 0.0) and np.all(v_ref == 0.0)


def test_separation_on_a_knot():
    """Width 8 on [0.5, 2.5): knots every 0.25, all exact in float64. r = 1.25 is knot 3: U_3 and F_3, whichever side of
    the knot the device's r falls on (the interpolant is continuous)."""
    r = 1.25
    f, v, f_ref, v_ref, U, F = _two(r, 8)
    e = np.array([1.0, 2.0, 2.0]) / 3.0
    expect = np.concatenate([-F[3] * e, [0.5 * U[3]]])  # particle 0 sits at -r e / 2: d = -r e, force = d F / r
    _close(f[0], expect, "on a knot, by hand")
    _close(f, f_ref, "on a knot")
    _close(v, v_ref, "on a knot virial")
    assert np.array_equal(f[1, :3], -f[0, :3]) and f[1, 3] == f[0, 3]


def test_last_interval_goes_to_zero():
    """r = 2.4 lies in the last interval [2.25, 2.5): f = 0.6, so U = 0.4 U_7 and F = 0.4 F_7 -- toward the implicit
    zero at the cutoff, from the folded last row."""
    r = 2.4
    f, v, f_ref, v_ref, U, F = _two(r, 8)
    e = np.array([1.0, 2.0, 2.0]) / 3.0
    frac = 1.0 - (r - 2.25) / 0.25
    expect = np.concatenate([-frac * F[7] * e, [0.5 * frac * U[7]]])
    _close(f[0], expect, "last interval, by hand")
    _close(f, f_ref, "last interval")
    _close(v, v_ref, "last interval virial")


def test_width_one():
    """One sample: a single interval from (r_min, U_0) to (r_cut, 0)."""
    r = 1.5
    f, v, f_ref, v_ref, U, F = _two(r, 1)
    e = np.array([1.0, 2.0, 2.0]) / 3.0
    expect = np.concatenate([-0.5 * F[0] * e, [0.25 * U[0]]])
    _close(f[0], expect, "width 1, by hand")
    _close(f, f_ref, "width 1")
    _close(v, v_ref, "width 1 virial")


# ---------------------------------------------------------------------------
# pair.Table in a Simulation
# ---------------------------------------------------------------------------
def _liquid_sim(r_cut=2.0, velocity=False):
    import azplugins_amd as azp

    pos, L, typeid = H.lattice_config(10, 1.1, 0.11, seed=3, ntypes=2)
    n = pos.shape[0]
    vel = None
    if velocity:
        tag = np.arange(n, dtype=np.uint64)
        vel = np.stack([syn.normal(23, tag, c) for c in range(3)], axis=1)
        vel -= vel.mean(axis=0)
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(azp.Snapshot.from_arrays(pos[:, :3], L, typeid=typeid, types=("A", "B"), velocity=vel))
    nl = azp.nlist.Cell(buffer=R_BUFF)
    pot = azp.pair.Table(nlist=nl, default_r_cut=r_cut)
    for (i, j), (a, b) in {(0, 0): ("A", "A"), (0, 1): ("A", "B"), (1, 1): ("B", "B")}.items():
        U, F = _samples(i, j, (64, 7, 1000)[i + j])
        pot.params[(a, b)] = dict(r_min=R_MIN, U=0.2 * U, F=0.2 * F)
    sim.operations.integrator = azp.Integrator(dt=0.001, forces=[pot], methods=[azp.ConstantVolume()])
    return sim, nl, pot, L


def _sim_reference(sim, pot, L):
    import oracle

    st = sim.state
    x = st.pos[: st.N].cpu().numpy()
    types = ("A", "B")
    rc = np.array([[pot.r_cut[(a, b)] for b in types] for a in types])
    tabs = [[None] * 2 for _ in range(2)]
    for i, a in enumerate(types):
        for j, b in enumerate(types):
            d = pot.params[(a, b)]
            tabs[i][j] = R.pair_table(d["r_min"], rc[i, j], d["U"], d["F"])
    nl = oracle.build_nlist(x, oracle.make_box(L), rc.max(), ntypes=2)
    return R.pair_forces(x, L, nl, tabs, rc, ntypes=2)


def test_simulation_plan_paths_and_r_cut_change():
    """1000 particles, two types: the plan compiled from the cells, the plan compiled from the list and the generic
    kernel give the restatement's forces; lowering r_cut[("A", "A")] repacks that table (dr changes with r_cut)."""
    sim, nl, pot, L = _liquid_sim()
    pot.compute_virial = True
    sim.run(0)
    assert pot.plan_info["valid"] == 1 and pot.plan_info["from_cells"] == 1 and nl.fused_active
    f_ref, v_ref = _sim_reference(sim, pot, L)
    _close(np.c_[pot.forces, pot.energies], f_ref, "plan from the cells")
    _close(pot.virials.T, v_ref, "plan from the cells, virial")
    pot.use_fused_plan = False
    pot.compute(0)
    assert pot.plan_info["valid"] == 1 and pot.plan_info["from_cells"] == 0
    _close(np.c_[pot.forces, pot.energies], f_ref, "plan from the list")
    pot.use_plan = False
    pot.compute(0)
    _close(np.c_[pot.forces, pot.energies], f_ref, "generic kernel")
    _close(pot.virials.T, v_ref, "generic kernel, virial")
    assert_per_particle(np.c_[pot.forces, pot.energies], f_ref)
    pot.use_plan = pot.use_fused_plan = True
    pot.r_cut[("A", "A")] = 1.6
    pot.compute(0)
    f_low, _ = _sim_reference(sim, pot, L)
    assert np.abs(f_low - f_ref).max() > 1e-3 * np.abs(f_ref).max()  # (the change is visible)
    _close(np.c_[pot.forces, pot.energies], f_low, "after lowering r_cut")
    back = pot.params[("A", "A")]
    assert back["r_min"] == R_MIN and len(back["U"]) == 64


def test_r_cut_lowered_to_r_min_is_an_error_at_the_first_compute():
    """What only shows with the final r_cut cannot be refused when the table is set: AzpError naming the pair."""
    sim, nl, pot, L = _liquid_sim()
    pot.r_cut[("A", "B")] = R_MIN
    with pytest.raises(_lib.AzpError, match=r"\('A', 'B'\).*r_min < r_cut"):
        sim.run(0)
    pot.r_cut[("A", "B")] = 0.0  # never evaluated: fine, whatever r_min is
    sim.run(0)
    f_ref, _ = _sim_reference(sim, pot, L)
    _close(np.c_[pot.forces, pot.energies], f_ref, "r_cut[A, B] = 0")


def _by_tag(sim):
    import torch

    torch.cuda.synchronize()
    st = sim.state
    order = torch.argsort(st.tag[: st.N])
    return {name: getattr(st, name)[: st.N].index_select(0, order).cpu() for name in ("pos", "vel")}


def test_two_runs_equal_one_run_bit_for_bit():
    """run(10); run(10) ends in the bits of run(20), with the particle sorter re-indexing every 5 steps (speculative
    launches in between); the forces of the last step are the restatement's at the final, re-ordered positions."""
    import torch

    ends = []
    for pieces in ((20,), (10, 10)):
        sim, nl, pot, L = _liquid_sim(velocity=True)
        sim.operations.tuners[0].trigger_period = 5
        for steps in pieces:
            sim.run(steps)
        assert sim.timestep == 20 and sim.operations.tuners[0].num_sorts >= 3
        ends.append(_by_tag(sim))
        _close(np.c_[pot.forces, pot.energies], _sim_reference(sim, pot, L)[0], "after run%s" % (pieces,))
    start = _by_tag(_liquid_sim(velocity=True)[0])
    assert not torch.equal(ends[0]["pos"], start["pos"])
    for name in ("pos", "vel"):
        assert torch.equal(ends[0][name], ends[1][name]), name
    assert bool(torch.isfinite(ends[0]["pos"]).all())


# ---------------------------------------------------------------------------
# bond.Table
# ---------------------------------------------------------------------------
B_MIN, B_MAX = 0.5, 1.6


def _bond_samples(t):
    width = (2, 513)[t]
    return R.smooth_curve(300 + t, width, 3.0), R.smooth_curve(400 + t, width, 30.0)


def _chain_sim(stretch=False):
    """Nine chains of 64 beads (576 particles: two full workgroups and a ragged one), bond types alternating between a
    width-2 and a width-513 table on [0.5, 1.6); bond lengths 0.97 .. 1.19. stretch: one bead moved 1.5 sideways, its
    two bonds ~1.85 long."""
    import azplugins_amd as azp

    cfg = syn.config_chains(64, 3, 3, 64)
    xyz = cfg["xyz"].copy()
    assert xyz.shape[0] == 576
    if stretch:
        xyz[5, 1] += 1.5
        xyz = syn.wrap(xyz, cfg["L"])
    bonds = np.asarray(cfg["bonds"])
    btype = np.arange(len(bonds)) % 2
    snap = azp.Snapshot.from_arrays(xyz, cfg["L"], bonds=bonds, bond_typeid=btype, bond_types=("A-A", "B-B"))
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(snap)
    pot = azp.bond.Table()
    for t, name in enumerate(("A-A", "B-B")):
        U, F = _bond_samples(t)
        pot.params[name] = dict(r_min=B_MIN, r_max=B_MAX, U=U, F=F)
    sim.operations.integrator = azp.Integrator(dt=0.001, forces=[pot])
    sim.operations.tuners.clear()  # (memory order = snapshot order: the reference below uses the snapshot's arrays)
    return sim, pot, syn.pos4(xyz), cfg["L"], bonds, btype


@pytest.mark.parametrize("virial", [False, True], ids=["plain", "virial"])
def test_bond_table(virial):
    sim, pot, pos, L, bonds, btype = _chain_sim()
    pot.compute_virial = virial
    sim.run(0)
    tabs = [R.bond_table(B_MIN, B_MAX, *_bond_samples(t)) for t in range(2)]
    f_ref, bad, v_ref = R.bond_forces(pos, L, bonds, btype, tabs)
    assert bad == 0
    _close(np.c_[pot.forces, pot.energies], f_ref, "bond force and energy")
    if virial:
        _close(pot.virials.T, v_ref, "bond virial")
    assert_per_particle(np.c_[pot.forces, pot.energies], f_ref)
    back = pot.params["B-B"]
    assert back["r_max"] == B_MAX and len(back["U"]) == 513


def test_bond_out_of_bounds_raises_and_the_process_goes_on():
    """A bond past r_max is rejected by the evaluator before it reads the table: the kernel's flag word, "bond out of
    bounds" on the host. The next, unstretched system computes as if nothing had happened."""
    sim, pot, pos, L, bonds, btype = _chain_sim(stretch=True)
    tabs = [R.bond_table(B_MIN, B_MAX, *_bond_samples(t)) for t in range(2)]
    assert R.bond_forces(pos, L, bonds, btype, tabs)[1] == 2
    with pytest.raises(_lib.AzpError, match="bond out of bounds"):
        sim.run(0)
        pot.check_flags()
    sim, pot, pos, L, bonds, btype = _chain_sim()
    sim.run(0)
    pot.check_flags()
    f_ref, bad, _ = R.bond_forces(pos, L, bonds, btype, tabs)
    _close(np.c_[pot.forces, pot.energies], f_ref, "after the rejected bond")
