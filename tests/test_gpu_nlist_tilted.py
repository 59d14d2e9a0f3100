"""The cell list in tilted boxes: fractional cells (azp_nlist_args.fractional_cells = 1, csrc/nlist.hip) through the C
ABI, nlist.Cell and Simulation.run.

Rows are compared with the all-pairs FP64 reference of tests/nlist_ref.py as exact sets, every row of every case, on
configurations without a borderline pair (the discipline of tests/test_gpu_nlist_rows.py, whose checks are reused).
Which kernel instance a grid selects: the minimum image per pair (MI = true) when some periodic axis has fewer than 4
cells, else the image of every staged particle fixed once relative to the home cell's centre in fractional
coordinates (MI = false, FRAC = true)."""

import ctypes as C
import functools

import numpy as np
import pytest

import box_ref
import helpers as H
import nlist_ref as R
import nlist_tilted_cases as T
import test_gpu_nlist_rows as ROWS
from azplugins_amd import _lib, nlist
from azplugins_amd import synthetic as syn

pytestmark = pytest.mark.gpu

SENT = H.NLIST_SENTINEL
TOL = 1e-10  # tests/test_gpu_parity.py::test_triclinic_box: max |F - F_ref| <= 1e-10 max |F_ref|
L_BIG = (9.0, 8.0, 7.5)
RL_TYPED = np.array([[1.5, 1.1], [1.1, 0.0]])  # two types, the pair 1-1 disabled


# ---------------------------------------------------------------------------
# binning and rows through the C ABI
# ---------------------------------------------------------------------------
def bin_cells(cfg, fractional=1, binning="native", dims=None):
    """azp_nlist_args for ``cfg`` with ``fractional_cells = fractional``, binned by azp_nlist_bin ("native") or by
    azp_nlist_cell_assign + the framework's stable sort + azp_nlist_cell_bounds ("sort"); (args, keepalive) as
    helpers.gpu_cells returns them, for helpers.gpu_nlist_rows. ``dims``: cells per axis instead of nlist.cell_grid's."""
    import torch

    import azplugins_amd as azp

    pos = np.ascontiguousarray(cfg["pos"], dtype=np.float64)
    L, tilt, periodic = cfg["L"], cfg.get("tilt", (0.0, 0.0, 0.0)), cfg["periodic"]
    rl = np.asarray(cfg["rl"], dtype=np.float64)
    n_total, N, ntypes = pos.shape[0], cfg["N"], rl.shape[0]
    if dims is None:
        dims = nlist.cell_grid(azp.Box(*L, xy=tilt[0], xz=tilt[1], yz=tilt[2], periodic=periodic), float(rl.max()))[0]
    a = _lib.NlistArgs()
    a.N, a.n_total, a.ntypes = N, n_total, ntypes
    t = dict(pos=H._dev(pos), rlistsq=H._dev((rl * rl).reshape(-1)))
    a.d_pos = t["pos"].data_ptr()
    a.d_rlistsq = t["rlistsq"].data_ptr()
    a.box = _lib.make_box(L, tilt, periodic)
    a.cell_subdivision = 1
    a.fractional_cells = fractional
    for k in range(3):
        a.grid.dim[k] = int(dims[k])
        a.grid.lo[k] = -0.5 if fractional else -0.5 * L[k]
        a.grid.width[k] = (1.0 if fractional else L[k]) / int(dims[k])
        a.grid.periodic[k] = 1 if periodic[k] else 0
    ncell = int(np.prod(dims))
    t["cell_of"] = torch.empty(n_total, dtype=torch.int32, device="cuda:0")
    t["cell_start"] = torch.empty(ncell + 1, dtype=torch.int32, device="cuda:0")
    a.d_cell_of = t["cell_of"].data_ptr()
    a.d_cell_start = t["cell_start"].data_ptr()
    l = _lib.lib()
    if binning == "native":
        t["order"] = torch.empty(n_total, dtype=torch.int32, device="cuda:0")
        t["cursor"] = torch.empty(ncell, dtype=torch.int32, device="cuda:0")
        t["order_tmp"] = torch.empty(n_total, dtype=torch.int32, device="cuda:0")
        a.d_order = t["order"].data_ptr()
        _lib.check(l.azp_nlist_bin(C.byref(a), t["cursor"].data_ptr(), t["order_tmp"].data_ptr(), H._stream()), "azp_nlist_bin")
    else:
        assert binning == "sort"
        _lib.check(l.azp_nlist_cell_assign(C.byref(a), H._stream()), "azp_nlist_cell_assign")
        t["cell_sorted"], order = torch.sort(t["cell_of"], stable=True)
        t["order"] = order.to(torch.int32)
        a.d_cell_sorted = t["cell_sorted"].data_ptr()
        a.d_order = t["order"].data_ptr()
        _lib.check(l.azp_nlist_cell_bounds(C.byref(a), H._stream()), "azp_nlist_cell_bounds")
    if cfg.get("exclusions") is not None:
        n_excl, excl = cfg["exclusions"]
        t["n_excl"] = H._dev(n_excl, np.uint32)
        t["excl"] = H._dev(np.ascontiguousarray(np.asarray(excl, dtype=np.uint32).T))  # [max][N]
        a.d_n_excl, a.d_excl, a.excl_pitch = t["n_excl"].data_ptr(), t["excl"].data_ptr(), N
    return a, t


def assert_single_pass(out, ref, cap):
    """The single-pass fill with rows of ``cap`` entries at i * cap: the full counts in d_n_neigh, every row that fits
    equal to the reference, a row that does not fit holds ``cap`` distinct entries of the reference row, *d_max_neigh
    raised to the longest row exactly when one overflowed, no other word written."""
    ref_n, ref_rows, borderline = ref
    assert borderline == 0 and out["rc_fill"] == 0
    assert np.array_equal(out["n_neigh"], ref_n) and np.all(out["n_guard"] == SENT)
    most = int(ref_n.max())
    assert out["max_neigh"][0] == (0 if cap >= most else most) and np.all(out["max_neigh"][1:] == 0)
    nl = out["nlist"]
    written = np.zeros(nl.size, dtype=bool)
    for i in range(ref_n.size):
        stored = min(int(ref_n[i]), cap)
        row = nl[i * cap: i * cap + stored]
        written[i * cap: i * cap + stored] = True
        if ref_n[i] <= cap:
            assert np.array_equal(np.sort(row), ref_rows[i]), i
        else:
            assert np.unique(row).size == cap and np.all(np.isin(row, ref_rows[i])), i
    assert np.all(nl[~written] == SENT) and np.all(nl[written] != SENT)


# id: (make(seed), cells the grid must have, MI instance)
def _liquid(L, tilt, periodic, n, rl=T.R_LIST, n_extra=0):
    return lambda s: T.tilted_liquid(L, tilt, periodic, n, s, rl=rl, n_extra=n_extra)


ROW_CASES = {
    # the system of test_gpu_nlist_rows.py::test_tilted_box_is_refused, which Cartesian cells cannot take
    "cube_xy": (lambda s: ROWS.tilted_system((0.5, 0.0, 0.0), s), (3, 4, 4), True),
    "cube_tilt3": (lambda s: ROWS.tilted_system(T.TILT3, s), (3, 4, 4), True),
    "big_tilt3": (_liquid(L_BIG, T.TILT3, (1, 1, 1), 2000), (4, 4, 5), False),
    # tilts at the limit of HOOMD's range; (3, 4, 6) cells are what r_list = 1.2 gives (w = 4.07, 5.66, 7.5), and
    # r_list = 1.5 puts 2 cells on x, whose "visit each cell once" stencil then meets the strongest tilt
    "big_strong": (_liquid(L_BIG, (-1.0, 0.7, 1.0), (1, 1, 1), 2000, rl=1.2), (3, 4, 6), True),
    "big_strong_2cells": (_liquid(L_BIG, (-1.0, 0.7, 1.0), (1, 1, 1), 2000), (2, 3, 5), True),
    "few_cells": (_liquid((4.0, 7.0, 3.2), T.TILT3, (1, 1, 1), 600), (2, 4, 2), True),
    # tilt3_open_y and tilt_xy_slab of tests/box_cases.py with 300 particles beyond the open faces (n_total > N), at
    # r_list = 1.5 (3 cells on x: MI = true) and 1.2 (>= 4 cells on the periodic axes: MI = false)
    "open_y": (_liquid((6.0, 7.0, 8.0), T.TILT3, (1, 0, 1), 1200, n_extra=300), (3, 4, 5), True),
    "open_y_staged": (_liquid((6.0, 7.0, 8.0), T.TILT3, (1, 0, 1), 1200, rl=1.2, n_extra=300), (4, 5, 6), False),
    "slab_xy": (_liquid((6.0, 7.0, 8.0), (-0.35, 0.0, 0.0), (1, 1, 0), 1200, n_extra=300), (3, 4, 5), True),
    "slab_xy_staged": (_liquid((6.0, 7.0, 8.0), (-0.35, 0.0, 0.0), (1, 1, 0), 1200, rl=1.2, n_extra=300), (4, 5, 6), False),
    # two types with a disabled pair, star polymers with up to 9 exclusions per particle
    "typed_stars": (lambda s: T.tilted_stars(L_BIG, T.TILT3, 64, 912, s, RL_TYPED), (4, 4, 5), False),
}


@functools.lru_cache(maxsize=None)
def row_case(case):
    make, dims, mi = ROW_CASES[case]
    cfg, ref = T.settled(make, 91)
    return cfg, ref, dims, mi


@pytest.mark.parametrize("binning", ["native", "sort"])
@pytest.mark.parametrize("case", list(ROW_CASES))
def test_rows_in_tilted_boxes(case, binning):
    """Count-then-fill, and the single pass with rows exactly as long as the longest row and one entry shorter."""
    cfg, ref, dims, mi = row_case(case)
    assert any(v != 0.0 for v in cfg["tilt"]) and ref[0].sum() > 10000
    a, t = bin_cells(cfg, binning=binning)
    assert tuple(a.grid.dim) == dims and a.fractional_cells == 1
    assert mi == any(cfg["periodic"][k] and dims[k] < 4 for k in range(3))  # (nlist_scan's choice of instance)
    if cfg["pos"].shape[0] > cfg["N"]:
        assert sum(int(np.count_nonzero(r >= cfg["N"])) for r in ref[1]) > 100  # listed particles beyond the open faces
    if "exclusions" in cfg:
        assert sorted(set(cfg["exclusions"][0].tolist())) == [0, 1, 4, 5, 9]
        typ = R.types_of(cfg["pos"])
        assert np.count_nonzero(typ == 1) > 100 and ref[0][typ == 0].min() > 0
    ROWS.assert_exact_rows(H.gpu_nlist_rows(a, t), ref)
    most = int(ref[0].max())
    for cap in (most, most - 1):
        assert_single_pass(H.gpu_nlist_rows(a, t, row_capacity=cap), ref, cap)


def test_untilted_box_both_cell_kinds():
    """An untilted box of (5, 4, 6) cells: fractional and Cartesian cells of the same counts give the same d_cell_of,
    the same d_order and the same list words, on both binning paths (MI = false: the FRAC = true instance against
    the orthorhombic one), rows exact against the reference."""
    dims = (5, 4, 6)
    rl = ROWS.RL3
    L = np.array(dims) * ROWS.WIDTH * rl.max()
    n = 1801

    def make(seed):
        return dict(pos=syn.pos4(T.uniform(seed, n, -0.5 * L, 0.5 * L), T.types(seed, n, 3)), L=L, periodic=(1, 1, 1), rl=rl, N=n)

    cfg, ref = T.settled(make, 33)
    outs = {}
    for binning in ("native", "sort"):
        for fractional in (0, 1):
            a, t = bin_cells(cfg, fractional=fractional, binning=binning, dims=dims)
            out = H.gpu_nlist_rows(a, t)
            ROWS.assert_exact_rows(out, ref)
            outs[binning, fractional] = (t["cell_of"].cpu().numpy(), t["order"].cpu().numpy(), out["nlist"])
    for key, got in outs.items():
        for x, y in zip(got, outs["native", 0]):
            assert np.array_equal(x, y), key
    # what gpu_cells builds (the product's own Cartesian grid) is the same binning
    a0, t0 = H.gpu_cells(cfg["pos"], (L, (0, 0, 0), (1, 1, 1)), rl, ntypes=3, N=n)
    assert tuple(a0.grid.dim) == dims and np.array_equal(t0["order"].cpu().numpy(), outs["sort", 1][1])


def test_fractional_cells_abi_refusals():
    """cell_subdivision = 2 stays refused by count / fill, a fractional_cells value other than 0 / 1 is refused by
    every entry point, azp_pair_plan_build_from_cells answers invalid_reason 6 for fractional cells."""
    cfg, ref, dims, mi = row_case("big_tilt3")
    a, t = bin_cells(cfg)
    a.cell_subdivision = 2
    out = H.gpu_nlist_rows(a, t)
    assert out["rc_count"] == ROWS.INVALID_ARGUMENT and np.all(out["n_count"] == SENT)
    a.cell_subdivision = 1
    a.fractional_cells = 2
    l = _lib.lib()
    assert l.azp_nlist_cell_assign(C.byref(a), H._stream()) == ROWS.INVALID_ARGUMENT
    assert l.azp_nlist_bin(C.byref(a), t["cursor"].data_ptr(), t["order_tmp"].data_ptr(), H._stream()) == ROWS.INVALID_ARGUMENT
    assert H.gpu_nlist_rows(a, t)["rc_count"] == ROWS.INVALID_ARGUMENT
    # the plan compiler reads Cartesian cells alone: fractional cells of an untilted box are refused like a tilted box
    flat = dict(cfg, tilt=(0.0, 0.0, 0.0))
    for tilted in (cfg, flat):
        b, tb = bin_cells(tilted, fractional=1, dims=dims)
        b.row_capacity = 160
        tb["n_neigh"] = H._dev(np.zeros(b.N, dtype=np.uint32))
        b.d_n_neigh = tb["n_neigh"].data_ptr()
        pa = _lib.PairArgs()
        pa.N, pa.n_max, pa.ntypes, pa.r_list_max = b.N, b.n_total, 1, T.R_LIST
        pa.d_pos, pa.box = b.d_pos, b.box
        rcsq = H._dev(np.array([1.3 ** 2]))
        pa.d_rcutsq = rcsq.data_ptr()
        plan = _lib.PairPlan()
        plan.build_from_cells(b, pa, H._stream())
        info = plan.info()
        assert info["valid"] == 0 and info["invalid_reason"] == 6, info


# ---------------------------------------------------------------------------
# nlist.Cell
# ---------------------------------------------------------------------------
def _tilted_box(L=L_BIG, tilt=T.TILT3):
    import azplugins_amd as azp

    return azp.Box(*L, xy=tilt[0], xz=tilt[1], yz=tilt[2])


def _api_rows(nl, n):
    nn = nl.n_neigh.cpu().numpy().astype(np.int64)
    hd = nl.head_list.cpu().numpy().astype(np.int64)
    li = nl.nlist.cpu().numpy().astype(np.int64)
    return nn, [np.sort(li[hd[i]: hd[i] + nn[i]]) for i in range(n)]


def test_api_rows_two_consumers_tilted_box():
    """nlist.Cell(buffer = 0.3) with two consumers of different r_cut matrices in the tilted (9, 8, 7.5) box: rows after
    run(0), after a move below half the buffer (kept) and after one above it (rebuilt); never in fused mode."""
    import torch

    import azplugins_amd as azp

    buffer = 0.3
    rc1 = np.array([[1.0, 0.8], [0.8, 1.2]])
    rc2 = np.array([[0.9, 1.1], [1.1, 0.7]])
    rl = np.maximum(rc1, rc2) + buffer
    assert rl.max() == 1.5
    n = 2000
    cfg, ref = T.settled(lambda s: T.tilted_liquid(L_BIG, T.TILT3, (1, 1, 1), n, s, rl=rl, ntypes=2), 101)
    snap = azp.Snapshot.from_arrays(cfg["pos"][:, :3], _tilted_box(), typeid=R.types_of(cfg["pos"]), types=("A", "B"))
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(snap)
    nl = azp.nlist.Cell(buffer=buffer)
    pots = []
    for rc in (rc1, rc2):
        pot = azp.pair.Hertz(nlist=nl, default_r_cut=1.0)
        for (ta, tb), name in (((0, 0), ("A", "A")), ((0, 1), ("A", "B")), ((1, 1), ("B", "B"))):
            pot.r_cut[name] = float(rc[ta, tb])
            pot.params[name] = dict(epsilon=1.0)
        pots.append(pot)
    sim.operations.integrator = azp.Integrator(dt=0.001, forces=pots)
    sim.operations.tuners.clear()
    sim.run(0)
    assert tuple(nl._cells.grid.dim) == (4, 4, 5) and nl._cells.fractional_cells == 1
    assert nl.fused_active is False and nl.num_builds == 1

    def assert_rows(ref):
        nn, rows = _api_rows(nl, n)
        assert ref[2] == 0 and np.array_equal(nn, ref[0])
        for i in range(n):
            assert np.array_equal(rows[i], ref[1][i]), i

    assert_rows(ref)
    nl.compute(sim.state, force=True)  # the fill alone, rows of the learned capacity
    assert nl.num_builds == 2 and nl.size == n * nl._row_capacity
    assert_rows(ref)

    def displacement(amplitude, seed):
        tag = np.arange(n, dtype=np.uint64)
        v = np.stack([syn.normal(seed, tag, c) for c in range(3)], axis=1)
        return v * (amplitude * (0.5 + 0.5 * syn.u01(seed + 1, tag, 0)) / np.linalg.norm(v, axis=1))[:, None]

    def move(amplitude, seed):
        sim.state.pos[:, :3] += torch.from_numpy(displacement(amplitude, seed)).to(sim.state.pos.device)
        sim.state.position_generation += 1
        nl.compute(sim.state)

    move(0.45 * buffer, 7)
    assert nl.num_builds == 2  # nobody moved farther than half the buffer: the rows stand
    assert_rows(ref)
    for seed in range(8, 18):  # (reseeded until the moved configuration has no borderline pair)
        pos = sim.state.pos.cpu().numpy()
        pos[:, :3] += displacement(0.9 * buffer, seed)
        ref2 = R.all_pairs_rows(pos, cfg["L"], T.TILT3, (1, 1, 1), rl, n)
        if ref2[2] == 0:
            break
    move(0.9 * buffer, seed)
    assert np.array_equal(sim.state.pos.cpu().numpy(), pos)
    assert np.linalg.norm(pos[:, :3] - cfg["pos"][:, :3], axis=1).max() > 0.5 * buffer
    assert nl.num_builds == 3 and nl.fused_active is False  # rebuilt (some particles now a little outside the box)
    assert_rows(ref2)


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------
def _fractional_lattice(nx, ny, nz, L, tilt, jitter, seed):
    """nx x ny x nz sites evenly spaced along the lattice vectors, jittered: no overlapping pair."""
    ix, iy, iz = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    f = (np.stack([ix.ravel(), iy.ravel(), iz.ravel()], axis=1) + 0.5) / np.array([nx, ny, nz]) - 0.5
    n = f.shape[0]
    tag = np.arange(n, dtype=np.uint64)
    xyz = f @ T.lattice(L, tilt) + np.stack([(2.0 * syn.u01(seed, tag, c) - 1.0) * jitter for c in range(3)], axis=1)
    return T.wrap_tilted(xyz, L, tilt)


def _oracle_list(pos, L, tilt, r_list):
    n_neigh, rows, _ = R.all_pairs_rows(pos, L, tilt, (1, 1, 1), r_list, pos.shape[0])
    head = (np.cumsum(n_neigh) - n_neigh).astype(np.uint64)
    return n_neigh.astype(np.uint32), head, np.concatenate(rows).astype(np.uint32)


def _assert_close(got, ref, what):
    scale = np.abs(ref).max()
    err = np.abs(got - ref).max()
    print("%s: max deviation %.3e, largest component %.3e" % (what, err, scale))
    assert np.all(np.isfinite(got)) and err <= TOL * scale, "%s: %g > %g" % (what, err, TOL * scale)


def _assert_inside(pos, L, tilt):
    f = box_ref.fractional(pos[:, :3], L, tilt)
    ulp = np.spacing(0.5)
    assert f.min() >= -0.5 - 4 * ulp and f.max() < 0.5 + 4 * ulp


def test_md_run_in_a_tilted_box(oracle):
    """PerturbedLennardJones, one consumer, in the tilted (9, 8, 7.5) box at rho* = 0.8 (sigma = 0.6, N = 2028): the
    tile kernel runs from the plan compiled from the list's rows (no fused mode). After thermalizing and run(60) with
    ConstantVolume the list was rebuilt at least three times; the forces equal the oracle's on an all-pairs list of the
    final positions, which lie inside the box."""
    import azplugins_amd as azp

    sigma, r_cut, buffer, dt = 0.6, 1.3, 0.1, 0.002
    xyz = _fractional_lattice(13, 12, 13, L_BIG, T.TILT3, 0.02, 5)
    n = xyz.shape[0]
    assert n == 2028 and abs(n * sigma ** 3 / np.prod(L_BIG) - 0.8) < 0.02
    sim = azp.Simulation(device="cuda:0", seed=3)
    sim.create_state_from_snapshot(azp.Snapshot.from_arrays(xyz, _tilted_box()))
    nl = azp.nlist.Cell(buffer=buffer)
    plj = azp.pair.PerturbedLennardJones(nlist=nl, default_r_cut=r_cut, mode="shift")
    prm = dict(epsilon=1.0, sigma=sigma, attraction_scale_factor=0.5)
    plj.params[("A", "A")] = prm
    sim.operations.integrator = azp.Integrator(dt=dt, forces=[plj], methods=[azp.ConstantVolume()])
    sim.thermalize_particle_momenta(kT=1.0, seed=11)
    sim.run(60)
    assert nl.num_builds >= 3 and nl.fused_active is False and nl._cells.fractional_cells == 1
    info = plj.plan_info
    assert info["valid"] == 1 and info["from_cells"] == 0  # the tile kernel, its plan compiled from the rows
    plj.compute(sim.timestep)
    pos = sim.state.pos[:n].cpu().numpy()
    _assert_inside(pos, L_BIG, T.TILT3)
    assert np.abs(pos[:, :3] - xyz).max() > buffer  # (the particles did move)
    box = oracle.make_box(L_BIG, tilt=T.TILT3)
    f_ref = oracle.pair_forces("PerturbedLennardJones", pos, box, _oracle_list(pos, L_BIG, T.TILT3, r_cut + buffer),
                               oracle.pack_pair_params("PerturbedLennardJones", prm), r_cut, mode="shift")
    _assert_close(plj.force_tensor[:n].cpu().numpy(), f_ref, "plj after 60 steps")


def test_dpd_run_in_a_tilted_box(oracle):
    """The DPD thermostat in the same box at rho = 3.7: forces against the oracle with the same seed and timestep
    after run(0) and run(10), as tests/test_gpu_parity.py::test_dpd_thermostat_parity compares them."""
    import azplugins_amd as azp

    n, r_cut, buffer, dt, kT, seed = 2000, 1.0, 0.3, 0.01, 1.0, 7
    xyz = T.uniform(21, n, -0.5, 0.5) @ T.lattice(L_BIG, T.TILT3)
    tag = np.arange(n, dtype=np.uint64)
    vel = np.stack([syn.normal(22, tag, c) for c in range(3)], axis=1)
    prm = dict(A=25.0, gamma=4.5, s=0.5)
    sim = azp.Simulation(device="cuda:0", seed=seed)
    sim.create_state_from_snapshot(azp.Snapshot.from_arrays(xyz, _tilted_box(), velocity=vel))
    nl = azp.nlist.Cell(buffer=buffer)
    pot = azp.pair.DPDGeneralWeight(nlist=nl, kT=kT, default_r_cut=r_cut)
    pot.params[("A", "A")] = prm
    sim.operations.integrator = azp.Integrator(dt=dt, forces=[pot], methods=[azp.ConstantVolume()])
    sim.operations.tuners.clear()
    box = oracle.make_box(L_BIG, tilt=T.TILT3)
    for steps in (0, 10):
        sim.run(steps)
        pot.compute(sim.timestep)  # (the run's last evaluation saw the half-kicked velocities)
        assert nl.fused_active is False and nl._cells.fractional_cells == 1
        st = sim.state
        pos = st.pos[:n].cpu().numpy()
        _assert_inside(pos, L_BIG, T.TILT3)
        f_ref = oracle.dpd_forces(pos, st.vel[:n].cpu().numpy(), st.tag[:n].cpu().numpy().view(np.uint32), box,
                                  _oracle_list(pos, L_BIG, T.TILT3, r_cut + buffer),
                                  oracle.pack_pair_params("DPDGeneralWeight", prm), r_cut, kT=kT, dt=dt, seed=seed, timestep=sim.timestep)
        _assert_close(np.c_[pot.forces, pot.energies], f_ref, "dpd after %d steps" % steps)


def test_same_lattice_two_boxes():
    """Lx = Ly with xy = 0 and with xy = 1 are the same lattice (b' = b + a): the same particles, re-wrapped into the
    tilted box, get the same forces and energies per tag to 1e-12 of the largest, and rows of the same lengths."""
    import azplugins_amd as azp

    L, sigma, r_cut, buffer = (9.0, 9.0, 7.5), 0.6, 1.3, 0.2
    rl = r_cut + buffer

    def make(seed):
        xyz = _fractional_lattice(13, 13, 12, L, (0.0, 0.0, 0.0), 0.05, seed)
        return dict(pos=syn.pos4(xyz), L=np.array(L), periodic=(1, 1, 1), rl=np.array([[rl]]), N=xyz.shape[0])

    cfg, ref = T.settled(make, 41)
    n = cfg["N"]
    sheared = T.wrap_tilted(cfg["pos"][:, :3], L, (1.0, 0.0, 0.0))
    moved = np.abs(sheared - cfg["pos"][:, :3]).max(axis=1) > 1.0
    assert 0.15 * n < np.count_nonzero(moved) < 0.35 * n  # |x - y| > L / 2: a quarter of the particles sit in another image
    got = []
    for xyz, tilt, dims in ((cfg["pos"][:, :3], (0.0, 0.0, 0.0), (6, 6, 5)), (sheared, (1.0, 0.0, 0.0), (4, 6, 5))):
        sim = azp.Simulation(device="cuda:0", seed=1)
        sim.create_state_from_snapshot(azp.Snapshot.from_arrays(xyz, _tilted_box(L, tilt)))
        nl = azp.nlist.Cell(buffer=buffer)
        nl.fused = False
        plj = azp.pair.PerturbedLennardJones(nlist=nl, default_r_cut=r_cut, mode="shift")
        plj.params[("A", "A")] = dict(epsilon=1.0, sigma=sigma, attraction_scale_factor=0.5)
        sim.operations.integrator = azp.Integrator(dt=0.001, forces=[plj])
        sim.operations.tuners.clear()
        sim.run(0)
        assert tuple(nl._cells.grid.dim) == dims and nl._cells.fractional_cells == (1 if tilt[0] else 0)
        got.append((np.c_[plj.forces, plj.energies], nl.n_neigh.cpu().numpy().astype(np.int64)))
    (f0, n0), (f1, n1) = got
    assert np.array_equal(n0, ref[0]) and np.array_equal(n1, n0)
    assert np.abs(f0[:, :3]).max() > 1.0
    for cols in (slice(0, 3), slice(3, 4)):
        assert np.abs(f1[:, cols] - f0[:, cols]).max() <= 1e-12 * np.abs(f0[:, cols]).max()


def test_attach_domain_refuses_a_tilted_box():
    import azplugins_amd as azp

    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(azp.Snapshot.from_arrays(np.zeros((4, 3)), _tilted_box()))
    with pytest.raises(_lib.AzpError, match=r"attach_domain: Box\(Lx=9, Ly=8, Lz=7.5, xy=0.5, xz=0.3, yz=-0.4\) is tilted"):
        sim.attach_domain(object())
