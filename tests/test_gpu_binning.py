"""azp_nlist_bin (counting sort of the particles by cell, csrc/cell_bin.hpp, + per-cell sort, csrc/nlist.hip) on every one of its paths,
through the C ABI against numpy's stable sort; the row builder on grids of many cells against the all-pairs reference
with both binnings; nlist.Cell._bin on its three branches through the API.

Which path a (grid, n_total) selects (binning_cases.paths_of, the rule of azp_nlist_bin):
  scan   nblk = ceil(ncell / 4096); three kernels (local scans, the scan of the block totals in d_order_tmp, the add)
         when nblk > 8 and nblk + 1 <= n_total, else one workgroup with nblk trips and the carry in a register;
  sort   one thread per cell when n_total <= 6 ncell (registers up to 8 particles, memory above), else one wave per
         cell (trips of 64).
The test ids name the expected path: scan1xT = one workgroup, T trips; scan3xB = three kernels, B blocks.
"""

import ctypes as C

import numpy as np
import pytest

import binning_cases as B
import helpers as H
from azplugins_amd import _lib
from azplugins_amd import synthetic as syn
from test_gpu_nlist_rows import RL3, assert_exact_rows, liquid
from test_gpu_parity import assert_close

pytestmark = pytest.mark.gpu

SENT = H.NLIST_SENTINEL
GUARD = 64
INVALID_ARGUMENT = -1  # AZP_ERROR_INVALID_ARGUMENT (include/azp.h)


# ---------------------------------------------------------------------------
# A1: azp_nlist_bin through the C ABI
# ---------------------------------------------------------------------------
def bin_args(xyz, dims, L, periodic=(1, 1, 1)):
    """azp_nlist_args for binning alone (grid filled by hand; no r_list) and the five sentinel-filled buffers, each
    with GUARD extra words."""
    import torch

    n = xyz.shape[0]
    ncell = int(np.prod(dims))
    a = _lib.NlistArgs()
    a.N, a.n_total, a.ntypes = n, n, 1
    t = dict(pos=H._dev(syn.pos4(xyz) if n else np.zeros((0, 4))))
    a.d_pos = t["pos"].data_ptr()
    a.box = _lib.make_box(L, periodic=periodic)
    for k in range(3):
        a.grid.dim[k] = int(dims[k])
        a.grid.width[k] = float(L[k]) / dims[k] if dims[k] else 1.0
        a.grid.lo[k] = -0.5 * float(L[k])
        a.grid.periodic[k] = int(periodic[k])
    for name, size in (("order", n), ("cell_start", ncell + 1), ("cell_of", n), ("cursor", ncell), ("order_tmp", n), ("assigned", n)):
        t[name] = torch.full((size + GUARD,), SENT, dtype=torch.int32, device="cuda:0")
    a.d_order, a.d_cell_start, a.d_cell_of = t["order"].data_ptr(), t["cell_start"].data_ptr(), t["cell_of"].data_ptr()
    return a, t


def host(x):
    return x.cpu().numpy().view(np.uint32).astype(np.int64)


def call_bin(a, t, cursor=True, order_tmp=True):
    import torch

    rc = _lib.lib().azp_nlist_bin(C.byref(a), t["cursor"].data_ptr() if cursor else None,
                                  t["order_tmp"].data_ptr() if order_tmp else None, H._stream())
    torch.cuda.synchronize()
    return rc


def assigned_cells(a, t):
    """What azp_nlist_cell_assign writes for the same positions (into a buffer of its own)."""
    import torch

    keep = a.d_cell_of
    a.d_cell_of = t["assigned"].data_ptr()
    _lib.check(_lib.lib().azp_nlist_cell_assign(C.byref(a), H._stream()), "azp_nlist_cell_assign")
    torch.cuda.synchronize()
    a.d_cell_of = keep
    return host(t["assigned"])


def assert_binned(a, t, n, ncell, want_cell=None):
    """order / cell_start / cell_of against numpy's stable sort of the cell ids; guard words of all five buffers
    intact (nothing is asserted about what the scratch buffers hold); a second call gives the identical order."""
    order, start, cell_of = host(t["order"]), host(t["cell_start"]), host(t["cell_of"])
    for name, size in (("order", n), ("cell_start", ncell + 1), ("cell_of", n), ("cursor", ncell), ("order_tmp", n)):
        assert np.all(host(t[name])[size:] == SENT), "guard words of %s" % name
    cell_of = cell_of[:n]
    assert cell_of.size == 0 or cell_of.max() < ncell
    assert np.array_equal(cell_of, assigned_cells(a, t)[:n])
    if want_cell is not None:
        assert np.array_equal(cell_of, want_cell)
    ref_order = np.argsort(cell_of, kind="stable")
    ref_start = np.searchsorted(cell_of[ref_order], np.arange(ncell + 1), side="left")
    bad = np.flatnonzero(start[: ncell + 1] != ref_start)
    assert bad.size == 0, "cell_start: first bad cell %d of %d (%d in all)" % (bad[0], ncell, bad.size)
    assert np.array_equal(order[:n], ref_order)
    t["order"].fill_(SENT)
    assert call_bin(a, t) == 0
    assert np.array_equal(host(t["order"])[:n], ref_order) and np.all(host(t["order"])[n:] == SENT)
    return cell_of


@pytest.mark.parametrize("memory_order", ["shuffled", "by_cell"])
@pytest.mark.parametrize("case", B.TABLE, ids=B.case_id)
def test_bin_is_the_stable_sort_on_every_path(case, memory_order):
    """shuffled: the lanes of a wave hold distinct keys; by_cell: all 64 lanes of most waves share a key (one atomic
    per wave in wave_aggregated_add)."""
    dims, n = case
    sys_ = B.occupancy_case(dims, n)
    ncell = int(np.prod(dims))
    counts = sys_["counts"]
    if n >= 100:  # (the occupancies the sort kernel's branches need; test_binning_ref.py has the rest)
        assert set(B.SMALL_SET if B.paths_of(dims, n)[1] == "small" else B.WAVE_SET) <= set(counts.tolist())
        assert np.all(counts[B.marked_cells(ncell)] > 0)
    perm = B.shuffled(n) if memory_order == "shuffled" else np.arange(n)
    if memory_order == "by_cell":
        assert np.all(np.diff(sys_["cell"]) >= 0)
    a, t = bin_args(sys_["xyz"][perm], dims, sys_["L"])
    assert call_bin(a, t) == 0
    cell_of = assert_binned(a, t, n, ncell, want_cell=sys_["cell"][perm])
    assert np.array_equal(np.bincount(cell_of, minlength=ncell), counts)


@pytest.mark.parametrize("dims", [(3, 3, 3), (41, 41, 41)], ids=["wave", "small"])
def test_bin_all_particles_in_one_cell(dims):
    """300 particles in one cell: five trips of the wave-per-cell sort on 27 cells, the memory path of the
    thread-per-cell sort on 41^3."""
    n = 300
    ncell = int(np.prod(dims))
    assert B.paths_of(dims, n)[1] == ("wave" if ncell == 27 else "small")
    L = np.asarray(dims) * B.CELL_WIDTH
    home = np.array([d // 2 for d in dims])
    u = np.stack([syn.u01(5, np.arange(n, dtype=np.uint64), c) for c in range(3)], axis=1)
    xyz = -0.5 * L + (home + 0.1 + 0.8 * u) * B.CELL_WIDTH
    a, t = bin_args(xyz, dims, L)
    assert call_bin(a, t) == 0
    cell_of = assert_binned(a, t, n, ncell)
    assert np.all(cell_of == (home[2] * dims[1] + home[1]) * dims[0] + home[0])
    assert np.array_equal(host(t["order"])[:n], np.arange(n))


def test_bin_wraps_and_clamps():
    """(1, 0, 1)-periodic grid: particles several box lengths outside a periodic axis are wrapped, ghosts beyond a
    non-periodic face are clamped into the outermost cell; particles exactly on +-L/2 and 1e-12 inside land in one of
    the two cells at that face."""
    dims, periodic = (5, 4, 6), (1, 0, 1)
    n = 2011
    xyz, L = liquid(dims, RL3, n, 17)
    w = L / np.asarray(dims)
    q = np.arange(n)
    far = (q >= 12) & (q % 7 == 0)       # several box lengths outside x or z
    shift = ((q // 7) % 7 - 3)            # -3 .. 3 box lengths
    xyz[far & (q % 2 == 0), 0] += (shift * L[0])[far & (q % 2 == 0)]
    xyz[far & (q % 2 == 1), 2] += (shift * L[2])[far & (q % 2 == 1)]
    ghost = (q >= 12) & (q % 7 == 1)     # up to 1.5 cells beyond a y face
    depth = 1.5 * w[1] * syn.u01(18, q.astype(np.uint64), 0)
    xyz[ghost, 1] = np.where(q % 2 == 0, 0.5 * L[1] + depth, -0.5 * L[1] - depth)[ghost]
    assert np.count_nonzero(np.abs(xyz[:, 0]) > 1.5 * L[0]) > 20 and np.count_nonzero(np.abs(xyz[:, 2]) > 1.5 * L[2]) > 20
    assert np.count_nonzero(xyz[:, 1] > 0.5 * L[1]) > 50 and np.count_nonzero(xyz[:, 1] < -0.5 * L[1]) > 50
    a, t = bin_args(xyz, dims, L, periodic)
    assert call_bin(a, t) == 0
    ncell = int(np.prod(dims))
    cell_of = assert_binned(a, t, n, ncell)
    frac = (xyz + 0.5 * L) / w
    clear = np.all(np.abs(frac - np.rint(frac)) > 1e-9, axis=1)
    assert np.all(clear[12:]) and not np.any(clear[:12])
    want = B.cell_rule(xyz, -0.5 * L, w, dims, periodic)
    assert np.array_equal(cell_of[clear], want[clear])
    for p in range(12):  # planted on the face of axis p // 4: the cell on either side of it
        e = np.zeros(3)
        e[p // 4] = 1e-6 * w[p // 4]
        either = {int(B.cell_rule(xyz[p: p + 1] + s * e, -0.5 * L, w, dims, periodic)[0]) for s in (-1.0, 1.0)}
        assert int(cell_of[p]) in either, p


def test_bin_keeps_nan_and_huge_coordinates_out_of_the_conversion():
    """(1, 0, 1)-periodic grid, a dozen ordinary particles (0.3 of a width off their cell's centre at most) and six
    that no cell rule covers: NaN, +1e300 and -1e300, each once on a periodic axis (x) and once on the clamped one (y).
    cell_coord bounds the coordinate before it converts it to int, so every particle gets SOME cell of the grid, the
    same one from azp_nlist_bin and azp_nlist_cell_assign, and the binning of all 18 is consistent; the ordinary ones
    have the reference's cells."""
    dims, periodic = (5, 4, 6), (1, 0, 1)
    ncell = int(np.prod(dims))
    n_ok = 12
    cell = (np.arange(n_ok, dtype=np.int64) * 23 + 5) % ncell
    ijk = np.stack([cell % dims[0], (cell // dims[0]) % dims[1], cell // (dims[0] * dims[1])], axis=1)
    jitter = np.stack([0.6 * (syn.u01(31, np.arange(n_ok, dtype=np.uint64), c) - 0.5) for c in range(3)], axis=1)
    L = np.asarray(dims) * B.CELL_WIDTH
    ok = -0.5 * L + (ijk + 0.5 + jitter) * B.CELL_WIDTH
    assert np.array_equal(B.cell_rule(ok, -0.5 * L, B.CELL_WIDTH, dims, periodic), cell)
    bad = np.tile(ok[:1], (6, 1))
    for k, v in enumerate((np.nan, 1e300, -1e300)):
        bad[2 * k, 0] = v      # periodic axis
        bad[2 * k + 1, 1] = v  # clamped axis
    xyz = np.concatenate([ok[:6], bad, ok[6:]])
    is_ok = np.r_[np.ones(6, bool), np.zeros(6, bool), np.ones(6, bool)]
    n = xyz.shape[0]
    a, t = bin_args(xyz, dims, L, periodic)
    assert call_bin(a, t) == 0
    cell_of, order, start = host(t["cell_of"])[:n], host(t["order"])[:n], host(t["cell_start"])[: ncell + 1]
    assert np.all(cell_of < ncell)
    assert np.array_equal(assigned_cells(a, t)[:n], cell_of)
    assert np.array_equal(np.sort(order), np.arange(n))
    assert np.array_equal(start, np.r_[0, np.cumsum(np.bincount(cell_of, minlength=ncell))])
    assert np.array_equal(cell_of[is_ok], cell)
    assert_binned(a, t, n, ncell)


def test_bin_edges():
    """n_total = 0: success, cell_start all zero. Null scratch pointers or a zero grid dimension: refused, nothing
    written."""
    dims = (41, 41, 41)
    ncell = 41 ** 3
    L = np.asarray(dims) * B.CELL_WIDTH
    a, t = bin_args(np.zeros((0, 3)), dims, L)
    assert call_bin(a, t) == 0
    start = host(t["cell_start"])
    assert np.all(start[: ncell + 1] == 0) and np.all(start[ncell + 1:] == SENT)
    assert np.all(host(t["order"]) == SENT) and np.all(host(t["cell_of"]) == SENT) and np.all(host(t["cursor"])[ncell:] == SENT)

    sys_ = B.occupancy_case((16, 16, 16), 24576)

    def untouched(t):
        return all(np.all(host(t[k]) == SENT) for k in ("order", "cell_start", "cell_of", "cursor", "order_tmp"))

    a, t = bin_args(sys_["xyz"], sys_["dims"], sys_["L"])
    assert call_bin(a, t, cursor=False) == INVALID_ARGUMENT and untouched(t)
    assert call_bin(a, t, order_tmp=False) == INVALID_ARGUMENT and untouched(t)
    for k in range(3):
        a, t = bin_args(sys_["xyz"], sys_["dims"], sys_["L"])
        a.grid.dim[k] = 0
        assert call_bin(a, t) == INVALID_ARGUMENT and untouched(t)


# ---------------------------------------------------------------------------
# A2: rows on grids of many cells, both binnings
# ---------------------------------------------------------------------------
RL3_KEY = tuple(tuple(float(x) for x in row) for row in RL3)


@pytest.mark.parametrize("dims", [(33, 33, 31), (41, 41, 41)], ids=lambda d: "x".join(str(x) for x in d))
def test_rows_on_grids_of_many_cells(dims):
    """(33, 33, 31) = 33,759 cells: the three-kernel scan, occupied cells above 2^15. 41^3 = 68,921 cells: above the
    2^16 cells at which nlist.Cell switches to azp_nlist_bin. A clumped system (rows of 8 on average although most
    cells are empty), every row against the all-pairs reference with the framework's sort and with azp_nlist_bin; both
    binnings give the same order and bounds."""
    cfg, ref = B.clumped_system(dims, RL3_KEY)
    facts = B.clumped_facts(cfg, ref, dims)
    ncell = int(np.prod(dims))
    assert facts["borderline"] == 0 and facts["mean_row"] >= 8 and all(c > 0 for c in facts["crossing"])
    assert facts["occupied_above"][32768] > 0 and (ncell <= 65536 or facts["occupied_above"][65536] > 0)
    assert B.paths_of(dims, cfg["N"]) == ("scan3x%d" % ((ncell + 4095) // 4096), "small")
    binned = {}
    for binning in ("sort", "native"):
        a, t = H.gpu_cells(cfg["pos"], (cfg["L"], (0, 0, 0), cfg["periodic"]), RL3, ntypes=3, N=cfg["N"], dims=dims, binning=binning)
        assert tuple(a.grid.dim) == dims
        assert_exact_rows(H.gpu_nlist_rows(a, t), ref)
        binned[binning] = (t["order"].cpu().numpy()[: cfg["N"]], t["cell_start"].cpu().numpy()[: ncell + 1], t["cell_of"].cpu().numpy())
    for x, y, what in zip(binned["sort"], binned["native"], ("order", "cell_start", "cell_of")):
        assert np.array_equal(x, y), what
    assert binned["native"][2].max() >= (65536 if ncell > 65536 else 32768)


# ---------------------------------------------------------------------------
# A3: nlist.Cell._bin through the API
# ---------------------------------------------------------------------------
R_CUT, BUFFER = 1.0, 0.07
API_WIDTH = 1.0001  # cells this much wider than the list radius: floor(L / r_list) is the intended grid


@pytest.mark.parametrize("dims,native,path", [((40, 40, 40), None, "sort16"), ((41, 41, 41), None, "native"),
                                              ((41, 41, 41), False, "sort32"), ((40, 40, 40), True, "native")],
                         ids=["40-default-sort16", "41-default-native", "41-off-sort32", "40-on-native"])
def test_cell_list_binning_branches(oracle, dims, native, path):
    """The clumped system behind azp.Simulation and azp.nlist.Cell with a Hertz potential (finite at contact: clump
    members overlap). 40^3 = 64,000 cells take the framework sort on 16-bit keys (cells >= 2^15: positive keys), 41^3
    azp_nlist_bin by default and the 32-bit framework sort when it is switched off. Rows (fused = False) against the
    all-pairs reference; forces and energies (fused, shuffled memory order, then after 20 steps with a particle sort
    and rebuilds) against the oracle."""
    import azplugins_amd as azp

    r_list = R_CUT + BUFFER
    cfg, ref = B.clumped_system(dims, ((r_list,),), width=API_WIDTH)
    facts = B.clumped_facts(cfg, ref, dims)
    assert facts["borderline"] == 0 and facts["mean_row"] >= 8 and facts["occupied_above"][32768] > 0
    n, L = cfg["N"], cfg["L"]
    box = oracle.make_box(L)
    params = oracle.pack_pair_params("Hertz", dict(epsilon=3.0))

    def simulation(fused):
        sim = azp.Simulation(device="cuda:0", seed=1)
        sim.create_state_from_snapshot(azp.Snapshot.from_arrays(cfg["pos"][:, :3], L))
        nl = azp.nlist.Cell(buffer=BUFFER)
        nl.native_binning = native  # (on the instance)
        if not fused:
            nl.fused = False
        pot = azp.pair.Hertz(nlist=nl, default_r_cut=R_CUT)
        pot.params[("A", "A")] = dict(epsilon=3.0)
        sim.operations.integrator = azp.Integrator(dt=0.005, forces=[pot], methods=[azp.ConstantVolume()])
        return sim, nl, pot

    def assert_forces(sim, pot):
        pos = syn.pos4(sim.state.pos[: sim.state.N, :3].cpu().numpy())
        onl = oracle.build_nlist(pos, box, R_CUT)
        assert_close(np.c_[pot.forces, pot.energies], oracle.pair_forces("Hertz", pos, box, onl, params, R_CUT, nthreads=8))

    # rows
    sim, nl, pot = simulation(fused=False)
    assert nl.binning_path is None
    sim.run(0)
    assert tuple(nl._cells.grid.dim) == dims and nl.binning_path == path
    nn = nl.n_neigh.cpu().numpy().astype(np.int64)
    hd = nl.head_list.cpu().numpy().astype(np.int64)
    li = nl.nlist.cpu().numpy().astype(np.int64)
    assert np.array_equal(nn, ref[0])
    for i in range(n):
        assert np.array_equal(np.sort(li[hd[i]: hd[i] + nn[i]]), ref[1][i]), i
    assert_forces(sim, pot)

    # forces, fused, shuffled memory order (the plan compile from the cells may refuse: the fall-back is exact too)
    sim, nl, pot = simulation(fused=True)
    sim.run(0)
    assert tuple(nl._cells.grid.dim) == dims and nl.binning_path == path
    info0 = dict(pot.plan_info or {})
    assert_forces(sim, pot)
    # 20 steps of a thermalised state; the default particle sorter with its period shortened from 200 to 10 steps, so
    # that a sort falls into the run
    sim.thermalize_particle_momenta(1.0, seed=3)
    sorter = sim.operations.tuners[0]
    sorter.trigger_period = 10
    builds = nl.num_builds
    sim.run(20)
    assert sorter.num_sorts >= 1 and nl.num_builds >= builds + 2
    assert nl.binning_path == path
    assert_forces(sim, pot)
    keys = ("valid", "from_cells", "invalid_reason")
    print("[binning] %s native_binning=%s: binning_path=%s builds=%d sorts=%d plan_info at run(0) %s, after run(20) %s"
          % ("x".join(str(d) for d in dims), native, nl.binning_path, nl.num_builds, sorter.num_sorts,
             {k: info0.get(k) for k in keys}, {k: (pot.plan_info or {}).get(k) for k in keys}))
