"""Neighbor-list exclusions beyond bonds (``nlist.Cell(exclusions=("bond", "1-3", "1-4"))``) on the GPU: PerturbedLJ
forces and energies through ``Simulation`` against the oracle's pair loop over a list built with the reference
exclusion table (``exclusion_ref``: adjacency sets and explicit walks), on every path that reads the table -- the fused
plan from cells, the fill of the HOOMD-format list, the list-based plan of a tilted box -- and after a particle sort.
The bound is the project's FP64 parity bound (tests/test_gpu_parity.py): 1e-10 of the largest component.

The system: 64 zig-zag chains of 8 and four 7-arm stars in a cubic box of 2.2 x (2 r_list). An interior chain bead has
2 + 2 + 2 = 6 exclusions and a star arm 1 + 6 = 7: past the four that the plan compiler keeps in registers."""

import functools

import numpy as np
import pytest

import azplugins_amd as azp
import box_ref
import exclusion_ref as xref
import nlist_ref
from azplugins_amd import synthetic as syn

pytestmark = pytest.mark.gpu

TOL = 1e-10
R_CUT, BUFFER = 3.0, 0.4
R_LIST = R_CUT + BUFFER
L = 2.2 * (2.0 * R_LIST)   # 14.96
KINDS = ("bond", "1-3", "1-4")
PARAMS = dict(epsilon=1.0, sigma=1.0, attraction_scale_factor=0.5)
TILT = (0.2, -0.1, 0.15)
N_CHAINS, CHAIN, N_STARS, ARMS = 64, 8, 4, 7
N = N_CHAINS * CHAIN + N_STARS * (ARMS + 1)


@functools.lru_cache(maxsize=None)
def _system():
    """(xyz, bonds): chains zig-zag along x (bond length 1, 1-3 distance 1.6, 1-4 distance 2.5 before the jitter), two
    to a row, rows 1.8 apart in y on four z layers; the stars on two layers of their own."""
    xyz = []
    for c in range(N_CHAINS):
        ix, iy, iz = c % 2, (c // 2) % 8, c // 16
        x0, y0, z0 = -7.2 + 7.5 * ix, -6.6 + 1.8 * iy, -6.5 + 1.5 * iz
        for k in range(CHAIN):
            xyz.append((x0 + 0.8 * k, y0 + (0.3 if k % 2 else -0.3), z0))
    arms = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (3 ** -0.5, 3 ** -0.5, 3 ** -0.5)])
    for s in range(N_STARS):
        centre = np.array([-5.0 + 3.4 * s, 2.0 * (s % 2) - 1.0, 2.5 + 2.6 * (s % 2)])
        xyz.append(tuple(centre))
        xyz += [tuple(centre + a) for a in arms]
    xyz = np.array(xyz)
    tag = np.arange(N, dtype=np.uint64)
    xyz += 0.1 * (np.stack([syn.u01(77, tag, c) for c in range(3)], axis=1) - 0.5)
    bonds = np.concatenate([xref.chain_bonds(N_CHAINS, CHAIN), xref.star_bonds(N_STARS, ARMS, first=N_CHAINS * CHAIN)])
    assert xyz.shape == (N, 3) and np.abs(xyz).max() < 0.5 * L
    return xyz, bonds


@functools.lru_cache(maxsize=None)
def _tables():
    _, bonds = _system()
    return {kinds: xref.table(xref.pair_set(kinds, bonds=bonds), N) for kinds in (KINDS, ("bond",))}


def _min_image_distance(xyz, i, j, tilt):
    x, y, z = nlist_ref.min_image(xyz[i] - xyz[j], (L, L, L), tilt, (1, 1, 1))
    return np.sqrt(x * x + y * y + z * z)


def test_system_is_what_the_tests_need():
    """On the CPU: every excluded pair lies inside r_list (so each one would be in the list without its exclusion), most
    of them inside r_cut (they carry force), and the rows are longer than the four entries the plan compiler keeps in
    registers."""
    xyz, bonds = _system()
    sets = xref.pair_sets(bonds=bonds)
    for tilt in ((0.0, 0.0, 0.0), TILT):
        pos = box_ref.wrap(xyz, None, (L, L, L), tilt)[0]
        for name in KINDS:
            ij = np.array(sorted(sets[name]))
            r = _min_image_distance(pos, ij[:, 0], ij[:, 1], tilt)
            print("%s: %d pairs, r in [%.3f, %.3f]" % (name, len(ij), r.min(), r.max()))
            assert r.max() < R_LIST
        ij = np.array(sorted(sets["1-4"]))
        assert np.count_nonzero(_min_image_distance(pos, ij[:, 0], ij[:, 1], tilt) < R_CUT) > 0.9 * len(ij)
    n_excl, excl = _tables()[KINDS]
    assert n_excl[3] == 6 and n_excl[N_CHAINS * CHAIN + 1] == 7 and n_excl[N_CHAINS * CHAIN] == 7 and excl.shape[1] == 7
    assert np.count_nonzero(n_excl > 4) > N // 2


@functools.lru_cache(maxsize=None)
def _reference(kinds, tilted):
    """The oracle's pair forces (N, 4) over a list with the reference exclusions: its own cell list in the cubic box,
    the all-pairs rows of nlist_ref in the tilted one (the oracle's list builder takes no tilt)."""
    import oracle

    xyz, _ = _system()
    tilt = TILT if tilted else (0.0, 0.0, 0.0)
    pos = syn.pos4(box_ref.wrap(xyz, None, (L, L, L), tilt)[0])
    box = oracle.make_box(L, tilt=tilt)
    table = _tables()[kinds]
    if tilted:
        n_neigh, rows, _ = nlist_ref.all_pairs_rows(pos, (L, L, L), tilt, (1, 1, 1), R_LIST, N, exclusions=table)
        onl = (n_neigh.astype(np.uint32), (np.cumsum(n_neigh) - n_neigh).astype(np.uint64), np.concatenate(rows).astype(np.uint32))
    else:
        onl = oracle.build_nlist(pos, box, R_LIST, exclusions=table)
    f = oracle.pair_forces("PerturbedLennardJones", pos, box, onl, oracle.pack_pair_params("PerturbedLennardJones", PARAMS),
                           R_CUT, mode="shift")
    f.setflags(write=False)
    return f


def _sim(exclusions, tilted=False, fused=True):
    xyz, bonds = _system()
    tilt = TILT if tilted else (0.0, 0.0, 0.0)
    snap = azp.Snapshot.from_arrays(box_ref.wrap(xyz, None, (L, L, L), tilt)[0], azp.Box(L, L, L, *tilt), bonds=bonds)
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(snap)
    sim.operations.tuners.clear()
    nl = azp.nlist.Cell(buffer=BUFFER, exclusions=exclusions)
    nl.fused = fused
    plj = azp.pair.PerturbedLennardJones(nlist=nl, default_r_cut=R_CUT, mode="shift")
    plj.params[("A", "A")] = PARAMS
    sim.operations.integrator = azp.Integrator(dt=0.001, forces=[plj])
    return sim, nl, plj


def _close(got, want, what):
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    print("%s: max deviation %.3e, largest component %.3e" % (what, err, scale))
    assert got.shape == want.shape and np.all(np.isfinite(got)) and err <= TOL * scale, "%s: %g > %g" % (what, err, TOL * scale)


def _by_tag(sim, force):
    tag = sim.state.tag.cpu().numpy().view(np.uint32)[: sim.state.N]
    out = np.zeros((sim.state.N, 4))
    out[tag] = np.c_[force.forces, force.energies]
    return out


def test_device_table_matches_reference():
    sim, _, _ = _sim(KINDS)
    n_excl, excl, pitch = sim.state.exclusion_table(KINDS)
    want_n, want = _tables()[KINDS]
    assert pitch == N and excl.shape == (7, N)
    assert np.array_equal(n_excl.cpu().numpy(), want_n.astype(np.int32))
    assert np.array_equal(excl.cpu().numpy().T, want.astype(np.int32))
    assert sim.state.exclusion_table(KINDS)[1] is excl      # kept
    sim.state.bond_group = sim.state.bond_group[:-1]        # a write to a group store drops it
    again = sim.state.exclusion_table(KINDS)
    assert again[1] is not excl and int(again[0].sum()) < int(n_excl.sum())


def test_fused_plan_from_cells():
    sim, nl, plj = _sim(KINDS)
    sim.run(0)
    assert nl.fused_active and plj.plan_info["valid"] == 1
    _close(np.c_[plj.forces, plj.energies], _reference(KINDS, False), "fused plan, bond + 1-3 + 1-4")


def test_list_fill():
    sim, nl, plj = _sim(KINDS, fused=False)
    sim.run(0)
    assert not nl.fused_active
    want_n = nlist_ref.all_pairs_rows(syn.pos4(_system()[0]), (L, L, L), (0.0, 0.0, 0.0), (1, 1, 1), R_LIST, N,
                                      exclusions=_tables()[KINDS])[0]
    assert np.array_equal(nl.n_neigh.cpu().numpy(), want_n)
    _close(np.c_[plj.forces, plj.energies], _reference(KINDS, False), "list fill, bond + 1-3 + 1-4")


def test_tilted_box_list_based_plan():
    sim, nl, plj = _sim(KINDS, tilted=True)
    sim.run(0)
    assert not nl.fused_active and nl._cells.fractional_cells == 1
    print("tilted box: plan %r" % ({k: plj.plan_info[k] for k in ("valid", "invalid_reason")} if plj.plan_info else None,))
    assert plj.plan_info is not None and plj.plan_info["valid"] == 1   # the tile kernel on a plan compiled from the list's rows
    _close(np.c_[plj.forces, plj.energies], _reference(KINDS, True), "tilted box, bond + 1-3 + 1-4")


def test_after_a_particle_sort():
    sim, nl, plj = _sim(KINDS)
    sim.run(0)
    sorter = azp.ParticleSorter(trigger_period=0, particles_per_block=64)
    order = sorter.sort(sim).cpu().numpy()
    assert sorted(order.tolist()) == list(range(N)) and not np.array_equal(order, np.arange(N))
    sim.run(0)
    assert nl.num_builds == 2
    # the table follows the particles: row i is the row of the tag now at i, in the new indices
    tag = sim.state.tag.cpu().numpy().view(np.uint32)[:N].astype(np.int64)
    inv = np.empty(N, dtype=np.int64)
    inv[tag] = np.arange(N)
    n_excl, excl = (t.cpu().numpy() for t in sim.state.exclusion_table(KINDS)[:2])
    want_n, want = _tables()[KINDS]
    assert np.array_equal(n_excl, want_n[tag].astype(np.int32))
    for i in (0, 3, N // 2, N - 1):
        assert sorted(excl[: n_excl[i], i].tolist()) == sorted(inv[want[tag[i], : want_n[tag[i]]]].tolist())
    _close(_by_tag(sim, plj), _reference(KINDS, False), "after a sort, by tag")


def test_negative_control_bond_only_differs():
    """The same system with the default exclusions: right against ITS reference, and far from the reference of
    bond + 1-3 + 1-4 -- the excluded 1-3 and 1-4 pairs carry force."""
    sim, nl, plj = _sim(("bond",))
    sim.run(0)
    got = np.c_[plj.forces, plj.energies]
    _close(got, _reference(("bond",), False), "bond only")
    want = _reference(KINDS, False)
    diff = np.abs(got - want).max() / np.abs(want).max()
    print("bond-only against the bond + 1-3 + 1-4 reference: %.3e of the largest component" % diff)
    assert diff > 1e6 * TOL


def test_decomposed_state_builds_its_table_from_the_topology_by_tag():
    """One rank of a chain of 6 (tags 10 .. 15) split 3 | 3 with a one-bond ghost shell, as a State with ghost rows and
    the topology by tag: the table holds the pairs whose two members are on the rank, as rows of the three locals. The
    rank's own bonds alone would miss (11, 13): its middle bead 12 is local here, but on the other side the 1-3 pair
    (12, 14) has the ghost 13 in the middle and 14 off the rank -- dropped, no error."""
    from azplugins_amd.state import State

    tags = 10 + xref.chain_bonds(1, 6)
    want_all = {(a + 10, b + 10) for a, b in xref.pair_set(KINDS, bonds=xref.chain_bonds(1, 6))}
    for rows in ([12, 10, 11, 13], [13, 15, 14, 12]):
        xyz = np.array([[0.9 * (t - 12.5), 0.0, 0.0] for t in rows])
        snap = azp.Snapshot.from_arrays(xyz, (20.0, 20.0, 20.0), tag=np.array(rows, dtype=np.uint32))
        st = State(snap, "cuda:0", n_local=3)
        st.set_global_bonds(tags, np.zeros(len(tags), dtype=np.uint32), ("A-A",))
        n_excl, excl, pitch = st.exclusion_table(KINDS)
        n_excl, excl = n_excl.cpu().numpy(), excl.cpu().numpy()
        assert pitch == 3 and excl.shape[1] == 3
        got = {tuple(sorted((rows[i], rows[int(j)]))) for i in range(3) for j in excl[: n_excl[i], i]}
        assert got == {p for p in want_all if p[0] in rows and p[1] in rows} and len(got) == 6
        assert sorted(n_excl.tolist()) == [3, 3, 3]
        # a migration re-indexes the rows: the kept table goes with the relocalized groups
        kept = st.exclusion_table(KINDS)[1]
        st.relocalize("bond")
        assert st.exclusion_table(KINDS)[1] is not kept
