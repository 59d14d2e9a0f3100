"""compute.RadialDistributionFunction(exclusions=...) on the GPU: exact integer equality throughout. The reference is
the all-pairs count of tests/rdf_ref.py minus a brute-force count over the reference pair set of tests/exclusion_ref.py
(adjacency sets and explicit walks), ordered pair by ordered pair, with rdf_ref's own distance and bin arithmetic."""

import functools

import numpy as np
import pytest

import exclusion_ref as xref
import rdf_ref

import azplugins_amd as azp
from azplugins_amd import _lib, compute
from azplugins_amd import synthetic as syn

pytestmark = pytest.mark.gpu

ALL_PAIRS, CELLS = _lib.RDF_PATH_ALL_PAIRS, _lib.RDF_PATH_CELLS
KINDS = ("bond", "1-3", "1-4")
CUBE = lambda L: ((L, L, L), (0.0, 0.0, 0.0), (True, True, True))  # noqa: E731


def reference_row(xyz, types, box, mask_a, mask_b, r_max, num_bins, pairs):
    """(the row with the pairs taken out, the row without exclusions): counts, N_A, N_B, N_AB, ordered pairs removed."""
    xyz = np.asarray(xyz, dtype=np.float64)
    full = rdf_ref.counts(xyz, types, box, mask_a, mask_b, r_max, num_bins)
    out = full.copy()
    in_a, in_b = rdf_ref._groups(types, mask_a, mask_b, xyz.shape[0])
    scale, rmaxsq = num_bins / float(r_max), float(r_max) * float(r_max)
    for lo, hi in sorted(pairs):
        for i, j in ((lo, hi), (hi, lo)):
            if in_a[i] and in_b[j]:
                rsq = rdf_ref._distances(xyz, np.array([i]), box)[0, j]
                if rsq < rmaxsq:
                    out[min(int(np.sqrt(rsq) * scale), num_bins - 1)] -= 1
                    out[num_bins + 3] += 1
    assert out[:num_bins].min() >= 0
    return out, full


def _sim(xyz, box, types=None, type_names=("A",), dt=None, **topology):
    L, tilt, periodic = box
    snap = azp.Snapshot.from_arrays(xyz, azp.Box(L[0], L[1], L[2], *tilt, periodic=periodic), typeid=types, types=type_names,
                                    **topology)
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(snap)
    sim.operations.tuners.clear()
    return sim


def _rdf(sim, group, r_max, num_bins, exclusions, path=0):
    f = [azp.All() if g is None else azp.Type(list(g)) for g in group]
    rdf = compute.RadialDistributionFunction(f[0], f[1], r_max, num_bins, exclusions=exclusions)
    rdf.path = path
    sim.operations.computes.append(rdf)
    return rdf


# ---------------------------------------------------------------------------
# 32 chains of 4 with alternating bead types
# ---------------------------------------------------------------------------
N_CHAINS, CHAIN, L_CHAINS, R_MAX, BINS = 32, 4, 9.0, 2.5, 50
GROUPS = {"all-all": (None, None), "A-B": (("A",), ("B",))}


@functools.lru_cache(maxsize=None)
def _chains():
    """Zig-zag chains (bond 1, 1-3 1.6, 1-4 2.5 before the jitter: some 1-4 pairs beyond r_max = 2.5, some inside), two
    to a row along x, a box of three cells of r_max + 0.5 on every axis."""
    xyz = []
    for c in range(N_CHAINS):
        x0, y0, z0 = -4.3 + 4.5 * (c % 2), -3.4 + 2.25 * ((c // 2) % 4), -3.4 + 2.25 * (c // 8)
        xyz += [(x0 + 0.8 * k, y0 + (0.3 if k % 2 else -0.3), z0) for k in range(CHAIN)]
    n = N_CHAINS * CHAIN
    xyz = np.array(xyz) + 0.2 * (np.stack([syn.u01(31, np.arange(n, dtype=np.uint64), c) for c in range(3)], axis=1) - 0.5)
    types = (np.arange(n) % 2).astype(np.uint32)
    bonds = xref.chain_bonds(N_CHAINS, CHAIN)
    return xyz, types, bonds


@functools.lru_cache(maxsize=None)
def _chains_reference(group):
    xyz, types, bonds = _chains()
    ga, gb = GROUPS[group]
    mask = lambda g: None if g is None else np.array([t in g for t in ("A", "B")])  # noqa: E731
    assert rdf_ref.edge_pairs(xyz, types, CUBE(L_CHAINS), mask(ga), mask(gb), R_MAX, BINS) == 0
    out, full = reference_row(xyz, types, CUBE(L_CHAINS), mask(ga), mask(gb), R_MAX, BINS, xref.pair_set(KINDS, bonds=bonds))
    out.setflags(write=False)
    full.setflags(write=False)
    return out, full


def test_chains_reference_removes_what_it_should():
    """On the CPU: all-all loses both orders of every bond and 1-3 pair and of the 1-4 pairs inside r_max; A-B (beads
    alternate) loses one order of the bonds and 1-4 pairs and no 1-3 pair."""
    xyz, types, bonds = _chains()
    sets = xref.pair_sets(bonds=bonds)
    assert len(sets["bond"]) == 96 and len(sets["1-3"]) == 64 and len(sets["1-4"]) == 32
    out, full = _chains_reference("all-all")
    removed = int(out[BINS + 3])
    assert 2 * (96 + 64) < removed < 2 * (96 + 64 + 32) and full[:BINS].sum() - out[:BINS].sum() == removed
    out_ab, full_ab = _chains_reference("A-B")
    assert 96 < out_ab[BINS + 3] < 96 + 32 and out_ab[BINS + 3] == full_ab[:BINS].sum() - out_ab[:BINS].sum()
    assert full[BINS + 3] == 0 and np.array_equal(out[BINS:BINS + 3], full[BINS:BINS + 3])


@pytest.mark.parametrize("path", [ALL_PAIRS, CELLS], ids=["all-pairs", "cells"])
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_chains(group, path):
    xyz, types, bonds = _chains()
    want, full = _chains_reference(group)
    sim = _sim(xyz, CUBE(L_CHAINS), types, ("A", "B"), bonds=bonds)
    rdf = _rdf(sim, GROUPS[group], R_MAX, BINS, KINDS, path)
    row = rdf._read("row")
    assert np.array_equal(row, want), (np.nonzero(row != want)[0][:8], row[-4:], want[-4:])
    assert rdf.excluded_pairs == want[BINS + 3] > 0
    assert np.array_equal(rdf.counts, want[:BINS]) and rdf.group_sizes == tuple(want[BINS:BINS + 3])
    # the normalisation is that of the run without exclusions
    assert np.array_equal(rdf.rdf, compute.rdf_from_counts(want[:BINS], want[BINS], want[BINS + 1], want[BINS + 2], L_CHAINS ** 3, R_MAX))
    # two reads agree bit for bit
    assert np.array_equal(rdf._read("row"), row)
    # without exclusions: the parent's row, the spare word zero
    plain = _rdf(sim, GROUPS[group], R_MAX, BINS, (), path)
    assert np.array_equal(plain._read("row"), full) and plain.excluded_pairs == 0
    # names that exclude nothing here leave the spare word zero too
    none = _rdf(sim, GROUPS[group], R_MAX, BINS, ("angle", "special_pair", "body"), path)
    assert np.array_equal(none._read("row"), full)


def test_ring_of_three_with_every_option():
    """Every pair of the ring is named by its bond, by a 1-3 walk, by an angle, by a dihedral and by special pairs in
    both orders: it must come out once. Without deduplication a bin would underflow."""
    xyz = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.5, 0.8, 0.0], [3.0, 3.0, 3.0], [3.0, 3.9, 3.0]])
    topology = dict(bonds=[(0, 1), (1, 2), (2, 0), (0, 1)], angles=[(0, 1, 2), (1, 2, 0), (2, 0, 1)], dihedrals=[(0, 1, 2, 1), (2, 1, 0, 2)],
                    pairs=[(0, 1), (1, 0), (2, 1), (0, 2)])
    pairs = xref.pair_set(xref.OPTIONS, **topology)
    assert pairs == {(0, 1), (0, 2), (1, 2)}
    box = CUBE(12.0)
    want, full = reference_row(xyz, np.zeros(5, dtype=np.uint32), box, None, None, 3.0, 24, pairs)
    sim = _sim(xyz, box, **topology)
    for path in (ALL_PAIRS, CELLS):
        row = _rdf(sim, (None, None), 3.0, 24, xref.OPTIONS, path)._read("row")
        assert np.array_equal(row, want) and row[24 + 3] == 6
        assert np.all(row[:24] <= full[:24]) and row[:24].sum() == 2     # what is left: the unbonded pair, both orders


def test_pairs_beyond_r_max_and_on_bin_edges():
    """Dyadic positions (exact in any order of operations). Bonded pairs at distance 1 (the lower edge of bin 8 of 32
    bins on [0, 4)), at exactly r_max = 4 (not counted, so not subtracted) and at 5 (beyond); an unbonded pair at
    distance 1 elsewhere, which must stay in bin 8."""
    xyz = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0],        # bonded, r = 1
                    [0.0, 2.5, 0.0], [1.0, 2.5, 0.0],        # not bonded, r = 1
                    [-6.0, -6.0, -6.0], [-2.0, -6.0, -6.0],  # bonded, r = 4 = r_max
                    [6.0, 6.0, 6.0], [6.0, 1.0, 6.0]])       # bonded, r = 5
    bonds = [(0, 1), (4, 5), (6, 7)]
    box = CUBE(32.0)
    want, full = reference_row(xyz, np.zeros(8, dtype=np.uint32), box, None, None, 4.0, 32, xref.pair_set(("bond",), bonds=bonds))
    assert full[8] == 4 and want[8] == 2 and want[32 + 3] == 2
    sim = _sim(xyz, box, bonds=bonds)
    for path in (ALL_PAIRS, CELLS):
        row = _rdf(sim, (None, None), 4.0, 32, ("bond",), path)._read("row")
        assert np.array_equal(row, want), (path, row, want)
        assert row[8] == 2 and row[32 + 3] == 2 and row[:32].sum() == full[:32].sum() - 2


def test_recorder_rows_equal_the_computes_rows():
    """dt = 0: every recorded frame is the state the compute reads afterwards."""
    xyz, types, bonds = _chains()
    want, _ = _chains_reference("all-all")
    sim = _sim(xyz, CUBE(L_CHAINS), types, ("A", "B"), bonds=bonds)
    dw = azp.bond.DoubleWell()
    dw.params["A-A"] = dict(r_0=1.0, r_1=1.5, U_1=1.0, U_tilt=0.5)
    sim.operations.integrator = azp.Integrator(dt=0.0, forces=[dw], methods=[azp.ConstantVolume()])
    rdf = compute.RadialDistributionFunction(azp.All(), azp.All(), R_MAX, BINS, exclusions=KINDS)
    sim.operations.add(rdf)
    rec = compute.RDFRecorder(rdf, 1)
    sim.operations.add(rec)
    sim.run(3)
    table = rec._table("rows")
    assert table.shape[0] >= 3 and table.shape[1] == BINS + 4
    row = rdf._read("row")
    assert np.array_equal(row, want)
    for frame in table:
        assert np.array_equal(frame, row)
    assert np.array_equal(rec.counts[0], want[:BINS])
    assert np.array_equal(rec.rdf[0], rdf.rdf)
