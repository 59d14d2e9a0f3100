"""Pins tests/nlist_ref.py, the all-pairs reference of the neighbor-row tests (no GPU needed)."""

import itertools

import numpy as np

import nlist_ref as R
from azplugins_amd import synthetic as syn


def test_hand_written_rows():
    """Five particles, L = 10, r_list = 1.5: 0-1 in range (1.0), 2-3 in range across the +-x face (0.3), 0-4 in
    range (1.2) but excluded, 1-4 out of range (1.5620)."""
    xyz = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [4.8, 0.0, 0.0], [-4.9, 0.0, 0.0], [0.0, 1.2, 0.0]])
    pos = syn.pos4(xyz, np.zeros(5, dtype=np.int64))
    n_excl = np.array([1, 0, 0, 0, 1], dtype=np.uint32)
    excl = np.array([[4], [0], [0], [0], [0]], dtype=np.uint32)  # (entries past n_excl are not exclusions)
    n, rows, borderline = R.all_pairs_rows(pos, 10.0, (0, 0, 0), (1, 1, 1), np.array([[1.5]]), 5, (n_excl, excl))
    assert borderline == 0
    assert [r.tolist() for r in rows] == [[1], [0], [3], [2], []]
    assert n.tolist() == [1, 1, 1, 1, 0]
    # without the exclusion 0 and 4 list each other; without periodicity in x the pair across the face goes
    n, rows, _ = R.all_pairs_rows(pos, 10.0, (0, 0, 0), (0, 1, 1), 1.5, 5)
    assert [r.tolist() for r in rows] == [[1, 4], [0], [], [], [0]]
    # rows for the first N only, over all n_total candidates; a disabled type pair lists nothing
    pos2 = syn.pos4(xyz, np.array([0, 1, 0, 0, 0]))
    n, rows, _ = R.all_pairs_rows(pos2, 10.0, (0, 0, 0), (1, 1, 1), np.array([[1.5, 0.0], [0.0, 1.5]]), 3)
    assert [r.tolist() for r in rows] == [[4], [], [3]] and n.shape == (3,)


def test_borderline_counts_pairs_on_the_cutoff():
    xyz = np.array([[0.0, 0.0, 0.0], [1.5, 0.0, 0.0], [0.0, 1.5 * (1 + 1e-7), 0.0]])
    _, rows, borderline = R.all_pairs_rows(syn.pos4(xyz, np.zeros(3, dtype=np.int64)), 10.0, (0, 0, 0), (1, 1, 1), 1.5, 3)
    assert borderline == 2  # the pair 0-1, seen from both sides; 0-2 is 2e-7 outside in r^2
    assert rows[0].tolist() == [1]


def test_matches_oracle_on_chains(oracle):
    """Cubic periodic box, two types, per-pair radii, bonded exclusions: the oracle's 27-cell search and the
    all-pairs reference list the same rows."""
    cfg = syn.config_chains(12, 12, 12, 12)
    n = cfg["xyz"].shape[0]
    typeid = (np.arange(n) // 3) % 2
    pos = syn.pos4(cfg["xyz"], typeid)
    rl = np.array([[2.3, 1.8], [1.8, 2.7]])
    excl = R.exclusions_from_bonds(n, cfg["bonds"])
    assert excl[1].shape[1] == 2
    o_n, o_head, o_list = oracle.build_nlist(pos, oracle.make_box(cfg["L"]), rl, ntypes=2, exclusions=excl)
    r_n, rows, borderline = R.all_pairs_rows(pos, cfg["L"], (0, 0, 0), (1, 1, 1), rl, n, excl)
    assert borderline == 0
    assert np.array_equal(r_n, o_n)
    for i in range(n):
        assert np.array_equal(rows[i], np.sort(o_list[o_head[i]: o_head[i] + o_n[i]])), i


def test_tilted_box_against_the_27_images():
    """xy = 0.5 and all three tilts non-zero: the rows equal those found by trying all 27 lattice images of
    every pair. (r_list < L/2 along every axis: HOOMD's sequential minimum image then finds the nearest image;
    tilts this small keep the nearest image of two particles of the box among the 27.)"""
    L = np.array([8.0, 8.0, 8.0])
    for tilt in ((0.5, 0.0, 0.0), (0.5, 0.2, -0.3)):
        xy, xz, yz = tilt
        lattice = np.array([[L[0], 0.0, 0.0], [xy * L[1], L[1], 0.0], [xz * L[2], yz * L[2], L[2]]])
        n = 150
        tag = np.arange(n, dtype=np.uint64)
        frac = np.stack([syn.u01(91, tag, c) - 0.5 for c in range(3)], axis=1)
        xyz = frac @ lattice
        typeid = np.arange(n) % 2
        rl = np.array([[2.4, 1.9], [1.9, 3.1]])
        pos = syn.pos4(xyz, typeid)
        n_neigh, rows, borderline = R.all_pairs_rows(pos, L, tilt, (1, 1, 1), rl, n)
        assert borderline == 0
        d = xyz[:, None, :] - xyz[None, :, :]
        best = np.full((n, n), np.inf)
        for i, j, k in itertools.product((-1, 0, 1), repeat=3):
            s = d + i * lattice[0] + j * lattice[1] + k * lattice[2]
            best = np.minimum(best, (s * s).sum(axis=2))
        r = rl[typeid[:, None], typeid[None, :]]
        want = (best <= r * r) & ~np.eye(n, dtype=bool)
        crossing = 0
        for i in range(n):
            assert np.array_equal(rows[i], np.flatnonzero(want[i])), (tilt, i)
            crossing += int(np.count_nonzero((d[i, rows[i]] ** 2).sum(axis=1) > r[i, rows[i]] ** 2))
        assert crossing > 100 and n_neigh.sum() == want.sum()  # many listed pairs are images across a face


def test_tilted_pair_across_the_y_face():
    """L = 10, xy = 0.5: fractional (0.5, 0.99) and (0.5, 0.01) are 0.22 apart through the y face and 4.9 apart in
    Cartesian x (three cells of width 1.5)."""
    L, xy = 10.0, 0.5
    frac = np.array([[0.5, 0.99, 0.5], [0.5, 0.01, 0.5]]) - 0.5
    lattice = np.array([[L, 0.0, 0.0], [xy * L, L, 0.0], [0.0, 0.0, L]])
    xyz = frac @ lattice
    assert abs(abs(xyz[0, 0] - xyz[1, 0]) - 4.9) < 1e-12
    _, rows, _ = R.all_pairs_rows(syn.pos4(xyz, np.zeros(2, dtype=np.int64)), L, (xy, 0, 0), (1, 1, 1), 1.5, 2)
    assert [r.tolist() for r in rows] == [[1], [0]]
    x, y, z = R.min_image(xyz[0] - xyz[1], (L, L, L), (xy, 0, 0), (1, 1, 1))
    assert abs(np.sqrt(x * x + y * y + z * z) - np.hypot(0.2, 0.1)) < 1e-12


def test_star_topology_bond_counts():
    bonds = R.star_bonds(3, first=5)
    n_excl, excl = R.exclusions_from_bonds(5 + 3 * R.STAR_SIZE + 2, bonds)
    assert sorted(set(n_excl.tolist())) == [0, 1, 4, 5, 9] and excl.shape[1] == 9
    assert bonds.shape == (3 * 16, 2) and len({tuple(sorted(b)) for b in bonds.tolist()}) == 48
