"""The exclusion table builder of azplugins_amd.state without a GPU, on CPU tensors, against the plain-Python reference
``exclusion_ref`` (adjacency sets and explicit walks): every option alone and all together on the topologies that guard
its corner cases, the bond-only default against what ``State.exclusion_table`` returned before there were options, the
names that are refused, the localization by tag of a decomposed run, and the "pair" kind through the group plumbing."""

import numpy as np
import pytest

import exclusion_ref as xref
from azplugins_amd import _lib, nlist
from azplugins_amd.state import (ARITY, EXCLUSIONS, KINDS, Snapshot, build_exclusion_table, build_group_table, check_exclusions,
                                 excluded_pairs, localize_groups, localize_pairs)

# name -> (number of particles, topology); the comments say what each guards
TOPOLOGIES = {
    # an interior bead gets 2 bonds + 2 1-3 + 2 1-4 = 6 entries
    "chain6": (6, dict(bonds=xref.chain_bonds(1, 6))),
    # its 1-3 pairs are also bonds, its only 1-4 walks end where they start
    "ring3": (3, dict(bonds=[(0, 1), (1, 2), (2, 0)])),
    # 1-3 pairs are reached by two walks, the 1-4 walks end on a bond
    "ring4": (4, dict(bonds=[(0, 1), (1, 2), (2, 3), (3, 0)])),
    # the centre has 5 entries, each arm has 1 bond and 4 1-3 pairs
    "star5": (6, dict(bonds=xref.star_bonds(1, 5))),
    # two disjoint chains plus explicit angles, dihedrals and special pairs that follow no bond
    "explicit": (10, dict(bonds=np.concatenate([xref.chain_bonds(1, 4), xref.chain_bonds(1, 5, first=4)]),
                          angles=[(0, 5, 9), (3, 1, 4), (2, 2, 7), (9, 0, 0)], dihedrals=[(0, 1, 2, 8), (9, 3, 3, 1), (6, 5, 4, 6)],
                          pairs=[(0, 9), (9, 0), (2, 6), (5, 5), (3, 4)])),
}
OPTION_SETS = [(name,) for name in xref.OPTIONS] + [tuple(xref.OPTIONS)]


def _members(topology):
    import torch

    key = dict(bonds="bond", angles="angle", dihedrals="dihedral", pairs="pair")
    return {key[k]: torch.as_tensor(np.asarray(v, dtype=np.int64).reshape(-1, ARITY[key[k]])) for k, v in topology.items()}


def _check_table(table, want_pairs, N):
    """The table holds exactly the pairs of ``want_pairs`` (unordered, both members below N here), symmetric, without
    duplicates and self-entries, every row ascending."""
    n_excl, excl, pitch = table
    n_excl, excl = n_excl.numpy(), excl.numpy()
    assert pitch == N and n_excl.shape == (N,) and excl.shape[1] == N and excl.shape[0] >= 1
    assert n_excl.dtype == np.int32 and excl.dtype == np.int32
    ordered = set()
    for i in range(N):
        row = excl[: n_excl[i], i].tolist()
        assert row == sorted(row), (i, row)
        assert len(set(row)) == len(row), (i, row)
        assert i not in row, (i, row)
        ordered |= {(i, j) for j in row}
        assert not excl[n_excl[i]:, i].any()
    assert all((j, i) in ordered for i, j in ordered)
    assert {(min(i, j), max(i, j)) for i, j in ordered} == want_pairs
    assert excl.shape[0] == max(int(n_excl.max()), 1)


@pytest.mark.parametrize("options", OPTION_SETS, ids=["+".join(o) for o in OPTION_SETS])
@pytest.mark.parametrize("name", sorted(TOPOLOGIES))
def test_builder_matches_reference(name, options):
    N, topology = TOPOLOGIES[name]
    want = xref.pair_set(options, **topology)
    pairs = excluded_pairs(check_exclusions(options), _members(topology))
    _check_table(build_exclusion_table(pairs, N), want, N)
    n_excl, excl = xref.table(want, N)
    got = build_exclusion_table(pairs, N)
    assert np.array_equal(got[0].numpy(), n_excl.astype(np.int32))
    assert np.array_equal(got[1].numpy().T[:, : excl.shape[1]], excl.astype(np.int32))


def test_reference_known_counts():
    """The reference itself on the cases whose numbers the topologies were chosen for."""
    s = xref.pair_sets(**TOPOLOGIES["chain6"][1])
    assert s["1-3"] == {(0, 2), (1, 3), (2, 4), (3, 5)} and s["1-4"] == {(0, 3), (1, 4), (2, 5)}
    n_excl, _ = xref.table(xref.pair_set(("bond", "1-3", "1-4"), **TOPOLOGIES["chain6"][1]), 6)
    assert n_excl.tolist() == [3, 4, 5, 5, 4, 3]
    chain8 = dict(bonds=xref.chain_bonds(1, 8))
    assert xref.table(xref.pair_set(("bond", "1-3", "1-4"), **chain8), 8)[0].max() == 6
    s = xref.pair_sets(**TOPOLOGIES["ring3"][1])
    assert s["1-3"] == s["bond"] == {(0, 1), (0, 2), (1, 2)} and s["1-4"] == set()
    s = xref.pair_sets(**TOPOLOGIES["ring4"][1])
    assert s["1-3"] == {(0, 2), (1, 3)} and s["1-4"] == s["bond"]
    s = xref.pair_sets(**TOPOLOGIES["star5"][1])
    assert len(s["bond"]) == 5 and len(s["1-3"]) == 10 and s["1-4"] == set()
    n_excl, _ = xref.table(s["bond"] | s["1-3"], 6)
    assert n_excl.tolist() == [5, 5, 5, 5, 5, 5]


def test_bond_only_is_the_bond_table_column():
    """``kinds == ("bond",)``: element for element what ``exclusion_table()`` has always returned -- the partner column
    of the bond table in that table's order (first-member bonds before second-member bonds), not the sorted merged form.
    ``State`` needs a device, so its method's two lines are restated on the CPU table they read."""
    import torch

    from test_bonded import BONDS, BOND_TYPES, N_LOCAL
    from azplugins_amd.state import State

    t = build_group_table(torch.tensor(BONDS, dtype=torch.int64), torch.tensor(BOND_TYPES, dtype=torch.int64), N_LOCAL, "bond")

    class _Stub:
        groups = {}
        bond_table = staticmethod(lambda: t)

    n_excl, excl, pitch = State.exclusion_table(_Stub(), ("bond",))
    assert pitch == N_LOCAL
    assert torch.equal(n_excl, t["n_bonds"]) and torch.equal(excl, t["table"][:, :, 0])
    assert excl[: int(n_excl[0]), 0].tolist() == [1, 3, 9, 2, 8]  # (table order: not ascending)
    n_excl_d, excl_d, _ = State.exclusion_table(_Stub())
    assert torch.equal(n_excl_d, n_excl) and torch.equal(excl_d, excl)


def test_names():
    assert check_exclusions(("1-4", "bond", "bond")) == ("bond", "1-4")
    assert check_exclusions(()) == ()
    assert check_exclusions(("body", "constraint", "meshbond")) == ()
    assert check_exclusions(EXCLUSIONS) == EXCLUSIONS
    for bad in (("bonds",), ("bond", "1-5"), ("pair",)):
        with pytest.raises(_lib.AzpError, match="unknown name"):
            check_exclusions(bad)
        with pytest.raises(_lib.AzpError, match="unknown name"):
            nlist.Cell(buffer=0.4, exclusions=bad)
    assert nlist.Cell(buffer=0.4).exclusions == ("bond",)
    nl = nlist.Cell(buffer=0.4, exclusions=("bond", "1-3", "body"))
    assert nl.exclusions == ("bond", "1-3", "body") and nl._exclusion_kinds == ("bond", "1-3")


def test_rdf_takes_the_same_names():
    from azplugins_amd import All, compute

    rdf = compute.RadialDistributionFunction(All(), All(), 2.0, 10, exclusions=("bond", "1-3", "meshbond"))
    assert rdf._exclusion_kinds == ("bond", "1-3")
    assert compute.RadialDistributionFunction(All(), All(), 2.0, 10).exclusions == ()
    with pytest.raises(_lib.AzpError, match="unknown name"):
        compute.RadialDistributionFunction(All(), All(), 2.0, 10, exclusions=("intramolecular",))


def test_localization_by_tag_of_a_split_chain():
    """A chain of 6 (tags 10 .. 15) split 3 | 3 with a one-bond ghost shell: each side holds exactly the pairs whose two
    members are on it, as rows for its three local particles. The 1-3 pair (12, 14) on the left has its middle bead as a
    ghost and its partner off the rank: dropped, no error."""
    import torch

    tags = 10 + xref.chain_bonds(1, 6)
    kinds = ("bond", "1-3", "1-4")
    pairs = excluded_pairs(kinds, {"bond": torch.as_tensor(tags)})
    want_all = {(a + 10, b + 10) for a, b in xref.pair_set(kinds, bonds=xref.chain_bonds(1, 6))}
    for rows in ([12, 10, 11, 13], [13, 15, 14, 12]):  # local rows, then the ghost
        tag = torch.tensor(rows, dtype=torch.int32)
        local = localize_pairs(pairs, tag, 3)
        on_rank = set(rows)
        want = {tuple(sorted((rows.index(a), rows.index(b)))) for a, b in want_all if a in on_rank and b in on_rank}
        assert len(want) == 6
        n_excl, excl, pitch = build_exclusion_table(local, 3)
        got = {(i, int(j)) for i in range(3) for j in excl[: int(n_excl[i]), i]}
        assert {(min(p), max(p)) for p in got} == want
        assert all((j, i) in got for i, j in got if j < 3)      # symmetric among the locals
        assert all(i < 3 for i, _ in got) and pitch == 3 and excl.shape[1] == 3
        assert sorted(n_excl.tolist()) == sorted([sum(1 for p in want if i in p) for i in range(3)])
    # a particle that is on the rank twice (a local and its own periodic ghost) is its lowest row
    local = localize_pairs(pairs, torch.tensor([10, 11, 12, 10], dtype=torch.int32), 3)
    assert set(map(tuple, local.tolist())) == {(0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (2, 1)}


def test_pair_kind_goes_through_the_group_plumbing():
    import torch

    assert "pair" in KINDS and ARITY["pair"] == 2
    snap = Snapshot.from_arrays(np.zeros((5, 3)), [10.0, 10.0, 10.0], pairs=[(0, 3), (4, 0), (1, 2)], pair_typeid=[0, 1, 1], pair_types=("s", "t"))
    assert snap.pairs.N == 3 and snap.pairs.types == ["s", "t"] and snap.pairs.group.tolist() == [[0, 3], [4, 0], [1, 2]]
    assert Snapshot().pairs.N == 0
    tab = build_group_table(torch.tensor(snap.pairs.group.astype(np.int64)), torch.tensor([0, 1, 1]), 4, "pair")
    assert "n_pairs" in tab and "n_bonds" not in tab
    assert tab["n_pairs"].tolist() == [2, 1, 1, 1] and tab["pitch"] == 4 and tab["width"] == 2
    assert tab["table"][:2, 0].tolist() == [[3, 0], [4, 1]] and tab["bond_pos"][:2, 0].tolist() == [0, 1]
    # the arities still name the three kinds they always named
    assert "n_bonds" in build_group_table(torch.zeros((0, 2), dtype=torch.int64), torch.zeros(0, dtype=torch.int64), 3, 2)
    tag = np.array([7, 8, 9, 20])
    group, tid = localize_groups(tag, 3, np.array([[7, 20], [9, 8], [20, 21]]), np.array([0, 1, 1]), 2, "pair")
    assert group.tolist() == [[0, 3], [2, 1]] and tid.tolist() == [0, 1]
    with pytest.raises(_lib.AzpError, match="special pair"):
        localize_groups(tag, 3, np.array([[7, 30]]), np.array([0]), 2, "pair")
    with pytest.raises(_lib.AzpError, match="narrower than a bond"):
        localize_groups(tag, 3, np.array([[7, 30]]), np.array([0]), 2)


def test_decomposition_carries_the_pair_kind():
    """The topology by tag that a decomposed run replicates holds the special pairs next to the other kinds."""
    from azplugins_amd.decomposition import _snapshot_topology

    snap = Snapshot.from_arrays(np.zeros((5, 3)), [10.0, 10.0, 10.0], tag=[7, 8, 9, 3, 4], bonds=[(0, 1)], pairs=[(0, 3), (4, 0)],
                                pair_typeid=[1, 0], pair_types=("s", "t"))
    topo = _snapshot_topology(snap)
    assert topo["pair_tags"].tolist() == [[7, 3], [4, 7]] and topo["pair_typeid"].tolist() == [1, 0] and topo["pair_types"] == ("s", "t")
    assert topo["bond_tags"].tolist() == [[7, 8]] and "angle_tags" not in topo
    only_pairs = _snapshot_topology(Snapshot.from_arrays(np.zeros((2, 3)), [10.0, 10.0, 10.0], pairs=[(0, 1)]))
    assert only_pairs["pair_tags"].tolist() == [[0, 1]] and only_pairs["bond_tags"].shape == (0, 2)
