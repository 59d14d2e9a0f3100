"""The shared bonded-group plumbing of azplugins_amd.state without a GPU, on CPU tensors: ``build_group_table`` at arity 2
against a plain loop, at arity 3 and 4 against the names it replaced, and ``localize_groups`` at arity 2."""

import numpy as np
import pytest

from azplugins_amd import _lib
from azplugins_amd.state import build_angle_table, build_dihedral_table, build_group_table, localize_bonds, localize_groups
from test_angle import _table_topology as angle_topology
from test_dihedral import _table_topology as dihedral_topology

# 12 rows, 8 of them local: a star of 5 bonds on particle 0 (two of its partners are ghosts), one of 4 on particle 4
# (two ghost partners), particle 7 without bonds, one bond between ghosts only. The stars' centres are now the first and
# now the second member of their bonds.
N_LOCAL = 8
BONDS = [(0, 1), (2, 0), (0, 3), (8, 0), (0, 9), (4, 5), (6, 4), (4, 10), (11, 4), (10, 11)]
BOND_TYPES = [j % 3 for j in range(len(BONDS))]


def _bond_table_loop(bonds, typeid, n_local):
    """The per-particle bond table by a plain loop: ``entries[i]`` is the list of (partner, type, position in the bond)
    of local particle ``i`` in slot order -- the bonds in which ``i`` is the first member, then those in which it is the
    second, each in bond order (the order of one stable sort over HOOMD's member-major list of (bond, member) pairs)."""
    entries = [[] for _ in range(n_local)]
    for which in (0, 1):
        for bond, t in zip(bonds, typeid):
            if bond[which] < n_local:
                entries[bond[which]].append((int(bond[1 - which]), int(t), which))
    return entries


def test_bond_table_matches_plain_loop():
    import torch

    tab = build_group_table(torch.tensor(BONDS, dtype=torch.int64), torch.tensor(BOND_TYPES, dtype=torch.int64), N_LOCAL, 2)
    want = _bond_table_loop(BONDS, BOND_TYPES, N_LOCAL)
    counts = [len(e) for e in want]
    assert counts == [5, 1, 1, 1, 4, 1, 1, 0]
    assert set(tab) == {"table", "bond_pos", "n_bonds", "pitch", "width"}
    assert tab["pitch"] == N_LOCAL and tab["width"] == 5
    assert tab["table"].shape == (5, N_LOCAL, 2) and tab["table"].dtype == torch.int32 and tab["table"].is_contiguous()
    assert tab["bond_pos"].shape == (5, N_LOCAL) and tab["bond_pos"].dtype == torch.int32
    assert tab["n_bonds"].dtype == torch.int32 and tab["n_bonds"].tolist() == counts
    table, bpos = tab["table"].numpy(), tab["bond_pos"].numpy()
    for i in range(N_LOCAL):
        got = [(int(table[s, i, 0]), int(table[s, i, 1]), int(bpos[s, i])) for s in range(counts[i])]
        assert got == want[i], i
        assert not table[counts[i]:, i].any() and not bpos[counts[i]:, i].any()  # unused slots stay zero
    # the slot order is pinned, not just the set of entries: particle 0 is first member of bonds 0, 2, 4 and second of 1, 3
    assert [e[0] for e in want[0]] == [1, 3, 9, 2, 8] and [e[2] for e in want[0]] == [0, 0, 0, 1, 1]
    assert [e[0] for e in want[4]] == [5, 10, 6, 11]
    # no bonds at all: one empty column per particle
    empty = build_group_table(torch.zeros((0, 2), dtype=torch.int64), torch.zeros(0, dtype=torch.int64), 5, 2)
    assert empty["width"] == 1 and empty["table"].shape == (1, 5, 2) and empty["bond_pos"].shape == (1, 5)
    assert empty["n_bonds"].tolist() == [0] * 5 and not empty["table"].any() and not empty["bond_pos"].any()


@pytest.mark.parametrize("arity", [3, 4])
def test_group_table_agrees_with_the_old_names(arity):
    import torch

    (groups, typeid, n_local), old = {3: (angle_topology(), build_angle_table), 4: (dihedral_topology(), build_dihedral_table)}[arity]
    g, t = torch.tensor(groups, dtype=torch.int64), torch.tensor(typeid, dtype=torch.int64)
    new, want = build_group_table(g, t, n_local, arity), old(g, t, n_local)
    assert set(new) == set(want) == {"table", "n_angles" if arity == 3 else "n_dihedrals", "pitch", "width"}
    for key, value in want.items():
        if torch.is_tensor(value):
            assert new[key].dtype == value.dtype and torch.equal(new[key], value), key
        else:
            assert new[key] == value, key


def test_localize_groups_arity_2():
    # rows 0-2 are local (tags 10, 11, 12), rows 3-5 ghosts (tags 13, 14 and tag 10 again: its own periodic image)
    tag = np.array([10, 11, 12, 13, 14, 10])
    bond_tags = np.array([[10, 11], [12, 13], [14, 10], [13, 14]])
    typeid = np.array([0, 1, 2, 3], dtype=np.uint32)
    group, tid = localize_groups(tag, 3, bond_tags, typeid, 2)
    assert group.dtype == np.uint32 and tid.dtype == np.uint32
    # every bond with a local member; tag 10 resolves to row 0, the lowest, not to its ghost copy in row 5; the bond
    # of two ghosts is dropped
    assert group.tolist() == [[0, 1], [2, 3], [4, 0]] and tid.tolist() == [0, 1, 2]
    for got, want in zip(localize_bonds(tag, 3, bond_tags, typeid), (group, tid)):
        assert np.array_equal(got, want)
    # a partner that is not on the rank: the shell is too narrow
    with pytest.raises(_lib.AzpError, match="a bonded partner of a local particle is neither local nor a ghost on this rank: the "
                                            r"ghost shell \(r_cut \+ buffer\) is narrower than a bond$"):
        localize_groups(tag, 3, np.array([[11, 15]]), np.array([0]), 2)
    # ... but a bond without a local member may miss a member
    group, _ = localize_groups(tag, 3, np.array([[13, 15]]), np.array([0]), 2)
    assert group.shape == (0, 2)
