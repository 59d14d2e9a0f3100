"""The numpy side of the kernel-instance tests (no GPU): the staged-set restatement and the builder of configurations
whose fullest tile stages exactly K particles."""

import numpy as np
import pytest

import staged_sets as S


def test_stage_sizes_by_hand():
    # rows of 4 particles, tiles of 2: tile 0 lists {1, 2} | {0, 3}, tile 1 lists {1} | {0}; the members count when listed
    n_neigh = np.array([2, 2, 1, 1], dtype=np.uint32)
    head = np.array([0, 2, 4, 5], dtype=np.uint64)
    nlist = np.array([1, 2, 0, 3, 1, 0], dtype=np.uint32)
    assert S.stage_sizes((n_neigh, head, nlist), 4, 4, 2).tolist() == [4, 2]
    assert S.stage_sizes((n_neigh, head, nlist), 4, 4, 4).tolist() == [4]
    assert [S.cap_for(k) for k in (1023, 1024, 1535, 1536, 1663, 1664, 2047, 2048, 2559)] == \
        [1024, 1536, 1536, 1664, 1664, 2048, 2048, 2560, 2560]


@pytest.mark.parametrize("K,tb", [(1023, 256), (1664, 128), (2559, 64)])
def test_builder_hits_the_staged_set_exactly(oracle, K, tb):
    cfg = S.staged_set_config(K, tb)
    n_neigh, head, nlist = cfg["nl"]
    stage = S.stage_sizes(cfg["nl"], cfg["N"], cfg["N"], tb)
    assert stage.max() == K and np.array_equal(stage, cfg["stage"])
    # an ordinary list: every entry within r_list (minimum image), symmetric, rows within the plan builder's limit
    owner, j = S.row_entries(cfg["nl"], cfg["N"])
    d = cfg["pos"][owner, :3] - cfg["pos"][j, :3]
    d -= cfg["L"] * np.rint(d / cfg["L"])
    assert np.all((d * d).sum(axis=1) < cfg["r_list"] ** 2)
    pairs = set(zip(owner.tolist(), j.tolist()))
    assert all((b, a) in pairs for a, b in pairs)
    assert int(n_neigh.max()) <= 512
    # a brute-force list of the same radius is the same list
    x = cfg["pos"][:, :3]
    i0 = np.flatnonzero(n_neigh)[:50]
    for i in i0.tolist():
        dd = x - x[i]
        dd -= cfg["L"] * np.rint(dd / cfg["L"])
        want = np.flatnonzero((dd * dd).sum(axis=1) < cfg["r_list"] ** 2)
        got = np.sort(nlist[head[i]:head[i] + n_neigh[i]])
        assert np.array_equal(got, want[want != i])
    # moved particles sit alone
    assert cfg["moved"] > 0 and int((n_neigh == 0).sum()) == cfg["moved"]


def test_builder_padding_tiles_stage_nothing(oracle):
    cfg = S.staged_set_config(2047, 256, S.LIQUID)
    assert cfg["N"] == 2 * S.LIQUID
    assert np.all(cfg["stage"][S.LIQUID // 256:] == 0) and cfg["stage"].max() == 2047
