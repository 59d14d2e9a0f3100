"""tests/reduction_ref.py (the host restatement of csrc/azp_reduce.hpp's addition order) against values worked out
by hand and against a slow restatement whose order can be read off its loops. No GPU."""

import math

import numpy as np
import pytest

import reduction_ref as red


@pytest.mark.parametrize("N,want", [
    (0, (1, 1)),                # nothing: one (empty) workgroup
    (1, (1, 1)),
    (256, (1, 1)),              # one full workgroup
    (257, (1, 2)),
    (524288, (1, 2048)),        # 2048 * 256: the last N with one particle per lane
    (524289, (2, 1025)),        # ceil(524289 / 512)
    (2**24, (32, 2048)),        # 2^24 / 2^19 = 32 per lane, 2^24 / (256 * 32) workgroups
    (2**26 + 1, (128, 2049)),   # 129 per lane clamped to 128; ceil((2^26 + 1) / 2^15)
])
def test_shape(N, want):
    assert red.shape(N) == want


@pytest.mark.parametrize("N", [1, 64, 65, 257, 1000, 524289])
def test_small_integers_sum_exactly(N):
    rng = np.random.default_rng(N)
    v = rng.integers(-1000, 1000, (3, N)).astype(np.float64)
    got = red.tree_sum(v)
    assert got.shape == (3,)
    assert got.tolist() == v.sum(axis=1).tolist() == [float(int(r.sum())) for r in v.astype(np.int64)]
    assert red.tree_sum(v[0]) == got[0]


def _slow_tree_sum(values):
    """The order of csrc/azp_reduce.hpp with Python floats, one addition at a time; rows past N are skipped, as the
    kernels skip them."""
    N = len(values)
    per_lane, n_blocks = red.shape(N)

    def butterfly(lanes):
        for s in (1, 2, 4, 8, 16, 32):
            lanes = [lanes[l] + lanes[l ^ s] for l in range(64)]
        return lanes[0]

    partials = []
    for b in range(n_blocks):
        waves = []
        for w in range(4):
            lanes = []
            for l in range(64):
                acc = 0.0
                for j in range(per_lane):
                    i = b * 256 * per_lane + j * 256 + w * 64 + l
                    if i < N:
                        acc += values[i]
                lanes.append(acc)
            waves.append(butterfly(lanes))
        s = waves[0]
        for w in (1, 2, 3):
            s += waves[w]
        partials.append(s)
    lanes = []
    for l in range(64):
        acc = 0.0
        for b in range(l, n_blocks, 64):
            acc += partials[b]
        lanes.append(acc)
    return butterfly(lanes)


def _planted(N):
    """1e16, 1.0, -1e16, 1.0 repeated, then scaled by position: the big terms cancel exactly in ``math.fsum``, while
    any order that adds a 1.0 to a 1e16 first loses it."""
    v = np.tile(np.array([1e16, 1.0, -1e16, 1.0]), (N + 3) // 4)[:N]
    return v * (1.0 + (np.arange(N) % 7))


@pytest.mark.parametrize("N", [65, 1000])
def test_order_is_the_documented_one(N):
    v = _planted(N)
    got = float(red.tree_sum(v))
    exact = math.fsum(v.tolist())
    print("N=%d tree %.17g fsum %.17g" % (N, got, exact))
    assert got != exact  # (the order matters on this array)
    assert got == _slow_tree_sum(v.tolist())
    # another order gives other bits: the planted array tells orders apart
    assert got != float(red.tree_sum(v[::-1]))
