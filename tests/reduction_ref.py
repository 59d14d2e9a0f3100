"""numpy restatement of the reproducible two-stage sum of csrc/azp_reduce.hpp: the same additions in the same order,
so that the sum of an array of per-particle terms comes out bit for bit as the kernels give it (thermo.hip,
wall_forces.hip).

Rows that a kernel skips (past N, not selected) are ``+0.0`` here. That is the same: an accumulator that starts at
``+0.0`` never becomes ``-0.0``, so adding ``+0.0`` changes no bit."""

import numpy as np

BLOCK = 256
WAVE = 64
TARGET_BLOCKS = 2048
MAX_PER_LANE = 128


def shape(N):
    """``(per_lane, n_blocks)`` of ``reduce_shape(N)``."""
    chunk = TARGET_BLOCKS * BLOCK
    per_lane = min(MAX_PER_LANE, max(1, (N + chunk - 1) // chunk))
    span = BLOCK * per_lane
    return per_lane, max(1, (N + span - 1) // span)


def _butterfly(v):
    """``group_sum<64>`` over the last axis (64 lanes): its DPP and permute steps pair lane ``l`` with ``l ^ s`` (or
    with a lane that holds the same value), and IEEE addition is commutative. Returns what lane 0 holds."""
    lanes = np.arange(WAVE)
    for s in (1, 2, 4, 8, 16, 32):
        v = v + v[..., lanes ^ s]
    return v[..., 0]


def tree_sum(values):
    """Sum over the last axis (the particles, ``N`` of them) of a float64 array, in the kernels' order. Leading axes
    (slots) are summed independently."""
    v = np.asarray(values, dtype=np.float64)
    lead, N = v.shape[:-1], v.shape[-1]
    per_lane, n_blocks = shape(N)
    padded = np.zeros(lead + (n_blocks * BLOCK * per_lane,))
    padded[..., :N] = v
    # particle b * 256 * per_lane + j * 256 + wave * 64 + lane
    x = padded.reshape(lead + (n_blocks, per_lane, BLOCK // WAVE, WAVE))
    acc = np.zeros(lead + (n_blocks, BLOCK // WAVE, WAVE))
    for j in range(per_lane):
        acc = acc + x[..., j, :, :]
    waves = _butterfly(acc)  # lead + (n_blocks, 4)
    partial = waves[..., 0]
    for w in range(1, BLOCK // WAVE):
        partial = partial + waves[..., w]
    # the fold: lane l takes the partials l, l + 64, ...
    trips = (n_blocks + WAVE - 1) // WAVE
    p = np.zeros(lead + (trips * WAVE,))
    p[..., :n_blocks] = partial
    p = p.reshape(lead + (trips, WAVE))
    acc = np.zeros(lead + (WAVE,))
    for t in range(trips):
        acc = acc + p[..., t, :]
    return _butterfly(acc)
