// azp_reduce.hpp -- the reproducible two-stage sum of double slots over the particles (thermo.hip, wall_forces.hip,
// and through controlled_verlet.hpp thermostat.hip and fire.hip).
// Nothing is atomic and every order is fixed by N alone, so two calls on the same state give bit-identical sums, and
// a host restatement of the order (tests/reduction_ref.py) reproduces them bit for bit from the per-particle terms.
//
// The order, for N particles and reduce_shape(N) = (per_lane, n_blocks):
//   the caller's loop  lane t of workgroup b (256 threads) takes the particles b * 256 * per_lane + j * 256 + t,
//                      j < per_lane, in turn (coalesced across the lanes) and adds each one's term to an accumulator
//                      that starts at +0.0. A row that is skipped (past N, not selected) adds nothing, which is what
//                      adding +0.0 would do: an accumulator that starts at +0.0 never becomes -0.0.
//   reduce_block_store the 64 lanes of a wave are added with the DPP butterfly (group_sum<64>: lanes l and l ^ s for
//                      s = 1, 2, 4, 8, 16, 32); lane 0 of each wave writes to LDS; the four waves are added in wave
//                      order, starting from wave 0's value; one partial per workgroup and slot goes to the scratch
//                      buffer, slot-major (scratch[slot * n_blocks + b]).
//   fold_partials      one wave per slot: lane l adds the partials l, l + 64, ... in turn from +0.0, then the
//                      butterfly. reduce_fold: lane 0 writes out[slot] (any device address); cv_advance_kernel
//                      (controlled_verlet.hpp) keeps the sums in registers.
//
// Addition depth (the longest chain of additions a term passes through), for a caller that makes A additions per
// particle before the term reaches its lane's accumulator: A + per_lane + 6 + 3 + ceil(n_blocks / 64) + 6.
// per_lane = ceil(N / (2048 * 256)) clamped to [1, 128], n_blocks = ceil(N / (256 * per_lane)). Up to N = 2^24:
// per_lane <= 32 and n_blocks <= 2048, so A + 32 + 6 + 3 + 32 + 6 = A + 79. Up to N = 2^26 the lane takes up to 128:
// A + 175. Beyond, n_blocks exceeds 2048 and the fold's serial part grows with N / 2^26. (thermo.hip: A = 7, that is
// 86 and 182; tests/thermo_ref.REL_BOUND allows 200.)
//
// Only additions happen here, so the contraction setting of the including file does not matter to it.
#pragma once

#include <algorithm>

#include "azp_device.hpp"

namespace azp
{
constexpr uint32_t REDUCE_BLOCK = 256;
constexpr uint32_t REDUCE_WAVES = REDUCE_BLOCK / WAVE;
constexpr uint32_t REDUCE_TARGET_BLOCKS = 2048; // partials per slot to aim for (256 CUs x 8)
constexpr uint32_t REDUCE_MAX_PER_LANE = 128;

struct ReduceShape
    {
    uint32_t per_lane;
    uint32_t n_blocks;
    };

static ReduceShape reduce_shape(uint32_t N)
    {
    ReduceShape s;
    const uint64_t chunk = (uint64_t)REDUCE_TARGET_BLOCKS * REDUCE_BLOCK;
    s.per_lane = (uint32_t)std::min<uint64_t>(REDUCE_MAX_PER_LANE, std::max<uint64_t>(1, ((uint64_t)N + chunk - 1) / chunk));
    const uint64_t span = (uint64_t)REDUCE_BLOCK * s.per_lane;
    s.n_blocks = (uint32_t)std::max<uint64_t>(1, ((uint64_t)N + span - 1) / span);
    return s;
    }

// Every thread of a REDUCE_BLOCK workgroup calls it with its NS accumulators. s_wave: REDUCE_WAVES * NS doubles of
// LDS that the caller owns. The workgroup's partial of slot slot0 + k goes to scratch[(slot0 + k) * n_blocks + block].
template<uint32_t NS>
__device__ __forceinline__ void reduce_block_store(const double (&acc)[NS], double* s_wave, double* scratch, uint32_t slot0,
                                                   uint32_t n_blocks, uint32_t block)
    {
    const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
#pragma unroll
    for (uint32_t k = 0; k < NS; ++k)
        {
        const double s = group_sum<WAVE>(acc[k]);
        if (lane == 0)
            s_wave[wave * NS + k] = s;
        }
    __syncthreads();
    if (tid < NS)
        {
        double s = s_wave[tid];
        for (uint32_t w = 1; w < REDUCE_WAVES; ++w)
            s += s_wave[w * NS + tid];
        scratch[(uint64_t)(slot0 + tid) * n_blocks + block] = s;
        }
    }

// Every lane of one wave calls it with the n_blocks partials of one slot; all lanes return the slot's sum.
__device__ __forceinline__ double fold_partials(const double* row, uint32_t n_blocks, uint32_t lane)
    {
    double s = 0.0;
    // (unrolled: eight independent loads in flight per lane; the adds keep their order)
#pragma unroll 8
    for (uint32_t b = lane; b < n_blocks; b += WAVE)
        s += row[b];
    return group_sum<WAVE>(s);
    }

// One wave per slot (grid = the number of slots, workgroups of one wave). NEG3OF4: the slots with slot % 4 != 3 are
// stored with their sign changed (wall_forces.hip: the force ON the wall and, fourth, its energy). The sign changes
// after the sum: a sum of no terms is +0.0 and leaves as -0.0, which negated terms would not give.
template<bool NEG3OF4> __global__ void __launch_bounds__(WAVE) reduce_fold(const double* scratch, uint32_t n_blocks, double* out)
    {
    const uint32_t slot = blockIdx.x;
    const double s = fold_partials(scratch + (uint64_t)slot * n_blocks, n_blocks, threadIdx.x);
    if (threadIdx.x == 0)
        out[slot] = (NEG3OF4 && (slot & 3u) != 3u) ? -s : s;
    }

} // namespace azp
