// sf_shape.hpp -- how the amplitude kernels cut the particles into stages and chunks: shared by structure_factor.hip
// (sf_partial) and displacement.hip (ss_partial), so that the two sums have the same shape, the same fold and the same
// addition depth. Moved here unchanged from structure_factor.hip.
#pragma once

#include <algorithm>

#include "azp_device.hpp"

namespace azp
{
constexpr uint32_t SF_BLOCK = 256;
constexpr uint32_t SF_TARGET_BLOCKS = 4096; // 256 CUs x 16
constexpr uint32_t SF_MIN_CHUNKS = 16, SF_MAX_CHUNKS = 512;

struct SfShape
    {
    uint32_t stages, n_chunks;
    };

static SfShape sf_shape(uint32_t N, uint32_t n_vectors)
    {
    const uint32_t vblocks = (n_vectors + SF_BLOCK - 1) / SF_BLOCK;
    const uint32_t target = std::min(std::max(SF_TARGET_BLOCKS / std::max(vblocks, 1u), SF_MIN_CHUNKS), SF_MAX_CHUNKS);
    const uint32_t n_stages = (uint32_t)(((uint64_t)N + SF_BLOCK - 1) / SF_BLOCK);
    SfShape s;
    s.stages = std::max(1u, (n_stages + target - 1) / target);
    s.n_chunks = std::max(1u, (n_stages + s.stages - 1) / s.stages);
    return s;
    }

} // namespace azp
