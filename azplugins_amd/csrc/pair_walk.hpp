// pair_walk.hpp -- the one owner of how the analysis computes find their pairs: azp_rdf_counts (rdf.hip),
// azp_steinhardt_compute (steinhardt.hip) and azp_cluster_compute (cluster.hip) compose their pair kernels from the
// pieces below and keep what differs: their per-slot extras, what a lane does with an accepted pair, their chunk loops.
//
// The walk. All particles are binned by bin_particles (cell_bin.hpp) into this call's scratch; the caller's sink leaves a
// row (x, y, z, flags) per slot of the cell order in `sorted`. A workgroup of 256 threads owns a contiguous range of
// cells; per non-empty cell it builds the table of the up to 27 contiguous candidate segments of the stencil and takes
// the cell's rows a tile at a time. A tile of T rows is served by 256 / pow2ceil(T) lanes per row (tile_lanes); the
// flat list of the M candidates is staged through LDS in chunks (walk_candidate_slot, walk_candidate: a candidate that
// is not wanted is staged as NaN, which fails rsq < r_max^2), and a pair is taken where walk_accept says so. The
// all-pairs kernels are the same tile against one segment, the row order itself.
// The cell loop and its stencil table are NOT here: rdf_cells, st_pairs_cells and cl_union_cells each write them out,
// line for line the same. As a shared function (taking the tile as a lambda, or only filling the table) they changed
// the minimum-image code the compiler emits for the pair loops, and every call took 1.4 to 6 % longer on an MI355X
// (profiles/pair_walk.md). Change the three together.
// The non-template host functions are inline: three translation units include this header.
#pragma once

#include <algorithm>
#include <cmath>

#include "cell_bin.hpp"

namespace azp
{
constexpr uint32_t WALK_BLOCK = 256;            // threads of a pair kernel
constexpr uint32_t WALK_TARGET_BLOCKS = 2048;   // 256 CUs x 8
constexpr uint32_t WALK_MAX_CELLS = 1u << 21;
// the flags word of a row of `sorted`, stored as a double
constexpr uint32_t WALK_ROW = 1u;        // the slot is a row: its pairs are wanted
constexpr uint32_t WALK_CANDIDATE = 2u;  // the slot is a candidate: it may be the other end of a pair

__device__ __forceinline__ double walk_flags(bool row, bool candidate)
    {
    return (double)((row ? WALK_ROW : 0u) | (candidate ? WALK_CANDIDATE : 0u));
    }

// T rows, Tp = pow2ceil(T) row slots, G = 256 / Tp lanes per row: this thread is lane `sub` of row slot r (a row iff
// r < T) and takes the staged candidates sub, sub + G, ...
struct TileLanes
    {
    uint32_t G, r, sub;
    };

__device__ __forceinline__ TileLanes tile_lanes(uint32_t T)
    {
    const uint32_t lg = T > 1 ? 32u - (uint32_t)__builtin_clz(T - 1) : 0u;
    return {WALK_BLOCK >> lg, threadIdx.x & ((1u << lg) - 1u), threadIdx.x >> lg};
    }

// this thread's row of the tile [slot0, slot0 + T): its position, and whether its pairs are wanted
__device__ __forceinline__ bool walk_row(const double* sorted, uint32_t slot0, uint32_t T, uint32_t r, double& xi, double& yi,
                                         double& zi)
    {
    xi = yi = zi = 0.0;
    if (r >= T)
        return false;
    const double4 p = load_scalar4(sorted, slot0 + r);
    xi = p.x; yi = p.y; zi = p.z;
    return ((uint32_t)p.w & WALK_ROW) != 0;
    }

// the slot of candidate q < M of the flat list; seg_end[s + 1] = candidates in segments 0 .. s, seg_end[0] = 0
__device__ __forceinline__ uint32_t walk_candidate_slot(uint32_t q, const uint32_t* seg_start, const uint32_t* seg_end)
    {
    uint32_t s = 0;
    while (q >= seg_end[s + 1])
        ++s;
    return seg_start[s] + (q - seg_end[s]);
    }

__device__ __forceinline__ double3 walk_no_candidate()
    {
    const double nan = __builtin_nan("");
    return make_double3(nan, nan, nan);
    }

// what is staged for a slot: its position, NaN unless it is a candidate
__device__ __forceinline__ double3 walk_candidate(const double* sorted, uint32_t slot)
    {
    const double4 p = load_scalar4(sorted, slot);
    return ((uint32_t)p.w & WALK_CANDIDATE) ? make_double3(p.x, p.y, p.z) : walk_no_candidate();
    }

// The acceptance test: d = r_i - r_j on entry, its minimum image on return, rsq = |d|^2. (This expression, in this order:
// the RDF bins on sqrt(rsq), and all three computes must accept the same pairs.)
__device__ __forceinline__ bool walk_accept(const BoxDev& b, double rmaxsq, double& dx, double& dy, double& dz, double& rsq)
    {
    min_image(b, dx, dy, dz);
    rsq = dx * dx + dy * dy + dz * dz;
    return rsq < rmaxsq;
    }

// ---------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------
// The cell grid of the walk over n particles: floor(L / r_max) cells per axis, at least 3 on a periodic one; false if the
// box does not allow it (tilted, or too narrow). winv = dim / L, filled here: make_grid_dev's 1 / (L / dim) may differ in
// the last bit.
inline bool walk_make_grid(const azp_box& b, double r_max, uint32_t n, GridDev& g)
    {
    if (b.tilt[0] != 0.0 || b.tilt[1] != 0.0 || b.tilt[2] != 0.0)
        return false;
    double dim[3];
    for (int d = 0; d < 3; ++d)
        {
        dim[d] = std::floor(b.L[d] / r_max);
        if (b.periodic[d] && dim[d] < 3.0)
            return false;
        dim[d] = std::min(std::max(dim[d], 1.0), 1024.0);
        }
    // (a sparse system: no more cells than a few per particle, at most WALK_MAX_CELLS; wider cells stay valid)
    const double cap = std::min<double>(WALK_MAX_CELLS, std::max<double>(64.0, 2.0 * n));
    for (int pass = 0; pass < 64 && dim[0] * dim[1] * dim[2] > cap; ++pass)
        {
        const double f = std::cbrt(cap / (dim[0] * dim[1] * dim[2]));
        for (int d = 0; d < 3; ++d)
            dim[d] = std::max(b.periodic[d] ? 3.0 : 1.0, std::floor(dim[d] * std::min(f, 0.95)));
        }
    if (dim[0] * dim[1] * dim[2] > (double)WALK_MAX_CELLS)
        return false;
    for (int d = 0; d < 3; ++d)
        {
        g.dim[d] = (int)dim[d];
        g.lo[d] = -0.5 * b.L[d];
        g.winv[d] = dim[d] / b.L[d];
        g.periodic[d] = b.periodic[d] != 0;
        }
    return true;
    }

inline uint64_t walk_align(uint64_t x) { return (x + 255) & ~(uint64_t)255; }

// The cell order's part of a call's scratch, behind the caller's own arrays: byte offsets of cell_id[n], count[ncell],
// start[ncell + 1] and, if asked for, perm[n] (slot -> row); `bytes` is where it ends.
struct CellOrder
    {
    uint32_t ncell;
    uint64_t off_cell_id, off_count, off_start, off_perm, bytes;
    };

inline CellOrder walk_cell_order(uint64_t base, uint64_t n, const GridDev& g, bool with_perm)
    {
    CellOrder o;
    o.ncell = (uint32_t)g.dim[0] * (uint32_t)g.dim[1] * (uint32_t)g.dim[2];
    o.off_cell_id = base;
    o.off_count = o.off_cell_id + walk_align(n * 4);
    o.off_start = o.off_count + walk_align((uint64_t)o.ncell * 4);
    o.off_perm = o.off_start + walk_align(((uint64_t)o.ncell + 1) * 4);
    o.bytes = o.off_perm + (with_perm ? walk_align(n * 4) : 0);
    return o;
    }

inline uint32_t* walk_words(void* scratch, uint64_t offset) { return reinterpret_cast<uint32_t*>(static_cast<char*>(scratch) + offset); }

// Bins the n particles into the cell order of `scratch`; sink(slot, i) writes particle i's row of `sorted` (n x 4
// doubles) and the caller's per-slot extras. The block totals of bin_particles' three-kernel scan live in the head of
// `sorted`, which the scatter fills only afterwards: nblk + 1 <= n words fit into n rows.
template<class Sink>
inline hipError_t walk_bin(uint32_t n, const double* pos, const GridDev& g, void* scratch, const CellOrder& o, double* sorted,
                           const Sink& sink, hipStream_t s)
    {
    return bin_particles(n, pos, g, nullptr, walk_words(scratch, o.off_cell_id), walk_words(scratch, o.off_count),
                         walk_words(scratch, o.off_start), reinterpret_cast<uint32_t*>(sorted), sink, s);
    }

// The launch of a cells kernel: a multiple of 8 workgroups, each a contiguous range of cells_per_block cells (xcd_remap
// gives every XCD one eighth of the grid).
inline uint32_t walk_launch_blocks(uint32_t ncell, uint32_t& cells_per_block)
    {
    const uint32_t grid = (std::min(ncell, WALK_TARGET_BLOCKS) + 7u) & ~7u;
    cells_per_block = (ncell + grid - 1) / grid;
    return grid;
    }
} // namespace azp
