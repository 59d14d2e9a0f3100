// cell_bin.hpp -- the only place that bins particles into cells: the grid and its cell rule, and a counting sort by cell
// (count with wave-aggregated atomics, exclusive scan, scatter through a caller's sink). bin_particles is run by
// azp_nlist_bin (nlist.hip) and, through walk_bin (pair_walk.hpp), by the cells paths of azp_rdf_counts (rdf.hip),
// azp_steinhardt_compute (steinhardt.hip) and azp_cluster_compute (cluster.hip); azp_nlist_cell_assign runs the assign
// kernel alone. The non-template kernels are static: several translation units include this header.
#pragma once

#include "azp_device.hpp"

namespace azp
{
struct GridDev
    {
    double lo[3], winv[3];
    int dim[3];
    int periodic[3];
    };

inline GridDev make_grid_dev(const azp_cell_grid& g)
    {
    GridDev d;
    for (int k = 0; k < 3; ++k)
        {
        d.lo[k] = g.lo[k];
        d.winv[k] = 1.0 / g.width[k];
        d.dim[k] = (int)g.dim[k];
        d.periodic[k] = g.periodic[k];
        }
    return d;
    }

// floor((x - lo) / width), wrapped on a periodic axis, clamped on another. fmax / fmin drop a NaN and bound everything
// else ahead of the double -> int conversion (undefined out of range): such a particle lands in some cell of the axis.
__device__ __forceinline__ int cell_coord(const GridDev& g, int k, double x)
    {
    int c = (int)floor(fmin(fmax((x - g.lo[k]) * g.winv[k], -1.0e9), 1.0e9));
    if (g.periodic[k])
        {
        c %= g.dim[k];
        if (c < 0) c += g.dim[k];
        }
    else
        c = min(max(c, 0), g.dim[k] - 1);
    return c;
    }

// Fractional cells (azp_nlist_args.fractional_cells): the grid lives in the coordinates f along the lattice vectors,
// f in [-0.5, 0.5) for a wrapped particle (wrap_into_box's own frame); the cells are parallelepipeds.
struct FracDev
    {
    double xy, xzp, yz; // xzp = xz - xy yz
    double Lxinv, Lyinv, Lzinv;
    };

inline FracDev make_frac_dev(const azp_box& b)
    {
    FracDev f;
    f.xy = b.tilt[0]; f.xzp = b.tilt[1] - b.tilt[0] * b.tilt[2]; f.yz = b.tilt[2];
    f.Lxinv = 1.0 / b.L[0]; f.Lyinv = 1.0 / b.L[1]; f.Lzinv = 1.0 / b.L[2];
    return f;
    }

__device__ __forceinline__ double3 fractional(const FracDev& f, double x, double y, double z)
    {
    return make_double3(__builtin_fma(-f.xzp, z, __builtin_fma(-f.xy, y, x)) * f.Lxinv, __builtin_fma(-f.yz, z, y) * f.Lyinv,
                        z * f.Lzinv);
    }

__device__ __forceinline__ uint32_t cell_index(const GridDev& g, const double3& p)
    {
    const int cx = cell_coord(g, 0, p.x), cy = cell_coord(g, 1, p.y), cz = cell_coord(g, 2, p.z);
    return (uint32_t)((cz * g.dim[1] + cy) * g.dim[0] + cx);
    }

// Lanes of a wave that hold the same key add to its counter with ONE atomic (consecutive particles of a spatially sorted
// system sit in the same cell: a plain atomic per lane serialises 32-deep on one address). Returns this lane's slot
// base + rank among the wave's lanes with that key.
__device__ __forceinline__ uint32_t wave_aggregated_add(uint32_t* counters, uint32_t key, bool active)
    {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t result = 0;
    unsigned long long todo = __ballot(active);
    while (todo)
        {
        const int leader = __builtin_ctzll(todo);
        const uint32_t k0 = (uint32_t)__shfl((int)key, leader, 64);
        const unsigned long long same = __ballot(active && key == k0) & todo;
        uint32_t base = 0;
        if ((int)lane == leader)
            base = atomicAdd(&counters[k0], (uint32_t)__popcll(same));
        base = (uint32_t)__shfl((int)base, leader, 64);
        if (active && key == k0)
            result = base + (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
        todo &= ~same;
        }
    return result;
    }

// cell_of[i] = cell of particle i (FRAC: of its fractional coordinates); COUNT: and one more in count[cell]
template<bool FRAC, bool COUNT>
__global__ void __launch_bounds__(256) cell_assign_kernel(uint32_t n_total, const double* __restrict__ pos, GridDev g, FracDev fr,
                                                          uint32_t* __restrict__ cell_of, uint32_t* __restrict__ count)
    {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = i < n_total;
    uint32_t c = 0;
    if (active)
        {
        double3 p = load_scalar3_of4(pos, i);
        if (FRAC)
            p = fractional(fr, p.x, p.y, p.z);
        c = cell_index(g, p);
        cell_of[i] = c;
        }
    if (COUNT)
        (void)wave_aggregated_add(count, c, active);
    }

constexpr uint32_t BIN_SCAN_BLOCK = 4096; // counters per workgroup of the three-kernel scan

// Exclusive scan of in[0 .. n) by ONE workgroup of 1,024 threads: out[0 .. n) = the prefix sums, out[n] = the total,
// mirror[0 .. n) = the prefix sums too unless NULL (the scatter's cursors). `in` may be `out` or `mirror`: a trip's reads
// all precede its writes (the barriers), and no pointer is __restrict__. Wave scans by shuffles, one LDS hop for the 16
// wave totals, the carry from trip to trip in a register. 4,096 counters per trip, four adjacent ones per thread (16 B
// per lane, 1 KB per wave: still whole cache lines): on 32^3 cells 6 us faster than one counter per thread and four
// times the trips (profiles/cell_bin.md). A span of ncell / 1024 counters per thread is what costs a line per lane.
static __global__ void __launch_bounds__(1024) bin_scan_kernel(uint32_t n, const uint32_t* in, uint32_t* out, uint32_t* mirror)
    {
    constexpr uint32_t PER = 4;
    __shared__ uint32_t s_wave[16];
    const uint32_t t = threadIdx.x;
    uint32_t carry = 0;
    for (uint32_t c0 = 0; c0 < n; c0 += 1024u * PER)
        {
        const uint32_t c = c0 + PER * t;
        uint32_t v[PER], mine = 0;
#pragma unroll
        for (uint32_t k = 0; k < PER; ++k)
            {
            v[k] = (c + k < n) ? in[c + k] : 0u;
            mine += v[k];
            }
        uint32_t total;
        uint32_t acc = carry + block_exclusive_scan<16>(mine, s_wave, total);
        __syncthreads(); // (every read of in[] and s_wave of this trip is done)
#pragma unroll
        for (uint32_t k = 0; k < PER; ++k)
            {
            if (c + k < n)
                {
                out[c + k] = acc;
                if (mirror)
                    mirror[c + k] = acc;
                }
            acc += v[k];
            }
        carry += total;
        }
    if (t == 0)
        out[n] = carry;
    }

// The same scan for grids of many cells (half-width cells: 2^18 at N = 2^20), where one workgroup's dependent trips
// would take longer than the rest of the binning: every workgroup scans 4,096 cells on its own and leaves its total,
// bin_scan_kernel scans the totals in place, a third pass adds them in.
static __global__ void __launch_bounds__(1024) bin_scan_local_kernel(uint32_t ncell, const uint32_t* __restrict__ count,
                                                                     uint32_t* __restrict__ cell_start, uint32_t* __restrict__ block_total)
    {
    __shared__ uint32_t s_wave[16];
    const uint32_t t = threadIdx.x;
    const uint32_t c = blockIdx.x * BIN_SCAN_BLOCK + 4u * t;
    uint32_t v[4];
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k)
        v[k] = (c + k < ncell) ? count[c + k] : 0u;
    uint32_t total;
    uint32_t acc = block_exclusive_scan<16>(v[0] + v[1] + v[2] + v[3], s_wave, total);
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k)
        {
        if (c + k < ncell)
            cell_start[c + k] = acc;
        acc += v[k];
        }
    if (t == 0)
        block_total[blockIdx.x] = total;
    }

static __global__ void __launch_bounds__(256) bin_scan_add_kernel(uint32_t ncell, const uint32_t* __restrict__ block_start,
                                                                  uint32_t* __restrict__ cursor, uint32_t* __restrict__ cell_start)
    {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c < ncell)
        {
        const uint32_t v = cell_start[c] + block_start[c >> 12];
        cell_start[c] = v;
        cursor[c] = v;
        }
    else if (c == ncell)
        cell_start[ncell] = block_start[(ncell + BIN_SCAN_BLOCK - 1u) >> 12]; // (the scan of the totals leaves the grand total behind the last)
    }

// sink(slot, i): particle i has the position `slot` of the cell order (any order of the WAVES inside a cell)
template<class Sink>
__global__ void __launch_bounds__(256) bin_scatter_kernel(uint32_t n_total, const uint32_t* __restrict__ cell_of, uint32_t* __restrict__ cursor,
                                                          const Sink sink)
    {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = i < n_total;
    const uint32_t c = active ? cell_of[i] : 0u;
    const uint32_t slot = wave_aggregated_add(cursor, c, active);
    if (active)
        sink(slot, i);
    }

// Counting sort of n particles by cell on stream s: cell_of[n] = the cell ids (fr non-NULL: fractional cells),
// cell_start[ncell + 1] = first slot of every cell + the total, and sink(slot, i) for every particle. cursor: ncell
// words of scratch. block_tmp: scratch of the three-kernel scan, taken iff the grid has more than 8 blocks of 4,096
// cells and nblk + 1 <= n, and then nblk + 1 words; the sink's own output may serve (the scatter runs afterwards).
template<class Sink>
inline hipError_t bin_particles(uint32_t n, const double* pos, const GridDev& g, const FracDev* fr, uint32_t* cell_of, uint32_t* cursor,
                                uint32_t* cell_start, uint32_t* block_tmp, const Sink& sink, hipStream_t s)
    {
    const uint32_t ncell = (uint32_t)g.dim[0] * (uint32_t)g.dim[1] * (uint32_t)g.dim[2];
    const hipError_t e = hipMemsetAsync(cursor, 0, sizeof(uint32_t) * (size_t)ncell, s);
    if (e != hipSuccess)
        return e;
    const dim3 per_particle((n + 255u) / 256u), b256(256), b1024(1024);
    if (n && fr)
        hipLaunchKernelGGL((cell_assign_kernel<true, true>), per_particle, b256, 0, s, n, pos, g, *fr, cell_of, cursor);
    else if (n)
        hipLaunchKernelGGL((cell_assign_kernel<false, true>), per_particle, b256, 0, s, n, pos, g, FracDev{}, cell_of, cursor);
    const uint32_t nblk = (ncell + BIN_SCAN_BLOCK - 1u) / BIN_SCAN_BLOCK;
    if (nblk > 8u && nblk + 1u <= n)
        {
        hipLaunchKernelGGL(bin_scan_local_kernel, dim3(nblk), b1024, 0, s, ncell, cursor, cell_start, block_tmp);
        hipLaunchKernelGGL(bin_scan_kernel, dim3(1), b1024, 0, s, nblk, block_tmp, block_tmp, (uint32_t*)nullptr);
        hipLaunchKernelGGL(bin_scan_add_kernel, dim3((ncell + 1u + 255u) / 256u), b256, 0, s, ncell, block_tmp, cursor, cell_start);
        }
    else
        hipLaunchKernelGGL(bin_scan_kernel, dim3(1), b1024, 0, s, ncell, cursor, cell_start, cursor);
    if (n)
        hipLaunchKernelGGL(bin_scatter_kernel<Sink>, per_particle, b256, 0, s, n, cell_of, cursor, sink);
    return hipGetLastError();
    }
} // namespace azp
