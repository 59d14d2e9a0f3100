// rdf.hip -- the pair counts behind compute.RadialDistributionFunction: for two groups A and B (per-type byte masks,
// NULL = every particle) counts[k] = number of ORDERED pairs (i in A, j in B, i != j), i over rows [0, N), j over rows
// [0, n_total), whose minimum-image distance r (min_image of azp_device.hpp) lies in bin k of num_bins equal bins on
// [0, r_max): counted iff rsq < r_max^2, r = sqrt(rsq) correctly rounded, k = min((uint32_t)(r * scale), num_bins - 1)
// with scale = num_bins / r_max from the host. The output row is num_bins + 4 uint64: the counts, then N_A, N_B and
// N_(A and B) over rows [0, N), then one zero. The call zeroes the row itself (hipMemsetAsync on the stream).
// azp_rdf_subtract_excluded, queued behind it, takes the pairs of an exclusion table out of the row again and counts
// them in that last word (rdf_subtract_excluded below): the intermolecular g(r).
//
// Two paths, the same integers wherever both are valid:
//   all-pairs  (any box, any N) grid (ceil(N / 256), segments of B). Thread t of a workgroup holds row
//              i = 256 blockIdx.x + t in registers; the workgroup streams its segment of rows [0, n_total) through LDS
//              in chunks of 256 (x, y, z as three double arrays; a candidate outside B is staged as NaN, which fails
//              rsq < r_max^2), every lane tests every staged candidate (one LDS address per wave: a broadcast read).
//   cells      (orthorhombic box, >= 3 cells of width >= r_max on every periodic axis; a non-periodic axis has
//              clamped cells, as azp_cell_grid.periodic = 0). The walk of pair_walk.hpp over all n_total particles:
//              binned in this call's scratch, the scatter writes (x, y, z, flags) rows into cell order (no order is
//              imposed inside a cell: pair counts do not depend on it); rdf_cells takes a cell's rows 256 at a time
//              and stages the members of the 27 stencil cells through LDS in chunks of 256 as above (never read
//              straight from global memory by the pair loop).
//
// Accumulation is integer throughout and on chip first: one uint32 histogram of num_bins words per workgroup in LDS,
// incremented with LDS integer atomics (ds_add_u32 without return). Overflow bound: between two flushes a bin
// receives at most one increment per (row, staged candidate) test; each staged chunk adds at most 256 x 256 = 2^16
// tests, the workgroup counts them in `pending` (the same value in every thread) and flushes before pending can pass
// 2^32 - 1. A flush adds the non-zero bins to the output row with 64-bit integer atomicAdd and clears them; the row is
// uint64, 2^64 > (2^32)^2 >= N n_total. Integer sums do not depend on the order of the adds: two calls on the same
// state give the same bits. No floating-point atomics.
//
// LDS: 3 x 256 doubles of staging (6 KB) + 4 num_bins bytes of histogram (32 KB at AZP_RDF_MAX_BINS = 8192) + the
// stencil table of the cells path (224 B).
// Bytes: all-pairs reads 32 B per (row tile, candidate): 32 n_total ceil(N / 256) in all. Cells: binning reads pos
// twice (64 B per particle) and writes 36 B per particle; the pair kernel reads 32 B per staged candidate, i.e.
// 32 x 27 x ceil(rows of the cell / 256) per particle, plus 32 B per row.
#include "pair_walk.hpp"

namespace azp
{
constexpr uint32_t RDF_BLOCK = WALK_BLOCK;
constexpr uint32_t RDF_CHUNK = 256;
constexpr uint32_t RDF_CHUNK_TESTS = RDF_BLOCK * RDF_CHUNK;       // most increments a bin gets from one staged chunk
constexpr uint32_t RDF_FLUSH_AT = 0xFFFFFFFFu - RDF_CHUNK_TESTS;  // flush once `pending` has passed this

struct RdfKArgs
    {
    const double* pos;
    const uint8_t* mask_a;
    const uint8_t* mask_b;
    unsigned long long* out;
    BoxDev box;
    double rmaxsq;
    double scale;
    uint32_t N;
    uint32_t n_total;
    uint32_t ntypes;
    uint32_t num_bins;
    // cells path
    GridDev grid;
    uint32_t ncell;
    double* sorted;        // n_total x 4: x, y, z, flags (WALK_ROW: row of A below N, WALK_CANDIDATE: member of B)
    uint32_t* start;       // ncell + 1
    uint32_t cells_per_block;
    uint32_t seg_len;      // all-pairs: candidates per segment of B (a multiple of RDF_CHUNK)
    };

// one (row, candidate) test: d = r_i - r_j before the minimum image, accepted by the rule of the walk (walk_accept)
__device__ __forceinline__ void rdf_test(const BoxDev& b, double dx, double dy, double dz, double rmaxsq, double scale,
                                         uint32_t last_bin, uint32_t* hist)
    {
    double rsq;
    if (walk_accept(b, rmaxsq, dx, dy, dz, rsq))
        {
        const double r = sqrt(rsq);  // (IEEE, correctly rounded: the bin of a pair is a property of its rsq alone)
        const uint32_t k = min((uint32_t)(r * scale), last_bin);
        atomicAdd(&hist[k], 1u);
        }
    }

// add the non-zero bins of the workgroup's histogram to the output row and clear them
__device__ __forceinline__ void rdf_flush(uint32_t* hist, uint32_t num_bins, unsigned long long* out)
    {
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < num_bins; k += RDF_BLOCK)
        {
        const uint32_t v = hist[k];
        if (v)
            {
            atomicAdd(&out[k], (unsigned long long)v);
            hist[k] = 0;
            }
        }
    __syncthreads();
    }

__global__ void __launch_bounds__(RDF_BLOCK) rdf_all_pairs(const RdfKArgs a)
    {
    extern __shared__ uint32_t s_hist[];
    __shared__ double s_x[RDF_CHUNK], s_y[RDF_CHUNK], s_z[RDF_CHUNK];
    const uint32_t tid = threadIdx.x;
    for (uint32_t k = tid; k < a.num_bins; k += RDF_BLOCK)
        s_hist[k] = 0;
    const uint64_t i = (uint64_t)blockIdx.x * RDF_BLOCK + tid;
    bool row = false;
    double xi = 0.0, yi = 0.0, zi = 0.0;
    if (i < a.N)
        {
        const double4 p = load_scalar4(a.pos, (uint32_t)i);
        xi = p.x; yi = p.y; zi = p.z;
        row = type_in_mask(a.mask_a, a.ntypes, p.w);
        }
    const uint64_t j0 = (uint64_t)blockIdx.y * a.seg_len;
    const uint64_t j1 = std::min<uint64_t>(j0 + a.seg_len, a.n_total);
    const uint32_t last_bin = a.num_bins - 1;
    const double nan = __builtin_nan("");
    uint32_t pending = 0;
    __syncthreads();
    for (uint64_t jb = j0; jb < j1; jb += RDF_CHUNK)
        {
        const uint64_t j = jb + tid;
        double x = nan, y = nan, z = nan;
        if (j < j1)
            {
            const double4 p = load_scalar4(a.pos, (uint32_t)j);
            if (type_in_mask(a.mask_b, a.ntypes, p.w))
                {
                x = p.x; y = p.y; z = p.z;
                }
            }
        s_x[tid] = x; s_y[tid] = y; s_z[tid] = z;
        __syncthreads();
        const uint32_t n = (uint32_t)std::min<uint64_t>(RDF_CHUNK, j1 - jb);
        if (row)
            {
            for (uint32_t c = 0; c < n; ++c)
                if (jb + c != i)
                    rdf_test(a.box, xi - s_x[c], yi - s_y[c], zi - s_z[c], a.rmaxsq, a.scale, last_bin, s_hist);
            }
        __syncthreads();
        pending += RDF_CHUNK_TESTS;
        if (pending > RDF_FLUSH_AT)
            {
            rdf_flush(s_hist, a.num_bins, a.out);
            pending = 0;
            }
        }
    rdf_flush(s_hist, a.num_bins, a.out);
    }

// ---------------------------------------------------------------------------------------------------------------
// pair counts from the binned particles
// ---------------------------------------------------------------------------------------------------------------
// what bin_particles' scatter leaves at a particle's slot of the cell order: its row of `sorted`
struct RdfRowSink
    {
    const double* pos;
    const uint8_t* mask_a;
    const uint8_t* mask_b;
    double* sorted;
    uint32_t N, ntypes;
    __device__ void operator()(uint32_t slot, uint32_t p) const
        {
        const double4 r = load_scalar4(pos, p);
        store_scalar4(sorted, slot, r.x, r.y, r.z,
                      walk_flags(p < N && type_in_mask(mask_a, ntypes, r.w), type_in_mask(mask_b, ntypes, r.w)));
        }
    };

__global__ void __launch_bounds__(RDF_BLOCK) rdf_cells(const RdfKArgs a)
    {
    extern __shared__ uint32_t s_hist[];
    __shared__ double s_x[RDF_CHUNK], s_y[RDF_CHUNK], s_z[RDF_CHUNK];
    __shared__ uint32_t s_seg_start[27], s_seg_end[28];  // s_seg_end[s + 1]: candidates in segments 0 .. s
    const uint32_t tid = threadIdx.x;
    for (uint32_t k = tid; k < a.num_bins; k += RDF_BLOCK)
        s_hist[k] = 0;
    const uint32_t b = xcd_remap(blockIdx.x, gridDim.x);
    const uint64_t c0 = (uint64_t)b * a.cells_per_block;
    const uint32_t c1 = (uint32_t)std::min<uint64_t>(c0 + a.cells_per_block, a.ncell);
    const uint32_t dx = a.grid.dim[0], dy = a.grid.dim[1], dz = a.grid.dim[2];
    const uint32_t last_bin = a.num_bins - 1;
    uint32_t pending = 0;
    __syncthreads();
    // (the cell loop and stencil table of the walk: the same lines in rdf_cells, st_pairs_cells and cl_union_cells,
    // pair_walk.hpp says why)
    for (uint32_t c = (uint32_t)c0; c < c1; ++c)
        {
        const uint32_t rs = a.start[c], rn = a.start[c + 1] - rs;
        if (rn == 0)
            continue;
        if (tid < 27)
            {
            const int cell[3] = {(int)(c % dx), (int)((c / dx) % dy), (int)(c / (dx * dy))};
            const int off[3] = {(int)(tid % 3) - 1, (int)((tid / 3) % 3) - 1, (int)(tid / 9) - 1};
            const int dim[3] = {(int)dx, (int)dy, (int)dz};
            int nbc[3];
            bool ok = true;
#pragma unroll
            for (int d = 0; d < 3; ++d)
                {
                int v = cell[d] + off[d];
                if (a.grid.periodic[d])
                    v = v < 0 ? v + dim[d] : (v >= dim[d] ? v - dim[d] : v);
                else if (v < 0 || v >= dim[d])
                    ok = false;
                nbc[d] = v;
                }
            uint32_t s0 = 0, cnt = 0;
            if (ok)
                {
                const uint32_t nc = ((uint32_t)nbc[2] * dy + (uint32_t)nbc[1]) * dx + (uint32_t)nbc[0];
                s0 = a.start[nc];
                cnt = a.start[nc + 1] - s0;
                }
            s_seg_start[tid] = s0;
            s_seg_end[tid + 1] = cnt;
            }
        __syncthreads();
        if (tid == 0)
            {
            uint32_t run = 0;
            s_seg_end[0] = 0;
            for (uint32_t s = 1; s <= 27; ++s)
                {
                run += s_seg_end[s];
                s_seg_end[s] = run;
                }
            }
        __syncthreads();
        const uint32_t M = s_seg_end[27];
        const uint32_t own0 = s_seg_end[13];  // the cell's own members start here in the flat candidate list
        for (uint32_t rt = 0; rt < rn; rt += RDF_BLOCK)
            {
            const uint32_t slot0 = rs + rt, T = min(RDF_BLOCK, rn - rt);
            const TileLanes l = tile_lanes(T);
            double xi, yi, zi;
            const bool row = walk_row(a.sorted, slot0, T, l.r, xi, yi, zi);
            const uint32_t self = own0 + rt + l.r;
            if (!__syncthreads_or(row))
                continue;
            for (uint32_t cb = 0; cb < M; cb += RDF_CHUNK)
                {
                const uint32_t q = cb + tid;
                double3 p = walk_no_candidate();
                if (q < M)
                    p = walk_candidate(a.sorted, walk_candidate_slot(q, s_seg_start, s_seg_end));
                s_x[tid] = p.x; s_y[tid] = p.y; s_z[tid] = p.z;
                __syncthreads();
                const uint32_t n = min(RDF_CHUNK, M - cb);
                if (row)
                    {
                    for (uint32_t cc = l.sub; cc < n; cc += l.G)
                        if (cb + cc != self)
                            rdf_test(a.box, xi - s_x[cc], yi - s_y[cc], zi - s_z[cc], a.rmaxsq, a.scale, last_bin, s_hist);
                    }
                __syncthreads();
                pending += RDF_CHUNK_TESTS;
                if (pending > RDF_FLUSH_AT)
                    {
                    rdf_flush(s_hist, a.num_bins, a.out);
                    pending = 0;
                    }
                }
            }
        }
    rdf_flush(s_hist, a.num_bins, a.out);
    }

// N_A, N_B, N_(A and B) over rows [0, N) into out[num_bins .. num_bins + 2]
__global__ void __launch_bounds__(RDF_BLOCK) rdf_group_counts(const RdfKArgs a)
    {
    __shared__ uint32_t s_n[3];
    const uint32_t tid = threadIdx.x;
    if (tid < 3)
        s_n[tid] = 0;
    __syncthreads();
    uint32_t n[3] = {0, 0, 0};
    for (uint64_t i = (uint64_t)blockIdx.x * RDF_BLOCK + tid; i < a.N; i += (uint64_t)gridDim.x * RDF_BLOCK)
        {
        const double w = a.pos[4ull * i + 3];
        const bool in_a = type_in_mask(a.mask_a, a.ntypes, w), in_b = type_in_mask(a.mask_b, a.ntypes, w);
        n[0] += in_a; n[1] += in_b; n[2] += in_a && in_b;
        }
#pragma unroll
    for (uint32_t k = 0; k < 3; ++k)
        if (n[k])
            atomicAdd(&s_n[k], n[k]);
    __syncthreads();
    if (tid < 3 && s_n[tid])
        atomicAdd(&a.out[a.num_bins + tid], (unsigned long long)s_n[tid]);
    }

// ---------------------------------------------------------------------------------------------------------------
// excluded pairs out of a finished row (azp_rdf_subtract_excluded)
// ---------------------------------------------------------------------------------------------------------------
// One lane per row i < N (grid-stride), walking the row's entries j of an exclusion table (entry s of row i at
// s * pitch + i: coalesced; the partner rows are gathers). Where i is in A and j in B the pair goes through rdf_test
// into the workgroup's histogram, exactly as the main pass put it there; the flush then SUBTRACTS the histogram from
// the row (adds 2^64 - v: integer arithmetic modulo 2^64, exact as long as the pair was counted) and adds its total
// to out[num_bins + 3]. The table is symmetric and free of duplicates, so every ordered pair comes up once.
// A workgroup's histogram takes one increment per table entry of its rows; 2^32 of them would need a table of
// 2^32 x 4 B per workgroup, which no device holds: no flush inside the loop.
__global__ void __launch_bounds__(RDF_BLOCK) rdf_subtract_excluded(const RdfKArgs a, const uint32_t* __restrict__ n_excl,
                                                                   const uint32_t* __restrict__ excl, const uint64_t pitch)
    {
    extern __shared__ uint32_t s_hist[];
    __shared__ unsigned long long s_total;
    const uint32_t tid = threadIdx.x;
    for (uint32_t k = tid; k < a.num_bins; k += RDF_BLOCK)
        s_hist[k] = 0;
    if (tid == 0)
        s_total = 0;
    __syncthreads();
    const uint32_t last_bin = a.num_bins - 1;
    for (uint64_t i = (uint64_t)blockIdx.x * RDF_BLOCK + tid; i < a.N; i += (uint64_t)gridDim.x * RDF_BLOCK)
        {
        const uint32_t n = n_excl[i];
        if (n == 0)
            continue;
        const double4 p = load_scalar4(a.pos, (uint32_t)i);
        if (!type_in_mask(a.mask_a, a.ntypes, p.w))
            continue;
        for (uint32_t s = 0; s < n; ++s)
            {
            const uint32_t j = excl[(uint64_t)s * pitch + i];
            if (j >= a.n_total || j == i)
                continue;
            const double4 q = load_scalar4(a.pos, j);
            if (type_in_mask(a.mask_b, a.ntypes, q.w))
                rdf_test(a.box, p.x - q.x, p.y - q.y, p.z - q.z, a.rmaxsq, a.scale, last_bin, s_hist);
            }
        }
    __syncthreads();
    unsigned long long mine = 0;
    for (uint32_t k = tid; k < a.num_bins; k += RDF_BLOCK)
        {
        const uint32_t v = s_hist[k];
        if (v)
            {
            atomicAdd(&a.out[k], 0ull - (unsigned long long)v);
            mine += v;
            }
        }
    if (mine)
        atomicAdd(&s_total, mine);
    __syncthreads();
    if (tid == 0 && s_total)
        atomicAdd(&a.out[a.num_bins + 3], s_total);
    }

// ---------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------
struct RdfPlan
    {
    int path;  // 1 all-pairs, 2 cells
    GridDev grid;
    CellOrder order;  // behind `sorted`, which heads the scratch
    uint64_t bytes;
    };

static int rdf_plan(const azp_rdf_args* a, RdfPlan& p)
    {
    if (!a || !(a->r_max > 0.0) || !std::isfinite(a->r_max) || a->num_bins < 1 || a->num_bins > AZP_RDF_MAX_BINS
        || !(a->scale > 0.0) || a->path > 2 || a->N > a->n_total)
        return AZP_ERROR_INVALID_ARGUMENT;
    if ((a->d_type_mask_a || a->d_type_mask_b) && a->ntypes == 0)
        return AZP_ERROR_INVALID_ARGUMENT;
    for (int d = 0; d < 3; ++d)
        if (!(a->box.L[d] > 0.0))
            return AZP_ERROR_INVALID_ARGUMENT;
    double w[3];
    box_plane_distances(a->box, w);
    for (int d = 0; d < 3; ++d)
        if (a->box.periodic[d] && a->r_max > 0.5 * w[d])
            return AZP_ERROR_INVALID_ARGUMENT;  // the minimum image would not be unique
    const bool cells = walk_make_grid(a->box, a->r_max, a->n_total, p.grid);
    if (a->path == 2 && !cells)
        return AZP_ERROR_INVALID_ARGUMENT;
    p.path = (a->path == 1 || !cells) ? 1 : 2;  // (path 0 takes the cells wherever they are valid)
    p.bytes = 0;
    if (p.path == 2)
        {
        p.order = walk_cell_order(walk_align((uint64_t)a->n_total * 32), a->n_total, p.grid, false);
        p.bytes = p.order.bytes;
        }
    return AZP_SUCCESS;
    }

static RdfKArgs rdf_kernel_args(const azp_rdf_args* args)
    {
    RdfKArgs k = {};
    k.pos = args->d_pos;
    k.mask_a = args->d_type_mask_a;
    k.mask_b = args->d_type_mask_b;
    k.out = reinterpret_cast<unsigned long long*>(args->d_out);
    k.box = make_box_dev(args->box);
    k.rmaxsq = args->r_max * args->r_max;
    k.scale = args->scale;
    k.N = args->N;
    k.n_total = args->n_total;
    k.ntypes = args->ntypes;
    k.num_bins = args->num_bins;
    return k;
    }

} // namespace azp

extern "C" int azp_rdf_scratch_size(const azp_rdf_args* args, uint64_t* bytes)
    {
    using namespace azp;
    if (!bytes)
        return AZP_ERROR_INVALID_ARGUMENT;
    RdfPlan p;
    const int rc = rdf_plan(args, p);
    if (rc != AZP_SUCCESS)
        return rc;
    *bytes = p.bytes;
    return AZP_SUCCESS;
    }

extern "C" int azp_rdf_counts(const azp_rdf_args* args, void* stream)
    {
    using namespace azp;
    RdfPlan p;
    const int rc = rdf_plan(args, p);
    if (rc != AZP_SUCCESS)
        return rc;
    if (!args->d_out || (args->n_total && !args->d_pos))
        return AZP_ERROR_INVALID_ARGUMENT;
    if (p.bytes && (!args->d_scratch || args->scratch_bytes < p.bytes))
        return AZP_ERROR_INVALID_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(args->d_out, 0, ((uint64_t)args->num_bins + 4) * sizeof(uint64_t), st);
    if (e != hipSuccess || args->N == 0)
        return (int)e;
    RdfKArgs k = rdf_kernel_args(args);
    const uint32_t n_tiles = (args->N + RDF_BLOCK - 1) / RDF_BLOCK;
    hipLaunchKernelGGL(rdf_group_counts, dim3(std::min(n_tiles, 1024u)), dim3(RDF_BLOCK), 0, st, k);
    if ((e = hipGetLastError()) != hipSuccess)
        return (int)e;
    const uint32_t lds = args->num_bins * sizeof(uint32_t);
    if (p.path == 1)
        {
        const uint32_t n_chunks = (uint32_t)(((uint64_t)args->n_total + RDF_CHUNK - 1) / RDF_CHUNK);
        uint32_t n_seg = std::min(n_chunks, std::max(1u, WALK_TARGET_BLOCKS / n_tiles));
        const uint32_t chunks_per_seg = (n_chunks + n_seg - 1) / n_seg;
        n_seg = (n_chunks + chunks_per_seg - 1) / chunks_per_seg;
        k.seg_len = chunks_per_seg * RDF_CHUNK;
        hipLaunchKernelGGL(rdf_all_pairs, dim3(n_tiles, n_seg), dim3(RDF_BLOCK), lds, st, k);
        return (int)hipGetLastError();
        }
    k.grid = p.grid;
    k.ncell = p.order.ncell;
    k.sorted = static_cast<double*>(args->d_scratch);
    k.start = walk_words(args->d_scratch, p.order.off_start);
    const RdfRowSink sink = {k.pos, k.mask_a, k.mask_b, k.sorted, k.N, k.ntypes};
    if ((e = walk_bin(args->n_total, k.pos, k.grid, args->d_scratch, p.order, k.sorted, sink, st)) != hipSuccess)
        return (int)e;
    const uint32_t grid = walk_launch_blocks(k.ncell, k.cells_per_block);
    hipLaunchKernelGGL(rdf_cells, dim3(grid), dim3(RDF_BLOCK), lds, st, k);
    return (int)hipGetLastError();
    }

extern "C" int azp_rdf_subtract_excluded(const azp_rdf_exclusion_args* xargs, void* stream)
    {
    using namespace azp;
    if (!xargs)
        return AZP_ERROR_INVALID_ARGUMENT;
    const azp_rdf_args* args = &xargs->rdf;
    azp_rdf_args any_path = *args;
    any_path.path = 1;  // (the pair pass has run: which path it took does not matter here)
    RdfPlan p;
    const int rc = rdf_plan(&any_path, p);
    if (rc != AZP_SUCCESS)
        return rc;
    if (!args->d_out || (args->n_total && !args->d_pos))
        return AZP_ERROR_INVALID_ARGUMENT;
    if (args->N == 0)
        return AZP_SUCCESS;
    if (!xargs->d_n_excl || !xargs->d_excl || xargs->excl_pitch < args->N)
        return AZP_ERROR_INVALID_ARGUMENT;
    RdfKArgs k = rdf_kernel_args(args);
    const uint32_t n_tiles = (args->N + RDF_BLOCK - 1) / RDF_BLOCK;
    hipLaunchKernelGGL(rdf_subtract_excluded, dim3(std::min(n_tiles, WALK_TARGET_BLOCKS)), dim3(RDF_BLOCK),
                       args->num_bins * sizeof(uint32_t), static_cast<hipStream_t>(stream), k, xargs->d_n_excl, xargs->d_excl,
                       xargs->excl_pitch);
    return (int)hipGetLastError();
    }
