// steinhardt.hip -- bond-orientational order behind compute.Steinhardt and compute.SolidLiquid (include/azp.h,
// DESIGN 4.28): per particle the fixed-point sums S_lm of the spherical harmonics of its bonds, q_l from them, the
// neighbour average (Lechner-Dellago) and the solid-bond count (ten Wolde-Frenkel), and one summary row.
//
// Every pass over the pairs is the walk of pair_walk.hpp: a tile of T <= `tile` rows that are contiguous
// in the order the pass works in, against a flat list of M candidates made of up to 27 contiguous segments of that
// order, staged through LDS in chunks (x, y, z as three double arrays), the lanes split over the rows by tile_lanes, a
// pair accepted by walk_accept.
//   cells      the order is the cell order (walk_bin in this call's scratch; the scatter leaves (x, y, z, flags) rows
//              and the permutation); st_pairs_cells takes a cell's rows `tile` at a time against the members of its 27
//              stencil cells. What the first pass leaves (S, N_b, then q_lm as fixed point or normalised) stays in cell
//              order, so the second pass stages it the same way.
//   all-pairs  the order is the row order, the candidates are the one segment [0, N); a workgroup per tile.
// Three passes (template MODE): 0 the terms, 1 the neighbour average, 2 the solid bonds.
//
// Accumulation: per row `words` int64 in LDS, added to with 64-bit integer LDS atomics by whichever lane accepted the
// pair (pass 0: straight from the recurrence, term by term, so no lane holds an array: the register count does not
// depend on the l asked for; pass 1: the candidate's staged words). The tile's rows are then stored once, no global
// atomics. Integers throughout: no order of the lanes, the chunks or the cells changes a bit.
// LDS: 3 x chunk doubles of staging + tile x words x 8 B of rows + in the second passes chunk x words x 8 B of candidate
// words. First pass: chunk 256, tile = min(256, pow2floor(ST_ROW_BYTES / (8 words))), 64 rows for l = (4, 6): 18.5 KB, so
// that eight workgroups share a CU (with 48 KB of rows and two per CU the pass took 1.7 times as long at N = 2^20,
// profiles/steinhardt.md). Second passes: tile = chunk = min(128, pow2floor(ST_ROW_BYTES_2 / (8 words))).
#include "pair_walk.hpp"
#include "steinhardt_device.hpp"

namespace azp
{
constexpr uint32_t ST_BLOCK = WALK_BLOCK;
constexpr uint32_t ST_ROW_BYTES = 12288;    // the rows of a first-pass tile
constexpr uint32_t ST_ROW_BYTES_2 = 24576;  // the rows of a second-pass tile, and as much again for a chunk's candidates

struct StKArgs
    {
    const double* pos;
    const uint8_t* mask;
    uint32_t N, ntypes;
    BoxDev box;
    double rmaxsq;
    SteinhardtTerms terms;
    uint32_t words;            // terms.words
    uint32_t tile, chunk;      // rows per tile and candidates per chunk of the pass being launched
    // the order the passes work in
    double* sorted;            // N x 4: x, y, z, flags (WALK_ROW | WALK_CANDIDATE: in G)
    const uint32_t* perm;      // slot -> row, NULL: the row order itself
    GridDev grid;
    uint32_t ncell, cells_per_block;
    const uint32_t* start;     // ncell + 1
    // per slot
    long long* S;              // N x words: pass 0; pass 1 leaves T here
    uint32_t* nb;              // N
    long long* Q;              // N x words: llrint(q_lm 2^40)
    double* qhat;              // N x words: q_lm / |q|, NaN where |q| == 0
    double q_threshold;
    uint32_t solid_threshold, flags, num_bins;
    // per row
    uint32_t* out_nb;
    long long* out_words;
    double* out_order;
    long long* out_avg_words;
    uint32_t* out_ncon;
    unsigned long long* summary;
    };

// particle p's row of `sorted` at `slot`
__device__ __forceinline__ void st_init_slot(const double* pos, const uint8_t* mask, uint32_t ntypes, double* sorted, uint32_t slot,
                                             uint32_t p)
    {
    const double4 r = load_scalar4(pos, p);
    const bool in = type_in_mask(mask, ntypes, r.w);
    store_scalar4(sorted, slot, r.x, r.y, r.z, walk_flags(in, in));
    }

// the rows in row order (the all-pairs path)
__global__ void __launch_bounds__(ST_BLOCK) st_rows_kernel(const StKArgs a)
    {
    const uint32_t p = blockIdx.x * ST_BLOCK + threadIdx.x;
    if (p < a.N)
        st_init_slot(a.pos, a.mask, a.ntypes, a.sorted, p, p);
    }

// the rows in cell order: what bin_particles' scatter leaves at a particle's slot
struct StRowSink
    {
    const double* pos;
    const uint8_t* mask;
    double* sorted;
    uint32_t* perm;
    uint32_t ntypes;
    __device__ void operator()(uint32_t slot, uint32_t p) const
        {
        st_init_slot(pos, mask, ntypes, sorted, slot, p);
        perm[slot] = p;
        }
    };

struct StEmit
    {
    unsigned long long* row;
    __device__ __forceinline__ void operator()(uint32_t w, long long v) const
        {
        if (v)
            atomicAdd(row + w, (unsigned long long)v);
        }
    };

// One tile: rows [slot0, slot0 + T) against the M candidates of the segment table; self0 = the flat candidate index of
// row slot0. Called by every thread of the workgroup with the same arguments.
template<int MODE>
__device__ __forceinline__ void st_tile(const StKArgs& a, uint32_t slot0, uint32_t T, uint32_t M, uint32_t self0,
                                        const uint32_t* s_seg_start, const uint32_t* s_seg_end)
    {
    extern __shared__ double st_lds[];
    const uint32_t C = a.chunk, W = a.words, tid = threadIdx.x;
    double* s_x = st_lds;
    double* s_y = s_x + C;
    double* s_z = s_y + C;
    unsigned long long* s_acc = reinterpret_cast<unsigned long long*>(s_z + C);  // tile x W (MODE 2: the rows' qhat)
    double* s_rowq = reinterpret_cast<double*>(s_acc);
    unsigned long long* s_cand = s_acc + (uint64_t)a.tile * W;                   // chunk x W (MODE 1: Q, MODE 2: qhat)
    double* s_candq = reinterpret_cast<double*>(s_cand);
    uint32_t* s_cnt = reinterpret_cast<uint32_t*>(s_cand + (MODE ? (uint64_t)C * W : 0));  // tile

    for (uint32_t k = tid; k < T * W; k += ST_BLOCK)
        {
        if (MODE == 2)
            s_rowq[k] = a.qhat[(uint64_t)slot0 * W + k];
        else
            s_acc[k] = 0;
        }
    if (tid < T)
        s_cnt[tid] = 0;
    const TileLanes l = tile_lanes(T);
    const uint32_t r = l.r;
    double xi, yi, zi;
    const bool row = walk_row(a.sorted, slot0, T, r, xi, yi, zi);
    const uint32_t self = self0 + r;
    if (__syncthreads_or(row))
        {
        for (uint32_t cb = 0; cb < M; cb += C)
            {
            const uint32_t q = cb + tid;
            if (tid < C)
                {
                double3 c = walk_no_candidate();
                if (q < M)
                    {
                    const uint32_t slot = walk_candidate_slot(q, s_seg_start, s_seg_end);
                    c = walk_candidate(a.sorted, slot);
                    if (MODE == 1)
                        for (uint32_t k = 0; k < W; ++k)
                            s_cand[(uint64_t)tid * W + k] = (unsigned long long)a.Q[(uint64_t)slot * W + k];
                    if (MODE == 2)
                        for (uint32_t k = 0; k < W; ++k)
                            s_candq[(uint64_t)tid * W + k] = a.qhat[(uint64_t)slot * W + k];
                    }
                s_x[tid] = c.x; s_y[tid] = c.y; s_z[tid] = c.z;
                }
            __syncthreads();
            const uint32_t n = min(C, M - cb);
            if (row)
                {
                for (uint32_t cc = l.sub; cc < n; cc += l.G)
                    {
                    if (MODE != 1 && cb + cc == self)
                        continue;
                    double dx = xi - s_x[cc], dy = yi - s_y[cc], dz = zi - s_z[cc], rsq;
                    if (!walk_accept(a.box, a.rmaxsq, dx, dy, dz, rsq))
                        continue;
                    if (MODE == 0)
                        {
                        atomicAdd(&s_cnt[r], 1u);
                        steinhardt_term(a.terms, -dx, -dy, -dz, rsq, StEmit{s_acc + (uint64_t)r * W});
                        }
                    else if (MODE == 1)
                        {
                        for (uint32_t k = 0; k < W; ++k)
                            {
                            const unsigned long long v = s_cand[(uint64_t)cc * W + k];
                            if (v)
                                atomicAdd(&s_acc[(uint64_t)r * W + k], v);
                            }
                        }
                    else
                        {
                        const double* qi = s_rowq + (uint64_t)r * W;
                        const double* qj = s_candq + (uint64_t)cc * W;
                        double d = qi[0] * qj[0];
                        for (uint32_t m = 1; m <= a.terms.l[0]; ++m)
                            d += 2.0 * (qi[2 * m] * qj[2 * m] + qi[2 * m + 1] * qj[2 * m + 1]);
                        if (d > a.q_threshold)  // (a NaN, from a norm of 0, is never solid)
                            atomicAdd(&s_cnt[r], 1u);
                        }
                    }
                }
            __syncthreads();
            }
        }
    if (MODE == 2)
        {
        if (tid < T)
            a.out_ncon[a.perm ? a.perm[slot0 + tid] : slot0 + tid] = s_cnt[tid];
        }
    else
        {
        for (uint32_t k = tid; k < T * W; k += ST_BLOCK)
            a.S[(uint64_t)slot0 * W + k] = (long long)s_acc[k];
        if (MODE == 0 && tid < T)
            a.nb[slot0 + tid] = s_cnt[tid];
        }
    __syncthreads();
    }

template<int MODE>
__global__ void __launch_bounds__(ST_BLOCK) st_pairs_all(const StKArgs a)
    {
    __shared__ uint32_t s_seg_start[1], s_seg_end[2];
    if (threadIdx.x == 0)
        {
        s_seg_start[0] = 0;
        s_seg_end[0] = 0;
        s_seg_end[1] = a.N;
        }
    __syncthreads();
    const uint32_t slot0 = blockIdx.x * a.tile;  // (the grid is ceil(N / tile): slot0 < N)
    st_tile<MODE>(a, slot0, min(a.tile, a.N - slot0), a.N, slot0, s_seg_start, s_seg_end);
    }

template<int MODE>
__global__ void __launch_bounds__(ST_BLOCK) st_pairs_cells(const StKArgs a)
    {
    __shared__ uint32_t s_seg_start[27], s_seg_end[28];  // s_seg_end[s + 1]: candidates in segments 0 .. s
    const uint32_t tid = threadIdx.x;
    const uint32_t b = xcd_remap(blockIdx.x, gridDim.x);
    const uint64_t c0 = (uint64_t)b * a.cells_per_block;
    const uint32_t c1 = (uint32_t)std::min<uint64_t>(c0 + a.cells_per_block, a.ncell);
    const uint32_t dx = a.grid.dim[0], dy = a.grid.dim[1], dz = a.grid.dim[2];
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
        for (uint32_t rt = 0; rt < rn; rt += a.tile)
            st_tile<MODE>(a, rs + rt, min(a.tile, rn - rt), M, own0 + rt, s_seg_start, s_seg_end);
        }
    }

// q_lm, q_l and what the second passes stage, per slot, from the first pass's sums; the per-row outputs of that pass
__global__ void __launch_bounds__(ST_BLOCK) st_finish_kernel(const StKArgs a)
    {
    const uint32_t s = blockIdx.x * ST_BLOCK + threadIdx.x;
    if (s >= a.N)
        return;
    const uint32_t p = a.perm ? a.perm[s] : s;
    const uint32_t W = a.words, nt = a.terms.n_terms;
    const uint32_t nb = a.nb[s];
    const double denom = (double)nb;
    const long long* w = a.S + (uint64_t)s * W;
    a.out_nb[p] = nb;
    for (uint32_t k = 0; k < W; ++k)
        a.out_words[(uint64_t)p * W + k] = w[k];
    for (uint32_t t = 0; t < nt; ++t)
        {
        const uint32_t l = a.terms.l[t], off = a.terms.offset[t];
        if (!(a.flags & AZP_STEINHARDT_AVERAGE))
            a.out_order[(uint64_t)p * nt + t] = steinhardt_ql(w + off, l, denom);
        else
            for (uint32_t k = 0; k < 2 * (l + 1); ++k)
                a.Q[(uint64_t)s * W + off + k] = (long long)llrint(steinhardt_component(w[off + k], denom) * ST_FIXED);
        if (a.flags & AZP_STEINHARDT_CONNECTIONS)
            {
            const double nsq = steinhardt_norm_sq(w + off, l, denom);
            const double norm = nsq > 0.0 ? sqrt(nsq) : __builtin_nan("");
            for (uint32_t k = 0; k < 2 * (l + 1); ++k)
                a.qhat[(uint64_t)s * W + off + k] = steinhardt_component(w[off + k], denom) / norm;
            }
        }
    }

// qbar_l per slot from the second pass's sums T (left in S)
__global__ void __launch_bounds__(ST_BLOCK) st_finish_avg_kernel(const StKArgs a)
    {
    const uint32_t s = blockIdx.x * ST_BLOCK + threadIdx.x;
    if (s >= a.N)
        return;
    const uint32_t p = a.perm ? a.perm[s] : s;
    const uint32_t W = a.words, nt = a.terms.n_terms;
    const double denom = (double)a.nb[s] + 1.0;
    const long long* w = a.S + (uint64_t)s * W;
    for (uint32_t k = 0; k < W; ++k)
        a.out_avg_words[(uint64_t)p * W + k] = w[k];
    for (uint32_t t = 0; t < nt; ++t)
        a.out_order[(uint64_t)p * nt + t] = steinhardt_ql(w + a.terms.offset[t], a.terms.l[t], denom);
    }

// the summary row from the per-row outputs: the workgroup's counts in LDS first (integer LDS atomics), then its
// non-zero words into the row with 64-bit integer atomics
__global__ void __launch_bounds__(ST_BLOCK) st_summary_kernel(const StKArgs a)
    {
    extern __shared__ double st_lds[];
    uint32_t* s_hist = reinterpret_cast<uint32_t*>(st_lds);  // n_terms x num_bins, then the 33 connection bins
    __shared__ unsigned long long s_head[4 + ST_MAX_TERMS];
    const uint32_t tid = threadIdx.x, nt = a.terms.n_terms;
    const uint32_t n_hist = nt * a.num_bins + AZP_STEINHARDT_CONNECTION_BINS;
    for (uint32_t k = tid; k < n_hist; k += ST_BLOCK)
        s_hist[k] = 0;
    if (tid < 4 + ST_MAX_TERMS)
        s_head[tid] = 0;
    __syncthreads();
    uint32_t* s_conn = s_hist + nt * a.num_bins;
    unsigned long long head[4] = {0, 0, 0, 0};
    long long sum_q[ST_MAX_TERMS] = {0, 0, 0, 0};
    for (uint64_t p = (uint64_t)blockIdx.x * ST_BLOCK + tid; p < a.N; p += (uint64_t)gridDim.x * ST_BLOCK)
        {
        if (!type_in_mask(a.mask, a.ntypes, a.pos[4ull * p + 3]))
            continue;
        const uint32_t nb = a.out_nb[p];
        head[0] += 1;
        head[1] += nb > 0;
        head[2] += nb;
#pragma unroll
        for (uint32_t t = 0; t < ST_MAX_TERMS; ++t)
            if (t < nt)
                {
                const double q = a.out_order[p * nt + t];
                sum_q[t] += (long long)llrint(q * ST_FIXED);
                atomicAdd(&s_hist[t * a.num_bins + min((uint32_t)(q * (double)a.num_bins), a.num_bins - 1)], 1u);
                }
        if (a.flags & AZP_STEINHARDT_CONNECTIONS)
            {
            const uint32_t nc = a.out_ncon[p];
            head[3] += nc >= a.solid_threshold;
            atomicAdd(&s_conn[min(nc, (uint32_t)AZP_STEINHARDT_CONNECTION_BINS - 1)], 1u);
            }
        }
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k)
        if (head[k])
            atomicAdd(&s_head[k], head[k]);
#pragma unroll
    for (uint32_t t = 0; t < ST_MAX_TERMS; ++t)
        if (sum_q[t])
            atomicAdd(&s_head[4 + t], (unsigned long long)sum_q[t]);
    __syncthreads();
    if (tid < 4 + nt && s_head[tid])
        atomicAdd(&a.summary[tid], s_head[tid]);
    for (uint32_t k = tid; k < n_hist; k += ST_BLOCK)
        if (s_hist[k])
            atomicAdd(&a.summary[4 + nt + k], (unsigned long long)s_hist[k]);
    }

// ---------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------
struct StPlan
    {
    int path;  // 1 all-pairs, 2 cells
    SteinhardtTerms terms;
    GridDev grid;
    CellOrder order;  // path 2: behind the per-slot arrays
    uint32_t tile, tile2;
    uint64_t off_S, off_nb, off_Q, off_qhat, bytes;
    };

static int st_plan(const azp_steinhardt_args* a, StPlan& p)
    {
    if (!a || !(a->r_max > 0.0) || !std::isfinite(a->r_max) || a->path > 2 || a->N > AZP_STEINHARDT_MAX_N
        || a->num_bins < 1 || a->num_bins > AZP_STEINHARDT_MAX_BINS
        || (a->flags & ~(AZP_STEINHARDT_AVERAGE | AZP_STEINHARDT_CONNECTIONS)))
        return AZP_ERROR_INVALID_ARGUMENT;
    if (!steinhardt_make_terms(a->n_terms, a->l, a->norm, p.terms))
        return AZP_ERROR_INVALID_ARGUMENT;
    if ((a->flags & AZP_STEINHARDT_CONNECTIONS) && (a->n_terms != 1 || !std::isfinite(a->q_threshold)))
        return AZP_ERROR_INVALID_ARGUMENT;
    if (a->d_type_mask && a->ntypes == 0)
        return AZP_ERROR_INVALID_ARGUMENT;
    for (int d = 0; d < 3; ++d)
        if (!(a->box.L[d] > 0.0))
            return AZP_ERROR_INVALID_ARGUMENT;
    double w[3];
    box_plane_distances(a->box, w);
    for (int d = 0; d < 3; ++d)
        if (a->box.periodic[d] && a->r_max > 0.5 * w[d])
            return AZP_ERROR_INVALID_ARGUMENT;  // the minimum image would not be unique
    const bool cells = walk_make_grid(a->box, a->r_max, a->N, p.grid);
    if (a->path == 2 && !cells)
        return AZP_ERROR_INVALID_ARGUMENT;
    p.path = (a->path == 1 || !cells) ? 1 : 2;
    const uint32_t W = p.terms.words;
    p.tile = ST_BLOCK;
    while ((uint64_t)p.tile * W * 8 > ST_ROW_BYTES)
        p.tile >>= 1;
    p.tile2 = ST_BLOCK / 2;
    while ((uint64_t)p.tile2 * W * 8 > ST_ROW_BYTES_2)
        p.tile2 >>= 1;
    const uint64_t n = a->N, row_words = walk_align(n * W * 8);
    p.off_S = walk_align(n * 32);
    p.off_nb = p.off_S + row_words;
    p.off_Q = p.off_nb + walk_align(n * 4);
    p.off_qhat = p.off_Q + ((a->flags & AZP_STEINHARDT_AVERAGE) ? row_words : 0);
    p.bytes = p.off_qhat + ((a->flags & AZP_STEINHARDT_CONNECTIONS) ? row_words : 0);
    if (p.path == 2)
        {
        p.order = walk_cell_order(p.bytes, n, p.grid, true);
        p.bytes = p.order.bytes;
        }
    return AZP_SUCCESS;
    }

static uint32_t st_summary_words(const azp_steinhardt_args* a)
    {
    return 4 + a->n_terms * (1 + a->num_bins) + AZP_STEINHARDT_CONNECTION_BINS;
    }

template<int MODE>
static hipError_t st_launch_pairs(const StPlan& p, StKArgs& k, hipStream_t st)
    {
    // the second passes hold the candidates' words beside the rows': as many candidates per chunk as rows per tile
    k.tile = MODE ? p.tile2 : p.tile;
    k.chunk = MODE ? p.tile2 : ST_BLOCK;
    const uint32_t lds = 8u * (3u * k.chunk + k.tile * k.words + (MODE ? k.chunk * k.words : 0u)) + 4u * k.tile;
    if (p.path == 1)
        hipLaunchKernelGGL(st_pairs_all<MODE>, dim3((k.N + k.tile - 1) / k.tile), dim3(ST_BLOCK), lds, st, k);
    else
        {
        const uint32_t grid = walk_launch_blocks(k.ncell, k.cells_per_block);
        hipLaunchKernelGGL(st_pairs_cells<MODE>, dim3(grid), dim3(ST_BLOCK), lds, st, k);
        }
    return hipGetLastError();
    }

} // namespace azp

extern "C" int azp_steinhardt_scratch_size(const azp_steinhardt_args* args, uint64_t* bytes)
    {
    using namespace azp;
    if (!bytes)
        return AZP_ERROR_INVALID_ARGUMENT;
    StPlan p;
    const int rc = st_plan(args, p);
    if (rc != AZP_SUCCESS)
        return rc;
    *bytes = p.bytes;
    return AZP_SUCCESS;
    }

extern "C" int azp_steinhardt_compute(const azp_steinhardt_args* args, void* stream)
    {
    using namespace azp;
    StPlan p;
    const int rc = st_plan(args, p);
    if (rc != AZP_SUCCESS)
        return rc;
    const bool avg = (args->flags & AZP_STEINHARDT_AVERAGE) != 0, conn = (args->flags & AZP_STEINHARDT_CONNECTIONS) != 0;
    if (!args->d_summary)
        return AZP_ERROR_INVALID_ARGUMENT;
    if (args->N && (!args->d_pos || !args->d_num_neighbors || !args->d_words || !args->d_order || (avg && !args->d_avg_words)
                    || (conn && !args->d_num_connections) || !args->d_scratch || args->scratch_bytes < p.bytes))
        return AZP_ERROR_INVALID_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(args->d_summary, 0, (uint64_t)st_summary_words(args) * sizeof(int64_t), st);
    if (e != hipSuccess || args->N == 0)
        return (int)e;
    char* base = static_cast<char*>(args->d_scratch);
    StKArgs k = {};
    k.pos = args->d_pos;
    k.mask = args->d_type_mask;
    k.N = args->N;
    k.ntypes = args->ntypes;
    k.box = make_box_dev(args->box);
    k.rmaxsq = args->r_max * args->r_max;
    k.terms = p.terms;
    k.words = p.terms.words;
    k.sorted = reinterpret_cast<double*>(base);
    k.S = reinterpret_cast<long long*>(base + p.off_S);
    k.nb = reinterpret_cast<uint32_t*>(base + p.off_nb);
    k.Q = reinterpret_cast<long long*>(base + p.off_Q);
    k.qhat = reinterpret_cast<double*>(base + p.off_qhat);
    k.q_threshold = args->q_threshold;
    k.solid_threshold = args->solid_threshold;
    k.flags = args->flags;
    k.num_bins = args->num_bins;
    k.out_nb = args->d_num_neighbors;
    k.out_words = reinterpret_cast<long long*>(args->d_words);
    k.out_order = args->d_order;
    k.out_avg_words = reinterpret_cast<long long*>(args->d_avg_words);
    k.out_ncon = args->d_num_connections;
    k.summary = reinterpret_cast<unsigned long long*>(args->d_summary);
    const dim3 per_row((args->N + ST_BLOCK - 1) / ST_BLOCK), block(ST_BLOCK);
    if (p.path == 1)
        {
        hipLaunchKernelGGL(st_rows_kernel, per_row, block, 0, st, k);
        if ((e = hipGetLastError()) != hipSuccess)
            return (int)e;
        }
    else
        {
        k.grid = p.grid;
        k.ncell = p.order.ncell;
        uint32_t* perm = walk_words(base, p.order.off_perm);
        k.perm = perm;
        k.start = walk_words(base, p.order.off_start);
        const StRowSink sink = {k.pos, k.mask, k.sorted, perm, k.ntypes};
        if ((e = walk_bin(args->N, k.pos, k.grid, base, p.order, k.sorted, sink, st)) != hipSuccess)
            return (int)e;
        }
    if ((e = st_launch_pairs<0>(p, k, st)) != hipSuccess)
        return (int)e;
    hipLaunchKernelGGL(st_finish_kernel, per_row, block, 0, st, k);
    if ((e = hipGetLastError()) != hipSuccess)
        return (int)e;
    if (avg)
        {
        if ((e = st_launch_pairs<1>(p, k, st)) != hipSuccess)
            return (int)e;
        hipLaunchKernelGGL(st_finish_avg_kernel, per_row, block, 0, st, k);
        if ((e = hipGetLastError()) != hipSuccess)
            return (int)e;
        }
    if (conn && (e = st_launch_pairs<2>(p, k, st)) != hipSuccess)
        return (int)e;
    const uint32_t lds = 4u * (args->n_terms * args->num_bins + AZP_STEINHARDT_CONNECTION_BINS);
    hipLaunchKernelGGL(st_summary_kernel, dim3(std::min<uint32_t>(per_row.x, 1024u)), block, lds, st, k);
    return (int)hipGetLastError();
    }
