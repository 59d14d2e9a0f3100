// cluster.hip -- connected components behind compute.Cluster (include/azp.h "clusters"): the graph whose
// vertices are the rows of a group G and whose edges are the pairs closer than r_max, labelled by a concurrent
// union-find over the slots of the order the pair walk works in.
//
// The launches of one call, all on the caller's stream:
//   order    cells: walk_bin (pair_walk.hpp) into this call's scratch, its scatter leaves (x, y, z, flags) per slot
//            and the permutation slot -> row; all-pairs: the row order. Group and d_member are folded into the flag
//            here, so the pair walk never gathers. parent[slot] = slot, min_tag = NONE, size = 0.
//   union    the walk of pair_walk.hpp, the one the Steinhardt and RDF passes take: a tile of
//            T <= 256 rows contiguous in the order, against up to 27 contiguous candidate segments staged through LDS
//            in chunks of 256 (x, y, z as three double arrays and the candidate's slot). A pair is taken where
//            candidate slot < row slot: united once, counted once. Pairs inside the tile are united in an LDS
//            union-find over the tile's rows; a pair
//            with a candidate before the tile is united in global memory at once; when the candidates are through,
//            every row that is not the root of its LDS component is united with that root in global memory. (One
//            cell's 300 particles, 44,850 edges: 255 + 43 such unions and 44 x 256 finds that end on one word after
//            the first few, where 44,850 CAS chains would run without the LDS step.)
//   flatten  a later launch, so everything the union pass wrote is visible to plain loads: root[slot] = find(slot),
//            then per wave and distinct root one atomicMin of the smallest tag and one atomicAdd of the number of its
//            lanes at the root (32-bit integer atomics).
//   relabel  cluster_key / cluster_size of the row of each slot, through the permutation; where the caller asks for it
//            also cluster_rep, the row of the slot's root (what cluster_properties.hip indexes its table by).
//   summary  over the roots of G: counts, sum of squares and histogram through LDS into the row with 64-bit integer
//            atomics; the largest cluster as one 64-bit atomicMax of size << 32 | ~key in the scratch head.
//   finish   one thread unpacks that maximum into words [2] and [3] (-1 for an empty G). (An atomicMax cannot leave two
//            separate words, and a "last workgroup done" step inside the summary kernel would need the cross-workgroup
//            hand-off this file avoids: the unpacking is a launch of its own.)
//
// The union-find. parent[] holds slots, parent[x] <= x always: a root r has parent[r] == r, and the only way a root
// stops being one is a compare-and-swap parent[hi]: hi -> lo with lo < hi. find walks strictly downward, so it ends
// whatever it reads; path halving stores an ancestor (which stays an ancestor for good) over a non-root's parent.
// Visibility: other workgroups write parent[] during the union launch, so every access to it there is an agent-scope
// relaxed atomic (load, compare-exchange, store), never a plain load. A stale value is an older ancestor: harmless. A
// compare-and-swap on a root that has been hooked meanwhile fails and returns the new parent, from which the loop goes
// on. No lane waits for a value that another workgroup has yet to write: every loop makes its own progress (find
// descends; a failed CAS means another hook succeeded, and there are at most N - 1 hooks). No flag, no ticket, no
// persistent workgroup. The LDS union-find is the same code at workgroup scope.
// What the call outputs is a function of the graph and the tags alone: the components do not depend on the order of the
// unions, the key is the smallest tag, sizes and counts are integers.
#include "pair_walk.hpp"

namespace azp
{
constexpr uint32_t CL_BLOCK = WALK_BLOCK;    // threads, rows per tile and candidates per chunk
constexpr uint32_t CL_HEAD_BYTES = 256;      // the packed maximum, zeroed per call
constexpr uint32_t CL_LDS_BYTES = 3u * CL_BLOCK * 8u + 2u * CL_BLOCK * 4u;

struct ClKArgs
    {
    const double* pos;
    const uint8_t* mask;
    const uint32_t* member;
    const uint32_t* tag;
    uint32_t N, ntypes, member_min, size_bins;
    BoxDev box;
    double rmaxsq;
    // the order the passes work in
    double* sorted;            // N x 4: x, y, z, flag (1.0: in G, else 0.0; rows and candidates are the same set, so
                               // this kernel keeps its one-value flag and not the two-bit word of pair_walk.hpp)
    const uint32_t* perm;      // slot -> row, NULL: the row order itself
    GridDev grid;
    uint32_t ncell, cells_per_block;
    const uint32_t* start;     // ncell + 1
    // per slot
    uint32_t* parent;
    uint32_t* root;            // AZP_CLUSTER_NONE outside G
    uint32_t* min_tag;
    uint32_t* size;
    unsigned long long* best;  // size << 32 | ~key of the largest cluster
    // per row
    uint32_t* out_key;
    uint32_t* out_size;
    uint32_t* out_rep;         // may be NULL: the row of the root slot
    unsigned long long* summary;
    };

__device__ __forceinline__ bool cl_in_group(const ClKArgs& a, uint32_t p, double w)
    {
    return type_in_mask(a.mask, a.ntypes, w) && (!a.member || a.member[p] >= a.member_min);
    }

__device__ __forceinline__ void cl_init_slot(const ClKArgs& a, uint32_t slot, uint32_t p)
    {
    const double4 r = load_scalar4(a.pos, p);
    store_scalar4(a.sorted, slot, r.x, r.y, r.z, cl_in_group(a, p, r.w) ? 1.0 : 0.0);
    a.parent[slot] = slot;
    a.min_tag[slot] = AZP_CLUSTER_NONE;
    a.size[slot] = 0;
    }

// the slots in row order (the all-pairs path)
__global__ void __launch_bounds__(CL_BLOCK) cl_rows_kernel(const ClKArgs a)
    {
    const uint32_t p = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (p < a.N)
        cl_init_slot(a, p, p);
    }

// the slots in cell order: what bin_particles' scatter leaves at a particle's slot
struct ClRowSink
    {
    ClKArgs a;
    uint32_t* perm;
    __device__ void operator()(uint32_t slot, uint32_t p) const
        {
        cl_init_slot(a, slot, p);
        perm[slot] = p;
        }
    };

// ---------------------------------------------------------------------------------------------------------------
// union-find: SCOPE = __HIP_MEMORY_SCOPE_AGENT on global memory, __HIP_MEMORY_SCOPE_WORKGROUP on a tile's LDS
// ---------------------------------------------------------------------------------------------------------------
// the root above x, whose parent p the caller has loaded
template<int SCOPE> __device__ __forceinline__ uint32_t uf_find(uint32_t* parent, uint32_t x, uint32_t p)
    {
    while (p != x)
        {
        const uint32_t g = __hip_atomic_load(parent + p, __ATOMIC_RELAXED, SCOPE);
        if (g != p)
            __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, SCOPE);  // path halving: x is no root, g an ancestor
        x = p;
        p = g;
        }
    return x;
    }

// Unites the sets of a and b and returns the root they share at that moment (an ancestor of both from then on).
template<int SCOPE> __device__ __forceinline__ uint32_t uf_unite(uint32_t* parent, uint32_t a, uint32_t b)
    {
    for (;;)
        {
        // (both first loads in flight together: the two walks are independent)
        const uint32_t pa = __hip_atomic_load(parent + a, __ATOMIC_RELAXED, SCOPE);
        const uint32_t pb = __hip_atomic_load(parent + b, __ATOMIC_RELAXED, SCOPE);
        a = uf_find<SCOPE>(parent, a, pa);
        b = uf_find<SCOPE>(parent, b, pb);
        if (a == b)
            return a;
        const uint32_t hi = max(a, b), lo = min(a, b);
        uint32_t seen = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, SCOPE))
            return lo;
        a = seen;  // (hi was hooked by another lane meanwhile: go on from its new parent)
        b = lo;
        }
    }

// One tile: rows [slot0, slot0 + T) against the M candidates of the segment table. Called by every thread of the
// workgroup with the same arguments; `edges` is the calling thread's count of the pairs it took.
__device__ __forceinline__ void cl_tile(const ClKArgs& a, uint32_t slot0, uint32_t T, uint32_t M, const uint32_t* s_seg_start,
                                        const uint32_t* s_seg_end, unsigned long long& edges)
    {
    extern __shared__ double cl_lds[];
    constexpr uint32_t C = CL_BLOCK;
    const uint32_t tid = threadIdx.x;
    double* s_x = cl_lds;
    double* s_y = s_x + C;
    double* s_z = s_y + C;
    uint32_t* s_slot = reinterpret_cast<uint32_t*>(s_z + C);  // the staged candidates' slots
    uint32_t* s_par = s_slot + C;                             // the tile's own union-find, over its rows
    s_par[tid] = tid;
    const TileLanes l = tile_lanes(T);
    const uint32_t r = l.r;
    bool row = false;
    double xi = 0.0, yi = 0.0, zi = 0.0;
    if (r < T)
        {
        const double4 p = load_scalar4(a.sorted, slot0 + r);
        xi = p.x; yi = p.y; zi = p.z;
        row = p.w != 0.0;
        }
    const uint32_t rslot = slot0 + r;
    uint32_t above = rslot;
    const double nan = __builtin_nan("");
    if (__syncthreads_or(row))  // (the barrier also orders s_par's initial values before the first LDS union)
        {
        for (uint32_t cb = 0; cb < M; cb += C)
            {
            const uint32_t q = cb + tid;
            double x = nan, y = nan, z = nan;
            uint32_t slot = 0;
            if (q < M)
                {
                slot = walk_candidate_slot(q, s_seg_start, s_seg_end);
                const double4 p = load_scalar4(a.sorted, slot);
                if (p.w != 0.0)
                    {
                    x = p.x; y = p.y; z = p.z;
                    }
                }
            s_x[tid] = x; s_y[tid] = y; s_z[tid] = z;
            s_slot[tid] = slot;
            __syncthreads();
            const uint32_t n = min(C, M - cb);
            if (row)
                {
                for (uint32_t cc = l.sub; cc < n; cc += l.G)
                    {
                    double dx = xi - s_x[cc], dy = yi - s_y[cc], dz = zi - s_z[cc], rsq;
                    if (!walk_accept(a.box, a.rmaxsq, dx, dy, dz, rsq))
                        continue;
                    const uint32_t cs = s_slot[cc];
                    if (cs >= rslot)  // (the row itself, and the pair that the other row takes)
                        continue;
                    ++edges;
                    if (cs >= slot0)
                        uf_unite<__HIP_MEMORY_SCOPE_WORKGROUP>(s_par, r, cs - slot0);
                    else  // (from the last root this lane saw above its row: an ancestor for good, usually still the root)
                        above = uf_unite<__HIP_MEMORY_SCOPE_AGENT>(a.parent, above, cs);
                    }
                }
            __syncthreads();
            }
        // one representative per LDS component: every other row joins it in global memory
        if (tid < T)
            {
            uint32_t x = tid, p;
            while ((p = s_par[x]) != x)
                x = p;
            if (x != tid)
                uf_unite<__HIP_MEMORY_SCOPE_AGENT>(a.parent, slot0 + tid, slot0 + x);
            }
        }
    __syncthreads();
    }

__device__ __forceinline__ void cl_store_edges(const ClKArgs& a, unsigned long long edges, unsigned long long* s_edges)
    {
    if (edges)
        atomicAdd(s_edges, edges);
    __syncthreads();
    if (threadIdx.x == 0 && *s_edges)
        atomicAdd(&a.summary[5], *s_edges);
    }

__global__ void __launch_bounds__(CL_BLOCK) cl_union_all(const ClKArgs a)
    {
    __shared__ uint32_t s_seg_start[1], s_seg_end[2];
    __shared__ unsigned long long s_edges;
    if (threadIdx.x == 0)
        {
        s_seg_start[0] = 0;
        s_seg_end[0] = 0;
        s_edges = 0;
        }
    const uint32_t slot0 = blockIdx.x * CL_BLOCK;  // (the grid is ceil(N / 256): slot0 < N)
    const uint32_t T = min(CL_BLOCK, a.N - slot0);
    // (a candidate behind the tile's last row never has slot < row slot: the list ends with the tile)
    if (threadIdx.x == 0)
        s_seg_end[1] = slot0 + T;
    __syncthreads();
    unsigned long long edges = 0;
    cl_tile(a, slot0, T, slot0 + T, s_seg_start, s_seg_end, edges);
    cl_store_edges(a, edges, &s_edges);
    }

__global__ void __launch_bounds__(CL_BLOCK) cl_union_cells(const ClKArgs a)
    {
    __shared__ uint32_t s_seg_start[27], s_seg_end[28];  // s_seg_end[s + 1]: candidates in segments 0 .. s
    __shared__ unsigned long long s_edges;
    const uint32_t tid = threadIdx.x;
    if (tid == 0)
        s_edges = 0;
    const uint32_t b = xcd_remap(blockIdx.x, gridDim.x);
    const uint64_t c0 = (uint64_t)b * a.cells_per_block;
    const uint32_t c1 = (uint32_t)std::min<uint64_t>(c0 + a.cells_per_block, a.ncell);
    const uint32_t dx = a.grid.dim[0], dy = a.grid.dim[1], dz = a.grid.dim[2];
    unsigned long long edges = 0;
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
        for (uint32_t rt = 0; rt < rn; rt += CL_BLOCK)
            cl_tile(a, rs + rt, min(CL_BLOCK, rn - rt), M, s_seg_start, s_seg_end, edges);
        }
    cl_store_edges(a, edges, &s_edges);
    }

// root[slot] by plain loads (the union launch is over), the root's smallest tag and its size
__global__ void __launch_bounds__(CL_BLOCK) cl_flatten_kernel(const ClKArgs a)
    {
    const uint32_t s = blockIdx.x * CL_BLOCK + threadIdx.x;
    const bool active = s < a.N && a.sorted[4ull * s + 3] != 0.0;
    uint32_t x = AZP_CLUSTER_NONE, tag = AZP_CLUSTER_NONE;
    if (active)
        {
        uint32_t p;
        x = s;
        while ((p = a.parent[x]) != x)
            x = p;
        tag = a.tag[a.perm ? a.perm[s] : s];
        }
    if (s < a.N)
        a.root[s] = x;
    // Lanes of a wave that found the same root send ONE atomicMin and ONE atomicAdd (neighbours in the cell order mostly
    // share their cluster; with one atomic per lane a cluster of all 2^20 particles serialised 2^21 atomics on two words:
    // 12.2 ms of a 15.2 ms call, profiles/cluster.md).
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long todo = __ballot(active);
    while (todo)
        {
        const int leader = __builtin_ctzll(todo);
        const uint32_t r0 = (uint32_t)__shfl((int)x, leader, 64);
        const bool mine = active && x == r0;
        const unsigned long long same = __ballot(mine) & todo;
        uint32_t t = mine ? tag : AZP_CLUSTER_NONE;
#pragma unroll
        for (int o = 32; o; o >>= 1)
            t = min(t, (uint32_t)__shfl_xor((int)t, o, 64));
        if ((int)lane == leader)
            {
            atomicMin(&a.min_tag[r0], t);
            atomicAdd(&a.size[r0], (uint32_t)__popcll(same));
            }
        todo &= ~same;
        }
    }

__global__ void __launch_bounds__(CL_BLOCK) cl_relabel_kernel(const ClKArgs a)
    {
    const uint32_t s = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (s >= a.N)
        return;
    const uint32_t p = a.perm ? a.perm[s] : s;
    const uint32_t root = a.root[s];
    const bool in = root != AZP_CLUSTER_NONE;
    a.out_key[p] = in ? a.min_tag[root] : AZP_CLUSTER_NONE;
    a.out_size[p] = in ? a.size[root] : 0u;
    if (a.out_rep)  // (azp_cluster_properties needs a row per cluster: tags are not bounded by N, rows are)
        a.out_rep[p] = in ? (a.perm ? a.perm[root] : root) : AZP_CLUSTER_NONE;
    }

// the summary row from the roots: the workgroup's counts in LDS first (integer LDS atomics), then its non-zero words
// into the row with 64-bit integer atomics
__global__ void __launch_bounds__(CL_BLOCK) cl_summary_kernel(const ClKArgs a)
    {
    extern __shared__ double cl_lds[];
    uint32_t* s_hist = reinterpret_cast<uint32_t*>(cl_lds);  // size_bins
    __shared__ unsigned long long s_head[4];                 // N_G, clusters, sum of size^2, the packed maximum
    const uint32_t tid = threadIdx.x;
    for (uint32_t k = tid; k < a.size_bins; k += CL_BLOCK)
        s_hist[k] = 0;
    if (tid < 4)
        s_head[tid] = 0;
    __syncthreads();
    unsigned long long n_g = 0, n_cl = 0, sumsq = 0, best = 0;
    for (uint64_t s = (uint64_t)blockIdx.x * CL_BLOCK + tid; s < a.N; s += (uint64_t)gridDim.x * CL_BLOCK)
        {
        const uint32_t root = a.root[s];
        if (root == AZP_CLUSTER_NONE)
            continue;
        n_g += 1;
        if (root != (uint32_t)s)
            continue;
        const unsigned long long sz = a.size[s];
        n_cl += 1;
        sumsq += sz * sz;
        best = max(best, (sz << 32) | (unsigned long long)(~a.min_tag[s]));
        atomicAdd(&s_hist[min((uint32_t)sz, a.size_bins) - 1u], 1u);  // (sz >= 1: the root itself)
        }
    if (n_g)
        atomicAdd(&s_head[0], n_g);
    if (n_cl)
        {
        atomicAdd(&s_head[1], n_cl);
        atomicAdd(&s_head[2], sumsq);
        atomicMax(&s_head[3], best);
        }
    __syncthreads();
    if (tid < 3 && s_head[tid])
        atomicAdd(&a.summary[tid == 2 ? 4 : tid], s_head[tid]);
    if (tid == 3 && s_head[3])
        atomicMax(a.best, s_head[3]);
    for (uint32_t k = tid; k < a.size_bins; k += CL_BLOCK)
        if (s_hist[k])
            atomicAdd(&a.summary[6 + k], (unsigned long long)s_hist[k]);
    }

// words [2] and [3] from the packed maximum (best == NULL: no particles at all)
__global__ void cl_finish_kernel(const unsigned long long* best, long long* summary)
    {
    const unsigned long long b = best ? *best : 0ull;
    const bool any = summary[0] != 0;
    summary[2] = any ? (long long)(b >> 32) : 0;
    summary[3] = any ? (long long)(uint32_t)~(uint32_t)b : -1;
    }

// ---------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------
struct ClPlan
    {
    int path;  // 1 all-pairs, 2 cells
    GridDev grid;
    CellOrder order;  // path 2: behind the per-slot arrays
    uint64_t off_sorted, off_parent, off_root, off_min_tag, off_size, bytes;
    };

static int cl_plan(const azp_cluster_args* a, ClPlan& p)
    {
    if (!a || !(a->r_max > 0.0) || !std::isfinite(a->r_max) || a->path > 2 || a->stages > 2 || a->N > AZP_CLUSTER_MAX_N
        || a->size_bins < 1 || a->size_bins > AZP_CLUSTER_MAX_BINS)
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
    const uint64_t n = a->N, words = walk_align(n * 4);
    p.off_sorted = CL_HEAD_BYTES;
    p.off_parent = p.off_sorted + walk_align(n * 32);
    p.off_root = p.off_parent + words;
    p.off_min_tag = p.off_root + words;
    p.off_size = p.off_min_tag + words;
    p.bytes = p.off_size + words;
    if (p.path == 2)
        {
        p.order = walk_cell_order(p.bytes, n, p.grid, true);
        p.bytes = p.order.bytes;
        }
    return AZP_SUCCESS;
    }

} // namespace azp

extern "C" int azp_cluster_scratch_size(const azp_cluster_args* args, uint64_t* bytes)
    {
    using namespace azp;
    if (!bytes)
        return AZP_ERROR_INVALID_ARGUMENT;
    ClPlan p;
    const int rc = cl_plan(args, p);
    if (rc != AZP_SUCCESS)
        return rc;
    *bytes = p.bytes;
    return AZP_SUCCESS;
    }

extern "C" int azp_cluster_compute(const azp_cluster_args* args, void* stream)
    {
    using namespace azp;
    ClPlan p;
    const int rc = cl_plan(args, p);
    if (rc != AZP_SUCCESS)
        return rc;
    if (!args->d_summary)
        return AZP_ERROR_INVALID_ARGUMENT;
    if (args->N && (!args->d_pos || !args->d_tag || !args->d_cluster_key || !args->d_cluster_size || !args->d_scratch
                    || args->scratch_bytes < p.bytes))
        return AZP_ERROR_INVALID_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    long long* summary = reinterpret_cast<long long*>(args->d_summary);
    hipError_t e = hipMemsetAsync(summary, 0, (6ull + args->size_bins) * sizeof(int64_t), st);
    if (e != hipSuccess)
        return (int)e;
    if (args->N == 0)
        {
        hipLaunchKernelGGL(cl_finish_kernel, dim3(1), dim3(1), 0, st, (const unsigned long long*)nullptr, summary);
        return (int)hipGetLastError();
        }
    char* base = static_cast<char*>(args->d_scratch);
    if ((e = hipMemsetAsync(base, 0, CL_HEAD_BYTES, st)) != hipSuccess)
        return (int)e;
    ClKArgs k = {};
    k.pos = args->d_pos;
    k.mask = args->d_type_mask;
    k.member = args->d_member;
    k.tag = args->d_tag;
    k.N = args->N;
    k.ntypes = args->ntypes;
    k.member_min = args->member_min;
    k.size_bins = args->size_bins;
    k.box = make_box_dev(args->box);
    k.rmaxsq = args->r_max * args->r_max;
    k.best = reinterpret_cast<unsigned long long*>(base);
    k.sorted = reinterpret_cast<double*>(base + p.off_sorted);
    k.parent = reinterpret_cast<uint32_t*>(base + p.off_parent);
    k.root = reinterpret_cast<uint32_t*>(base + p.off_root);
    k.min_tag = reinterpret_cast<uint32_t*>(base + p.off_min_tag);
    k.size = reinterpret_cast<uint32_t*>(base + p.off_size);
    k.out_key = args->d_cluster_key;
    k.out_size = args->d_cluster_size;
    k.out_rep = args->d_cluster_rep;
    k.summary = reinterpret_cast<unsigned long long*>(args->d_summary);
    const dim3 per_row((args->N + CL_BLOCK - 1) / CL_BLOCK), block(CL_BLOCK);
    if (p.path == 1)
        {
        hipLaunchKernelGGL(cl_rows_kernel, per_row, block, 0, st, k);
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
        const ClRowSink sink = {k, perm};
        if ((e = walk_bin(args->N, k.pos, k.grid, base, p.order, k.sorted, sink, st)) != hipSuccess)
            return (int)e;
        }
    if (args->stages == 1)
        return AZP_SUCCESS;
    if (p.path == 1)
        hipLaunchKernelGGL(cl_union_all, per_row, block, CL_LDS_BYTES, st, k);
    else
        {
        const uint32_t grid = walk_launch_blocks(k.ncell, k.cells_per_block);
        hipLaunchKernelGGL(cl_union_cells, dim3(grid), block, CL_LDS_BYTES, st, k);
        }
    if ((e = hipGetLastError()) != hipSuccess || args->stages == 2)
        return (int)e;
    hipLaunchKernelGGL(cl_flatten_kernel, per_row, block, 0, st, k);
    if ((e = hipGetLastError()) != hipSuccess)
        return (int)e;
    hipLaunchKernelGGL(cl_relabel_kernel, per_row, block, 0, st, k);
    if ((e = hipGetLastError()) != hipSuccess)
        return (int)e;
    hipLaunchKernelGGL(cl_summary_kernel, dim3(std::min<uint32_t>(per_row.x, 1024u)), block, 4u * args->size_bins, st, k);
    if ((e = hipGetLastError()) != hipSuccess)
        return (int)e;
    hipLaunchKernelGGL(cl_finish_kernel, dim3(1), dim3(1), 0, st, (const unsigned long long*)k.best, summary);
    return (int)hipGetLastError();
    }
