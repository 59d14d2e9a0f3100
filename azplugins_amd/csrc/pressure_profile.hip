// pressure_profile.hip -- the configurational part of compute.PressureProfile: the Irving-Kirkwood contour stress along
// one Cartesian axis. Not part of the reference; the semantics are defined in include/azp.h ("pressure profile") and
// DESIGN 4.33. Every unordered pair (i, j) that a force acts on is taken once, from the side of the smaller tag:
// d = minimum image of r_i - r_j, rsq by walk_accept, force_divr from the force's own evaluator (evaluators.hpp), the
// six virial words w_ab = (force_divr d_a) d_b, spread over the bins that the segment from z1 = r_i[axis] to
// z0 = z1 - d[axis] crosses (pp_spread below: the one place where the weights are computed).
//
// Three kernels, the same integers wherever more than one is valid:
//   pp_all_pairs<P>  (any box) the tile of rdf_all_pairs: thread t holds row 256 blockIdx.x + t, the workgroup streams
//                    its segment of the rows through LDS in chunks of 256 (x, y, z, tag, type).
//   pp_cells<P>      (orthorhombic box, walk_make_grid) the walk of pair_walk.hpp; the scatter leaves (x, y, z, flags)
//                    and the per-slot extras (tag, type) in cell order.
//   pp_listed<P, BOND>  one lane per row over a per-particle table: the merged exclusion table (partners alone: the
//                    pair evaluator, sign -1, takes out exactly what the walk put in) or the bond / special-pair table
//                    (azp_bond_entry: the bond evaluator of the entry's type, sign +1).
// P is the evaluator policy: PPPair<E, XPLOR> keeps E::Coeff per type pair, PPBond<E> E::Params per group type, both
// in LDS behind the histogram.
//
// Accumulation is integer throughout: a term lambda_k w_ab is refused and counted if it is not finite or
// |term| >= max_term, else converted ONCE, q = round-to-nearest-even(term 2^shift), and added with a 64-bit integer
// atomic -- into the workgroup's row of 6 num_bins words in LDS where num_bins <= AZP_PRESSURE_PROFILE_LDS_BINS
// (48 KiB of the 64 KiB a workgroup has without opting in; the non-zero words go to the output row at the end), else
// straight into the output row. Sums modulo 2^64 do not depend on the order of the adds, and a term is a function of
// the unordered pair alone: a row is the same bits between two calls, between the paths and under any reordering of
// the rows that carries the tags. No floating-point atomics.
//
// LDS: 8 KiB of staging (3 x 256 doubles, 2 x 256 words) + 48 num_bins bytes of histogram (at most 48 KiB) + the
// coefficient table + 224 B of stencil table. Bytes: as rdf.hip, plus 8 B per staged candidate for the extras.
#include "evaluators.hpp"
#include "pair_walk.hpp"

namespace azp
{
constexpr uint32_t PP_BLOCK = WALK_BLOCK;
constexpr uint32_t PP_CHUNK = 256;
typedef unsigned long long pp_word;

struct PPKArgs
    {
    const double* pos;
    const uint32_t* tag;
    pp_word* out;
    BoxDev box;
    double rmaxsq;
    double lower, scale;    // bin coordinate s = (z - lower) * scale
    double two_shift;       // 2^shift
    double max_term;
    const double* rcutsq;
    const double* ronsq;
    uint32_t N, ntypes, n_coeff, shift_mode;
    uint32_t num_bins, axis, wrap, use_lds;
    int32_t sign;
    // cells path
    GridDev grid;
    uint32_t ncell;
    double* sorted;         // N x 4: x, y, z, flags
    uint2* extras;          // N: tag, type of the slot
    uint32_t* start;
    uint32_t cells_per_block;
    uint32_t seg_len;
    // listed pairs
    const void* table;
    const uint32_t* counts;
    uint64_t pitch;
    };

// what one thread counts; added to the summary words at the end (modulo 2^64: a pass with sign -1 counts down)
struct PPCount
    {
    pp_word pairs, terms, over;
    };

// ---------------------------------------------------------------------------------------------------------------
// evaluator policies
// ---------------------------------------------------------------------------------------------------------------
template<class E, bool XPLOR> struct PPPair
    {
    typedef typename E::Params Params;
    struct Coeff
        {
        typename E::Coeff c;
        double ronsq;
        };
    // as prepare_coeff of pair_kernel.hpp: the energy shift matters to the force under xplor alone
    static __device__ __forceinline__ Coeff prepare(const PPKArgs& a, const Params* params, uint32_t t)
        {
        const double rcutsq = a.rcutsq[t];
        bool energy_shift = (a.shift_mode == AZP_SHIFT_SHIFT);
        if (a.shift_mode == AZP_SHIFT_XPLOR && a.ronsq[t] > rcutsq)
            energy_shift = true;
        Coeff c;
        c.c = E::prepare(params[t], rcutsq, energy_shift);
        c.ronsq = XPLOR ? a.ronsq[t] : 0.0;
        return c;
        }
    static __device__ __forceinline__ bool eval(const Coeff& c, double rsq, double& force_divr)
        {
        double pair_eng;
        const bool evaluated = E::eval(c.c, rsq, force_divr, pair_eng);
        if (XPLOR && evaluated)
            apply_xplor(rsq, c.ronsq, c.c.rcutsq, force_divr, pair_eng);
        return evaluated;
        }
    };

template<class E> struct PPBond
    {
    typedef typename E::Params Params;
    typedef Params Coeff;
    static __device__ __forceinline__ Coeff prepare(const PPKArgs&, const Params* params, uint32_t t) { return params[t]; }
    static __device__ __forceinline__ bool eval(const Coeff& c, double rsq, double& force_divr)
        {
        double bond_eng;
        return E::eval(c, rsq, force_divr, bond_eng);
        }
    };

// ---------------------------------------------------------------------------------------------------------------
// spreading
// ---------------------------------------------------------------------------------------------------------------
// the six terms lambda * w of one bin k (already mapped into [0, num_bins))
__device__ __forceinline__ void pp_add(const PPKArgs& a, pp_word* hist, uint32_t k, double lambda, const double (&w)[6], PPCount& n)
    {
    const pp_word one = (pp_word)(long long)a.sign;
#pragma unroll
    for (int c = 0; c < 6; ++c)
        {
        const double t = lambda * w[c];
        if (fabs(t) < a.max_term) // (false for a NaN)
            {
            const long long q = __double2ll_rn(t * a.two_shift);
            const pp_word v = (pp_word)(a.sign > 0 ? q : -q);
            if (a.use_lds) // (uniform; two address spaces, two instructions)
                atomicAdd(&hist[6u * k + c], v);
            else
                atomicAdd(&a.out[6u * k + c], v);
            n.terms += one;
            }
        else
            n.over += one;
        }
    }

// The weights (include/azp.h states these expressions; tests/pressure_profile_ref.py follows them). No contraction:
// every operation below rounds once.
__device__ __forceinline__ void pp_spread(const PPKArgs& a, pp_word* hist, double z1, double daxis, const double (&w)[6], PPCount& n)
    {
#pragma clang fp contract(off)
    const double s1 = (z1 - a.lower) * a.scale;
    const double s0 = ((z1 - daxis) - a.lower) * a.scale;
    const double lo = fmin(s0, s1), hi = fmax(s0, s1);
    const double nb = (double)a.num_bins;
    if (!(fabs(lo) < 1.0e9 && fabs(hi) < 1.0e9))
        {
        n.over += (pp_word)(long long)(6 * a.sign); // (a coordinate that is not finite: no bin)
        return;
        }
    const double flo = floor(lo), fhi = floor(hi);
    double k0 = flo, k1 = fhi;
    if (!a.wrap)
        {
        k0 = fmax(k0, 0.0);
        k1 = fmin(k1, nb - 1.0);
        }
    const double len = hi - lo;
    for (double kf = k0; kf <= k1; kf += 1.0)
        {
        // (one bin: lambda = 1 whatever len is, d_axis = 0 included)
        const double lambda = (flo == fhi) ? 1.0 : (fmin(hi, kf + 1.0) - fmax(lo, kf)) / len;
        if (!(lambda > 0.0))
            continue;
        int k = (int)kf;
        if (a.wrap)
            {
            k %= (int)a.num_bins;
            if (k < 0)
                k += (int)a.num_bins;
            }
        pp_add(a, hist, (uint32_t)k, lambda, w, n);
        }
    }

// one pair from the side of its smaller tag: d = r_i - r_j before the minimum image
template<class P>
__device__ __forceinline__ void pp_pair(const PPKArgs& a, pp_word* hist, const typename P::Coeff& c, double z1, double dx, double dy,
                                        double dz, PPCount& n)
    {
    double rsq;
    if (!walk_accept(a.box, a.rmaxsq, dx, dy, dz, rsq))
        return;
    double force_divr;
    if (!P::eval(c, rsq, force_divr))
        return;
    n.pairs += (pp_word)(long long)a.sign;
    const double fx = force_divr * dx, fy = force_divr * dy, fz = force_divr * dz;
    const double w[6] = {fx * dx, fx * dy, fx * dz, fy * dy, fy * dz, fz * dz};
    pp_spread(a, hist, z1, a.axis == 0 ? dx : (a.axis == 1 ? dy : dz), w, n);
    }

__device__ __forceinline__ double pp_axis(const PPKArgs& a, double x, double y, double z) { return a.axis == 0 ? x : (a.axis == 1 ? y : z); }

// the dynamic LDS: the histogram (use_lds), then the coefficient table
template<class P>
__device__ __forceinline__ typename P::Coeff* pp_setup(const PPKArgs& a, const typename P::Params* params, pp_word* s_dyn)
    {
    const uint32_t words = a.use_lds ? 6u * a.num_bins : 0u;
    for (uint32_t k = threadIdx.x; k < words; k += PP_BLOCK)
        s_dyn[k] = 0;
    typename P::Coeff* s_coeff = reinterpret_cast<typename P::Coeff*>(s_dyn + words);
    for (uint32_t t = threadIdx.x; t < a.n_coeff; t += PP_BLOCK)
        s_coeff[t] = P::prepare(a, params, t);
    __syncthreads();
    return s_coeff;
    }

// the workgroup's histogram and counts into the output row
__device__ __forceinline__ void pp_finish(const PPKArgs& a, pp_word* hist, const PPCount& n)
    {
    __shared__ pp_word s_n[3];
    if (threadIdx.x < 3)
        s_n[threadIdx.x] = 0;
    __syncthreads();
    if (n.pairs) atomicAdd(&s_n[0], n.pairs);
    if (n.terms) atomicAdd(&s_n[1], n.terms);
    if (n.over) atomicAdd(&s_n[2], n.over);
    __syncthreads();
    if (threadIdx.x < 3 && s_n[threadIdx.x])
        atomicAdd(&a.out[6ull * a.num_bins + threadIdx.x], s_n[threadIdx.x]);
    if (a.use_lds)
        for (uint32_t k = threadIdx.x; k < 6u * a.num_bins; k += PP_BLOCK)
            {
            const pp_word v = hist[k];
            if (v)
                atomicAdd(&a.out[k], v);
            }
    }

// ---------------------------------------------------------------------------------------------------------------
// the walks
// ---------------------------------------------------------------------------------------------------------------
template<class P>
__global__ void __launch_bounds__(PP_BLOCK) pp_all_pairs(const PPKArgs a, const typename P::Params* __restrict__ params)
    {
    extern __shared__ __attribute__((aligned(16))) pp_word s_dyn[];
    __shared__ double s_x[PP_CHUNK], s_y[PP_CHUNK], s_z[PP_CHUNK];
    __shared__ uint32_t s_tag[PP_CHUNK], s_type[PP_CHUNK];
    const typename P::Coeff* s_coeff = pp_setup<P>(a, params, s_dyn);
    const uint32_t tid = threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * PP_BLOCK + tid;
    const bool row = i < a.N;
    double xi = 0.0, yi = 0.0, zi = 0.0;
    uint32_t tagi = 0xFFFFFFFFu, typei = 0;
    if (row)
        {
        const double4 p = load_scalar4(a.pos, (uint32_t)i);
        xi = p.x; yi = p.y; zi = p.z;
        typei = min((uint32_t)type_from_w(p.w), a.ntypes - 1u);
        tagi = a.tag[i];
        }
    const double z1 = pp_axis(a, xi, yi, zi);
    const uint64_t j0 = (uint64_t)blockIdx.y * a.seg_len;
    const uint64_t j1 = std::min<uint64_t>(j0 + a.seg_len, a.N);
    const double nan = __builtin_nan("");
    PPCount n = {0, 0, 0};
    for (uint64_t jb = j0; jb < j1; jb += PP_CHUNK)
        {
        const uint64_t j = jb + tid;
        double x = nan, y = nan, z = nan;
        uint32_t tg = 0, ty = 0;
        if (j < j1)
            {
            const double4 p = load_scalar4(a.pos, (uint32_t)j);
            x = p.x; y = p.y; z = p.z;
            ty = min((uint32_t)type_from_w(p.w), a.ntypes - 1u);
            tg = a.tag[j];
            }
        s_x[tid] = x; s_y[tid] = y; s_z[tid] = z; s_tag[tid] = tg; s_type[tid] = ty;
        __syncthreads();
        const uint32_t m = (uint32_t)std::min<uint64_t>(PP_CHUNK, j1 - jb);
        if (row)
            {
            for (uint32_t c = 0; c < m; ++c)
                if (tagi < s_tag[c])
                    pp_pair<P>(a, s_dyn, s_coeff[typei * a.ntypes + s_type[c]], z1, xi - s_x[c], yi - s_y[c], zi - s_z[c], n);
            }
        __syncthreads();
        }
    pp_finish(a, s_dyn, n);
    }

// what bin_particles' scatter leaves at a particle's slot of the cell order
struct PPRowSink
    {
    const double* pos;
    const uint32_t* tag;
    double* sorted;
    uint2* extras;
    uint32_t ntypes;
    __device__ void operator()(uint32_t slot, uint32_t p) const
        {
        const double4 r = load_scalar4(pos, p);
        store_scalar4(sorted, slot, r.x, r.y, r.z, walk_flags(true, true));
        extras[slot] = make_uint2(tag[p], min((uint32_t)type_from_w(r.w), ntypes - 1u));
        }
    };

template<class P>
__global__ void __launch_bounds__(PP_BLOCK) pp_cells(const PPKArgs a, const typename P::Params* __restrict__ params)
    {
    extern __shared__ __attribute__((aligned(16))) pp_word s_dyn[];
    __shared__ double s_x[PP_CHUNK], s_y[PP_CHUNK], s_z[PP_CHUNK];
    __shared__ uint32_t s_tag[PP_CHUNK], s_type[PP_CHUNK];
    __shared__ uint32_t s_seg_start[27], s_seg_end[28];  // s_seg_end[s + 1]: candidates in segments 0 .. s
    const typename P::Coeff* s_coeff = pp_setup<P>(a, params, s_dyn);
    const uint32_t tid = threadIdx.x;
    const uint32_t b = xcd_remap(blockIdx.x, gridDim.x);
    const uint64_t c0 = (uint64_t)b * a.cells_per_block;
    const uint32_t c1 = (uint32_t)std::min<uint64_t>(c0 + a.cells_per_block, a.ncell);
    const uint32_t dx = a.grid.dim[0], dy = a.grid.dim[1], dz = a.grid.dim[2];
    PPCount n = {0, 0, 0};
    // (the cell loop and stencil table of the walk: the same lines as in rdf_cells, st_pairs_cells and cl_union_cells,
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
        for (uint32_t rt = 0; rt < rn; rt += PP_BLOCK)
            {
            const uint32_t slot0 = rs + rt, T = min(PP_BLOCK, rn - rt);
            const TileLanes l = tile_lanes(T);
            double xi, yi, zi;
            const bool row = walk_row(a.sorted, slot0, T, l.r, xi, yi, zi);
            uint32_t tagi = 0xFFFFFFFFu, typei = 0;
            if (row)
                {
                const uint2 e = a.extras[slot0 + l.r];
                tagi = e.x; typei = e.y;
                }
            const double z1 = pp_axis(a, xi, yi, zi);
            for (uint32_t cb = 0; cb < M; cb += PP_CHUNK)
                {
                const uint32_t q = cb + tid;
                double3 p = walk_no_candidate();
                uint2 e = make_uint2(0u, 0u);
                if (q < M)
                    {
                    const uint32_t slot = walk_candidate_slot(q, s_seg_start, s_seg_end);
                    p = walk_candidate(a.sorted, slot);
                    e = a.extras[slot];
                    }
                s_x[tid] = p.x; s_y[tid] = p.y; s_z[tid] = p.z; s_tag[tid] = e.x; s_type[tid] = e.y;
                __syncthreads();
                const uint32_t m = min(PP_CHUNK, M - cb);
                if (row)
                    {
                    for (uint32_t cc = l.sub; cc < m; cc += l.G)
                        if (tagi < s_tag[cc])
                            pp_pair<P>(a, s_dyn, s_coeff[typei * a.ntypes + s_type[cc]], z1, xi - s_x[cc], yi - s_y[cc], zi - s_z[cc], n);
                    }
                __syncthreads();
                }
            }
        }
    pp_finish(a, s_dyn, n);
    }

// ---------------------------------------------------------------------------------------------------------------
// listed pairs
// ---------------------------------------------------------------------------------------------------------------
// One lane per row i < N (grid-stride) over the row's entries: entry s at s * pitch + i, a partner row (uint32: the
// exclusion table; the coefficients of the two particle types) or an azp_bond_entry (BOND: the parameters of the entry's
// type). A pair is taken from the row with the smaller tag; an entry that names a row >= N, the row itself or a type
// outside the table is skipped.
template<class P, bool BOND>
__global__ void __launch_bounds__(PP_BLOCK) pp_listed(const PPKArgs a, const typename P::Params* __restrict__ params)
    {
    extern __shared__ __attribute__((aligned(16))) pp_word s_dyn[];
    const typename P::Coeff* s_coeff = pp_setup<P>(a, params, s_dyn);
    PPCount n = {0, 0, 0};
    for (uint64_t i = (uint64_t)blockIdx.x * PP_BLOCK + threadIdx.x; i < a.N; i += (uint64_t)gridDim.x * PP_BLOCK)
        {
        const uint32_t cnt = a.counts[i];
        if (cnt == 0)
            continue;
        const double4 p = load_scalar4(a.pos, (uint32_t)i);
        const uint32_t tagi = a.tag[i];
        const uint32_t typei = min((uint32_t)type_from_w(p.w), a.ntypes - 1u);
        const double z1 = pp_axis(a, p.x, p.y, p.z);
        for (uint32_t s = 0; s < cnt; ++s)
            {
            uint32_t j, t;
            if (BOND)
                {
                const azp_bond_entry e = static_cast<const azp_bond_entry*>(a.table)[(uint64_t)s * a.pitch + i];
                j = e.idx; t = e.type;
                }
            else
                {
                j = static_cast<const uint32_t*>(a.table)[(uint64_t)s * a.pitch + i];
                t = 0;
                }
            if (j >= a.N || j == i || t >= a.n_coeff)
                continue;
            if (!(tagi < a.tag[j]))
                continue;
            const double4 q = load_scalar4(a.pos, j);
            if (!BOND)
                t = typei * a.ntypes + min((uint32_t)type_from_w(q.w), a.ntypes - 1u);
            pp_pair<P>(a, s_dyn, s_coeff[t], z1, p.x - q.x, p.y - q.y, p.z - q.z, n);
            }
        }
    __syncthreads();
    pp_finish(a, s_dyn, n);
    }

// the shift into the last summary word of a row that the memset has zeroed
__global__ void pp_begin(pp_word* out, uint32_t num_bins, uint32_t shift) { out[6ull * num_bins + 3] = shift; }

// ---------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------
struct PPPlan
    {
    int path;  // 1 all-pairs, 2 cells
    GridDev grid;
    CellOrder order;  // behind `sorted` and `extras`, which head the scratch
    uint64_t off_extras, bytes;
    };

static int pp_check(const azp_pressure_profile_args* a)
    {
    if (!a || a->axis > 2 || a->num_bins < 1 || a->num_bins > AZP_PRESSURE_PROFILE_MAX_BINS || !(a->scale > 0.0)
        || !std::isfinite(a->scale) || !std::isfinite(a->lower) || !(a->max_term > 0.0) || !std::isfinite(a->max_term)
        || a->shift > 52 || a->ntypes == 0)
        return AZP_ERROR_INVALID_ARGUMENT;
    for (int d = 0; d < 3; ++d)
        if (!(a->box.L[d] > 0.0))
            return AZP_ERROR_INVALID_ARGUMENT;
    return AZP_SUCCESS;
    }

static int pp_plan(const azp_pressure_profile_args* a, PPPlan& p)
    {
    const int rc = pp_check(a);
    if (rc != AZP_SUCCESS)
        return rc;
    if (!(a->r_max > 0.0) || !std::isfinite(a->r_max) || a->path > 2 || a->shift_mode > AZP_SHIFT_XPLOR)
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
    p.bytes = p.off_extras = 0;
    if (p.path == 2)
        {
        p.off_extras = walk_align((uint64_t)a->N * 32);
        p.order = walk_cell_order(p.off_extras + walk_align((uint64_t)a->N * 8), a->N, p.grid, false);
        p.bytes = p.order.bytes;
        }
    return AZP_SUCCESS;
    }

static PPKArgs pp_kernel_args(const azp_pressure_profile_args* args)
    {
    PPKArgs k = {};
    k.pos = args->d_pos;
    k.tag = args->d_tag;
    k.out = reinterpret_cast<pp_word*>(args->d_out);
    k.box = make_box_dev(args->box);
    k.rmaxsq = args->r_max * args->r_max;
    k.lower = args->lower;
    k.scale = args->scale;
    k.two_shift = std::ldexp(1.0, (int)args->shift);
    k.max_term = args->max_term;
    k.rcutsq = args->d_rcutsq;
    k.ronsq = args->d_ronsq;
    k.N = args->N;
    k.ntypes = args->ntypes;
    k.n_coeff = args->ntypes * args->ntypes;
    k.shift_mode = args->shift_mode;
    k.num_bins = args->num_bins;
    k.axis = args->axis;
    k.wrap = args->wrap ? 1u : 0u;
    k.use_lds = args->num_bins <= AZP_PRESSURE_PROFILE_LDS_BINS ? 1u : 0u;
    k.sign = 1;
    return k;
    }

template<class Coeff> static bool pp_lds_bytes(const PPKArgs& k, uint32_t& bytes)
    {
    const uint64_t b = (k.use_lds ? 48ull * k.num_bins : 0ull) + (uint64_t)sizeof(Coeff) * k.n_coeff;
    bytes = (uint32_t)b;
    return b <= 54ull * 1024;  // (beside the 8.3 KiB of static LDS: the 64 KiB a workgroup has without opting in)
    }

template<class P> static int pp_walk(const azp_pressure_profile_args* args, const typename P::Params* d_params, void* stream)
    {
    PPPlan p;
    const int rc = pp_plan(args, p);
    if (rc != AZP_SUCCESS)
        return rc;
    if (args->N == 0)
        return AZP_SUCCESS;
    if (!args->d_out || !args->d_pos || !args->d_tag || !d_params || !args->d_rcutsq
        || (args->shift_mode == AZP_SHIFT_XPLOR && !args->d_ronsq))
        return AZP_ERROR_INVALID_ARGUMENT;
    if (p.bytes && (!args->d_scratch || args->scratch_bytes < p.bytes))
        return AZP_ERROR_INVALID_ARGUMENT;
    PPKArgs k = pp_kernel_args(args);
    uint32_t lds;
    if (!pp_lds_bytes<typename P::Coeff>(k, lds))
        return AZP_ERROR_TOO_MANY_TYPES;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (p.path == 1)
        {
        const uint32_t n_tiles = (args->N + PP_BLOCK - 1) / PP_BLOCK;
        const uint32_t n_chunks = (uint32_t)(((uint64_t)args->N + PP_CHUNK - 1) / PP_CHUNK);
        uint32_t n_seg = std::min(n_chunks, std::max(1u, WALK_TARGET_BLOCKS / n_tiles));
        const uint32_t chunks_per_seg = (n_chunks + n_seg - 1) / n_seg;
        n_seg = (n_chunks + chunks_per_seg - 1) / chunks_per_seg;
        k.seg_len = chunks_per_seg * PP_CHUNK;
        hipLaunchKernelGGL(pp_all_pairs<P>, dim3(n_tiles, n_seg), dim3(PP_BLOCK), lds, st, k, d_params);
        return (int)hipGetLastError();
        }
    k.grid = p.grid;
    k.ncell = p.order.ncell;
    k.sorted = static_cast<double*>(args->d_scratch);
    k.extras = reinterpret_cast<uint2*>(static_cast<char*>(args->d_scratch) + p.off_extras);
    k.start = walk_words(args->d_scratch, p.order.off_start);
    const PPRowSink sink = {k.pos, k.tag, k.sorted, k.extras, k.ntypes};
    const hipError_t e = walk_bin(args->N, k.pos, k.grid, args->d_scratch, p.order, k.sorted, sink, st);
    if (e != hipSuccess)
        return (int)e;
    const uint32_t grid = walk_launch_blocks(k.ncell, k.cells_per_block);
    hipLaunchKernelGGL(pp_cells<P>, dim3(grid), dim3(PP_BLOCK), lds, st, k, d_params);
    return (int)hipGetLastError();
    }

template<class E> static int pp_walk_mode(const azp_pressure_profile_args* args, const typename E::Params* d_params, void* stream)
    {
    if (args && args->shift_mode == AZP_SHIFT_XPLOR)
        return pp_walk<PPPair<E, true>>(args, d_params, stream);
    return pp_walk<PPPair<E, false>>(args, d_params, stream);
    }

template<class P, bool BOND> static int pp_list(const azp_pressure_profile_list_args* x, const void* d_params, void* stream)
    {
    const azp_pressure_profile_args* args = &x->profile;
    if (args->N == 0)
        return AZP_SUCCESS;
    if (!args->d_out || !args->d_pos || !args->d_tag || !d_params || !x->d_table || !x->d_counts || x->pitch < args->N
        || (x->sign != 1 && x->sign != -1))
        return AZP_ERROR_INVALID_ARGUMENT;
    PPKArgs k = pp_kernel_args(args);
    if (BOND)
        {
        if (x->n_types == 0)
            return AZP_ERROR_INVALID_ARGUMENT;
        k.n_coeff = x->n_types;
        k.rmaxsq = INFINITY;  // (a bond has no cutoff of the walk: its evaluator decides)
        }
    else
        {
        if (!(args->r_max > 0.0) || !std::isfinite(args->r_max) || !args->d_rcutsq
            || (args->shift_mode == AZP_SHIFT_XPLOR && !args->d_ronsq) || args->shift_mode > AZP_SHIFT_XPLOR)
            return AZP_ERROR_INVALID_ARGUMENT;
        }
    k.sign = x->sign;
    k.table = x->d_table;
    k.counts = x->d_counts;
    k.pitch = x->pitch;
    uint32_t lds;
    if (!pp_lds_bytes<typename P::Coeff>(k, lds))
        return AZP_ERROR_TOO_MANY_TYPES;
    const uint32_t n_tiles = (args->N + PP_BLOCK - 1) / PP_BLOCK;
    hipLaunchKernelGGL((pp_listed<P, BOND>), dim3(std::min(n_tiles, WALK_TARGET_BLOCKS)), dim3(PP_BLOCK), lds,
                       static_cast<hipStream_t>(stream), k, static_cast<const typename P::Params*>(d_params));
    return (int)hipGetLastError();
    }

template<class E> static int pp_list_pair(const azp_pressure_profile_list_args* x, const void* d_params, void* stream)
    {
    if (x->profile.shift_mode == AZP_SHIFT_XPLOR)
        return pp_list<PPPair<E, true>, false>(x, d_params, stream);
    return pp_list<PPPair<E, false>, false>(x, d_params, stream);
    }
} // namespace azp

extern "C" int azp_pressure_profile_scratch_size(const azp_pressure_profile_args* args, uint64_t* bytes)
    {
    using namespace azp;
    if (!bytes)
        return AZP_ERROR_INVALID_ARGUMENT;
    PPPlan p;
    const int rc = pp_plan(args, p);
    if (rc != AZP_SUCCESS)
        return rc;
    *bytes = p.bytes;
    return AZP_SUCCESS;
    }

extern "C" int azp_pressure_profile_begin(const azp_pressure_profile_args* args, void* stream)
    {
    using namespace azp;
    const int rc = pp_check(args);
    if (rc != AZP_SUCCESS)
        return rc;
    if (!args->d_out)
        return AZP_ERROR_INVALID_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const hipError_t e = hipMemsetAsync(args->d_out, 0, (6ull * args->num_bins + 4) * sizeof(uint64_t), st);
    if (e != hipSuccess)
        return (int)e;
    hipLaunchKernelGGL(pp_begin, dim3(1), dim3(1), 0, st, reinterpret_cast<pp_word*>(args->d_out), args->num_bins, args->shift);
    return (int)hipGetLastError();
    }

extern "C" int azp_pressure_profile_pairs_perturbed_lennard_jones(const azp_pressure_profile_args* args, const azp_plj_params* d_params,
                                                                  void* stream)
    {
    return azp::pp_walk_mode<azp::EvalPLJ>(args, d_params, stream);
    }

extern "C" int azp_pressure_profile_pairs_hertz(const azp_pressure_profile_args* args, const azp_hertz_params* d_params, void* stream)
    {
    return azp::pp_walk_mode<azp::EvalHertz>(args, d_params, stream);
    }

extern "C" int azp_pressure_profile_pairs_expanded_yukawa(const azp_pressure_profile_args* args, const azp_yukawa_params* d_params,
                                                          void* stream)
    {
    return azp::pp_walk_mode<azp::EvalYukawa>(args, d_params, stream);
    }

extern "C" int azp_pressure_profile_pairs_colloid(const azp_pressure_profile_args* args, const azp_colloid_params* d_params, void* stream)
    {
    return azp::pp_walk_mode<azp::EvalColloid>(args, d_params, stream);
    }

extern "C" int azp_pressure_profile_pairs_dpd_conservative(const azp_pressure_profile_args* args, const azp_dpd_params* d_params,
                                                           void* stream)
    {
    if (args && args->shift_mode != AZP_SHIFT_NONE)
        return AZP_ERROR_INVALID_ARGUMENT;
    return azp::pp_walk<azp::PPPair<azp::EvalDPDConservative, false>>(args, d_params, stream);
    }

extern "C" int azp_pressure_profile_pairs_table(const azp_pressure_profile_args* args, const azp_table_params* d_params, void* stream)
    {
    if (args && args->shift_mode != AZP_SHIFT_NONE)
        return AZP_ERROR_INVALID_ARGUMENT;
    return azp::pp_walk<azp::PPPair<azp::EvalTable, false>>(args, d_params, stream);
    }

extern "C" int azp_pressure_profile_listed(const azp_pressure_profile_list_args* x, const void* d_params, void* stream)
    {
    using namespace azp;
    if (!x)
        return AZP_ERROR_INVALID_ARGUMENT;
    const int rc = pp_check(&x->profile);
    if (rc != AZP_SUCCESS)
        return rc;
    const bool plain = x->profile.shift_mode == AZP_SHIFT_NONE;
    switch (x->evaluator)
        {
    case AZP_PP_PERTURBED_LENNARD_JONES: return pp_list_pair<EvalPLJ>(x, d_params, stream);
    case AZP_PP_HERTZ: return pp_list_pair<EvalHertz>(x, d_params, stream);
    case AZP_PP_EXPANDED_YUKAWA: return pp_list_pair<EvalYukawa>(x, d_params, stream);
    case AZP_PP_COLLOID: return pp_list_pair<EvalColloid>(x, d_params, stream);
    case AZP_PP_DPD_CONSERVATIVE:
        return plain ? pp_list<PPPair<EvalDPDConservative, false>, false>(x, d_params, stream) : AZP_ERROR_INVALID_ARGUMENT;
    case AZP_PP_PAIR_TABLE:
        return plain ? pp_list<PPPair<EvalTable, false>, false>(x, d_params, stream) : AZP_ERROR_INVALID_ARGUMENT;
    case AZP_PP_BOND_DOUBLE_WELL: return pp_list<PPBond<EvalDoubleWell>, true>(x, d_params, stream);
    case AZP_PP_BOND_QUARTIC: return pp_list<PPBond<EvalQuartic>, true>(x, d_params, stream);
    case AZP_PP_BOND_TABLE: return pp_list<PPBond<EvalTable>, true>(x, d_params, stream);
    case AZP_PP_SPECIAL_PAIR_LJ: return pp_list<PPBond<EvalSpecialPairLJ>, true>(x, d_params, stream);
    default: return AZP_ERROR_INVALID_ARGUMENT;
        }
    }
