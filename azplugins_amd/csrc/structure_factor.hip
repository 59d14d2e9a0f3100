// structure_factor.hip -- the density Fourier amplitudes behind compute.StructureFactor: for two groups A and B (per-type
// byte masks, NULL = every particle) and n_vectors integer triples m = (h, k, l),
//   rho_G(m) = sum over rows j < N of group G of exp(-2 pi i m . f_j),
// f_j = fractional() of cell_bin.hpp (the coordinates along the lattice vectors, [-0.5, 0.5) for a wrapped particle), so
// m . f = q(m) . r / 2 pi for q(m) = 2 pi H^-T m. The output row is 4 n_vectors + 4 doubles: Re rho_A, Im rho_A, Re rho_B,
// Im rho_B (n_vectors each), then N_A, N_B, N_(A and B), 0. Ghost rows (>= N) are never read.
//
// One lane owns one wavevector. Grid (ceil(n_vectors / 256), n_chunks): a workgroup takes the particles of its chunk
// 256 at a time (a STAGE): thread t loads particle base + t, computes its f and its group flags and leaves them in LDS;
// then every lane walks the staged particles in order, all lanes reading the same particle (one LDS address per wave: a
// broadcast read, no bank conflict). A particle in neither group is skipped by the whole wave (the flag is uniform).
//   path 1 (direct)  t = h f_x + k f_y + l f_z (FMA-contracted, left to right), sincospi(2 t): the term is (c, -s).
//   path 2 (powers)  a stage is walked in sub-stages of SF_SUB = 32 particles. Ahead of each, thread (axis, p) of the
//                    first 96 builds the powers e_axis^n, 0 <= n <= m_max[axis], of the base phasor
//                    e = exp(-2 pi i f_axis) = (c, -s) of sincospi(2 f_axis): e^0 = 1, e^n = e^(n-1) e by complex
//                    multiplication (two products, one of them an FMA, per component). The table of a particle is one
//                    row of ne = Hx + Hy + Hz + 3 entries (made odd) of 16 B: x powers, y powers, z powers; a lane reads
//                    the entry of |h| and flips the sign of its imaginary part where h < 0 (e^-n = conj(e^n): one XOR
//                    with a mask the lane keeps; storing the negative powers too would double the LDS and halve the
//                    workgroups per CU). The term is (e_x^h e_y^k) e_z^l. In the (l, k, h) order of the vector list the
//                    lanes of a wave read consecutive (or, across h = 0, equal) 16-byte entries of the x powers and a
//                    handful of adjacent entries of the y and z powers (distinct banks or a broadcast). The tables of
//                    a sub-stage have to fit AZP_SF_POWERS_LDS_BYTES; where they do not, the path does not exist.
// Both paths make the same additions in the same order.
//
// Order of summation (no floating-point atomics; two calls on one state give the same bits), with
// (stages, n_chunks) = sf_shape(N, n_vectors):
//   per lane     a stage accumulator starts at +0.0 and takes the terms of the stage's particles in row order (at most
//                256 additions); it is then added to the lane's chunk accumulator, which starts at +0.0 (at most `stages`
//                additions). The chunk accumulator goes to scratch[(slot * n_vectors + v) * n_chunks + chunk].
//   sf_fold      one wave per (slot, vector): fold_partials of azp_reduce.hpp over the n_chunks partials (lane l adds
//                the partials l, l + 64, ... in turn from +0.0, then the butterfly).
//   sf_shape     target = clamp(4096 / ceil(n_vectors / 256), 16, 512) chunks; stages = max(1, ceil(ceil(N / 256) /
//                target)); n_chunks = max(1, ceil(ceil(N / 256) / stages)) <= target.
// Addition depth D = 256 + stages + ceil(n_chunks / 64) + 6. N = 2^20 with up to 2,048 vectors: stages = 8, n_chunks =
// 512, D = 278; with 65,536 vectors: stages = 256, n_chunks = 16, D = 519.
// The group sizes are counted as integers (LDS integer atomics per workgroup of the first vector block), leave as
// doubles in three more rows of partials and go through the same fold: sums of integers below 2^53 are exact.
#include <algorithm>
#include <cmath>

#include "azp_reduce.hpp"
#include "cell_bin.hpp"
#include "sf_shape.hpp"

namespace azp
{
// (SF_BLOCK, the chunk targets and sf_shape: sf_shape.hpp, shared with displacement.hip)
constexpr uint32_t SF_SUB = 32;             // particles per table sub-stage of the powers path
// path 0: the powers path wherever its tables fit (profiles/structure_factor.md)
constexpr bool SF_AUTO_TAKES_POWERS = true;

struct SfKArgs
    {
    const double* pos;
    const uint8_t* mask_a;
    const uint8_t* mask_b;
    const int32_t* vectors;
    double* scratch;
    FracDev frac;
    uint32_t N, ntypes, n_vectors, stages, n_chunks;
    int32_t H[3];   // powers path: the bound of |h|, |k|, |l|
    uint32_t ne;    // powers path: entries of one particle's table row
    };

__device__ __forceinline__ double2 sf_cmul(const double2& a, const double2& b)
    {
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
    }

// conj(a) where sign is the sign bit, a where it is 0
__device__ __forceinline__ double2 sf_conj_if(const double2& a, int sign)
    {
    return make_double2(a.x, __hiloint2double(__double2hiint(a.y) ^ sign, __double2loint(a.y)));
    }

// NS = 2: A and B are the same group (slots Re A, Im A); NS = 4: slots Re A, Im A, Re B, Im B
template<uint32_t NS, bool POWERS> __global__ void __launch_bounds__(SF_BLOCK) sf_partial(const SfKArgs a)
    {
    __shared__ double s_fx[SF_BLOCK], s_fy[SF_BLOCK], s_fz[SF_BLOCK];
    __shared__ uint32_t s_flag[SF_BLOCK];
    __shared__ uint32_t s_count[3];
    extern __shared__ double2 s_tab[];  // powers path: SF_SUB rows of ne entries
    const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1);
    const uint32_t v = blockIdx.x * SF_BLOCK + tid;
    const uint32_t chunk = blockIdx.y;
    int32_t h = 0, k = 0, l = 0;
    if (v < a.n_vectors)
        {
        h = a.vectors[3ull * v];
        k = a.vectors[3ull * v + 1];
        l = a.vectors[3ull * v + 2];
        }
    const double dh = (double)h, dk = (double)k, dl = (double)l;
    uint32_t ix = 0, iy = 0, iz = 0;
    int sx = 0, sy = 0, sz = 0;  // the sign bit of the imaginary part where the index is negative
    if (POWERS)
        {
        // (an index beyond the stated bound would leave the table: clamped, the caller's bound is part of the contract)
        ix = (uint32_t)min(abs(h), a.H[0]);
        iy = (uint32_t)min(abs(k), a.H[1]) + (uint32_t)a.H[0] + 1u;
        iz = (uint32_t)min(abs(l), a.H[2]) + (uint32_t)(a.H[0] + a.H[1]) + 2u;
        sx = h < 0 ? (int)0x80000000 : 0;
        sy = k < 0 ? (int)0x80000000 : 0;
        sz = l < 0 ? (int)0x80000000 : 0;
        }
    if (tid < 3)
        s_count[tid] = 0;
    double acc[NS];
#pragma unroll
    for (uint32_t s = 0; s < NS; ++s)
        acc[s] = 0.0;
    uint32_t n_a = 0, n_b = 0, n_ab = 0;
    for (uint32_t stage = 0; stage < a.stages; ++stage)
        {
        const uint64_t base = ((uint64_t)chunk * a.stages + stage) * SF_BLOCK;
        if (base >= a.N)
            break;
        const uint32_t cnt = (uint32_t)std::min<uint64_t>(SF_BLOCK, a.N - base);
        double3 f = make_double3(0.0, 0.0, 0.0);
        uint32_t flag = 0;
        if (tid < cnt)
            {
            const double4 p = load_scalar4(a.pos, (uint32_t)(base + tid));
            f = fractional(a.frac, p.x, p.y, p.z);
            const bool in_a = type_in_mask(a.mask_a, a.ntypes, p.w);
            const bool in_b = NS == 2 ? in_a : type_in_mask(a.mask_b, a.ntypes, p.w);
            flag = (in_a ? 1u : 0u) | (in_b ? 2u : 0u);
            n_a += in_a;
            n_b += in_b;
            n_ab += in_a && in_b;
            }
        __syncthreads();  // (the previous stage has been read)
        s_fx[tid] = f.x;
        s_fy[tid] = f.y;
        s_fz[tid] = f.z;
        s_flag[tid] = flag;
        __syncthreads();
        double st[NS];
#pragma unroll
        for (uint32_t s = 0; s < NS; ++s)
            st[s] = 0.0;
        if (!POWERS)
            {
            for (uint32_t p0 = 0; p0 < cnt; p0 += WAVE)
                {
                // the flags of 64 staged particles as two scalar masks (every wave makes its own copy)
                const uint32_t mine = s_flag[p0 + lane];
                const unsigned long long in_a = __ballot(mine & 1u), in_b = NS == 4 ? __ballot(mine & 2u) : 0ull;
                const uint32_t end = min((uint32_t)WAVE, cnt - p0);
                for (uint32_t j = 0; j < end; ++j)
                    {
                    const bool a_j = (in_a >> j) & 1ull, b_j = NS == 4 && ((in_b >> j) & 1ull);
                    if (!(a_j || b_j))
                        continue;
                    const uint32_t p = p0 + j;
                    const double t = dh * s_fx[p] + dk * s_fy[p] + dl * s_fz[p];
                    double sn, cs;
                    sincospi(2.0 * t, &sn, &cs);
                    if (a_j)
                        {
                        st[0] += cs;
                        st[1] -= sn;
                        }
                    if (NS == 4 && b_j)
                        {
                        st[2] += cs;
                        st[3] -= sn;
                        }
                    }
                }
            }
        else
            {
            for (uint32_t sub = 0; sub < cnt; sub += SF_SUB)
                {
                const uint32_t sub_cnt = min(SF_SUB, cnt - sub);
                __syncthreads();  // (the previous tables have been read)
                if (tid < 3u * SF_SUB && (tid & (SF_SUB - 1u)) < sub_cnt)
                    {
                    const uint32_t axis = tid / SF_SUB, p = tid & (SF_SUB - 1u);
                    const double fa = axis == 0 ? s_fx[sub + p] : axis == 1 ? s_fy[sub + p] : s_fz[sub + p];
                    const int32_t H = a.H[axis];
                    const uint32_t off = axis == 0 ? 0u : axis == 1 ? (uint32_t)a.H[0] + 1u : (uint32_t)(a.H[0] + a.H[1]) + 2u;
                    double2* row = s_tab + (size_t)p * a.ne + off;  // (row[n] = e^n, 0 <= n <= H)
                    double sn, cs;
                    sincospi(2.0 * fa, &sn, &cs);
                    const double2 e = make_double2(cs, -sn);
                    double2 w = make_double2(1.0, 0.0);
                    row[0] = w;
                    for (int32_t n = 1; n <= H; ++n)
                        {
                        w = sf_cmul(w, e);
                        row[n] = w;
                        }
                    }
                __syncthreads();
                // the flags of the sub-stage as two scalar masks (every wave makes its own copy)
                const uint32_t mine = lane < sub_cnt ? s_flag[sub + lane] : 0u;
                const uint32_t in_a = (uint32_t)__ballot(mine & 1u), in_b = NS == 4 ? (uint32_t)__ballot(mine & 2u) : 0u;
                for (uint32_t p = 0; p < sub_cnt; ++p)
                    {
                    const bool a_p = (in_a >> p) & 1u, b_p = NS == 4 && ((in_b >> p) & 1u);
                    if (!(a_p || b_p))
                        continue;
                    const double2* row = s_tab + (size_t)p * a.ne;
                    const double2 w = sf_cmul(sf_cmul(sf_conj_if(row[ix], sx), sf_conj_if(row[iy], sy)), sf_conj_if(row[iz], sz));
                    if (a_p)
                        {
                        st[0] += w.x;
                        st[1] += w.y;
                        }
                    if (NS == 4 && b_p)
                        {
                        st[2] += w.x;
                        st[3] += w.y;
                        }
                    }
                }
            }
#pragma unroll
        for (uint32_t s = 0; s < NS; ++s)
            acc[s] += st[s];
        }
    if (v < a.n_vectors)
        {
#pragma unroll
        for (uint32_t s = 0; s < NS; ++s)
            a.scratch[((uint64_t)s * a.n_vectors + v) * a.n_chunks + chunk] = acc[s];
        }
    if (blockIdx.x == 0)
        {
        // the group sizes of this chunk: integers, whatever the order of the atomics
        __syncthreads();  // (s_count was zeroed)
        if (n_a) atomicAdd(&s_count[0], n_a);
        if (n_b) atomicAdd(&s_count[1], n_b);
        if (n_ab) atomicAdd(&s_count[2], n_ab);
        __syncthreads();
        if (tid < 3)
            a.scratch[((uint64_t)NS * a.n_vectors + tid) * a.n_chunks + chunk] = (double)s_count[tid];
        }
    }

// One wave per row of partials: NS * n_vectors amplitude rows, then the three group sizes. With NS = 2 the B half of
// the output is the copy of the A half.
template<uint32_t NS> __global__ void __launch_bounds__(SF_BLOCK) sf_fold(const double* scratch, uint32_t n_vectors, uint32_t n_chunks,
                                                                           double* out)
    {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint64_t item = (uint64_t)blockIdx.x * (SF_BLOCK / WAVE) + threadIdx.x / WAVE;
    const uint64_t n_amp = (uint64_t)NS * n_vectors;
    if (item >= n_amp + 3)
        return;
    const double s = fold_partials(scratch + item * n_chunks, n_chunks, lane);
    if (lane != 0)
        return;
    if (item < n_amp)
        {
        out[item] = s;
        if (NS == 2)
            out[item + n_amp] = s;
        }
    else
        {
        const uint64_t c = item - n_amp;  // 0: N_A, 1: N_B, 2: N_AB
        out[4ull * n_vectors + c] = s;
        if (c == 2)
            out[4ull * n_vectors + 3] = 0.0;
        }
    }

struct SfPlan
    {
    int path;  // 1 direct, 2 powers
    uint32_t ns;
    SfShape shape;
    uint32_t ne;
    uint64_t lds, bytes;
    };

static int sf_plan(const azp_structure_factor_args* a, SfPlan& p)
    {
    if (!a || a->n_vectors == 0 || a->n_vectors > AZP_SF_MAX_VECTORS || a->path > 2)
        return AZP_ERROR_INVALID_ARGUMENT;
    if ((a->d_type_mask_a || a->d_type_mask_b) && a->ntypes == 0)
        return AZP_ERROR_INVALID_ARGUMENT;
    for (int d = 0; d < 3; ++d)
        if (!(a->box.L[d] > 0.0) || !std::isfinite(a->box.L[d]) || !a->box.periodic[d] || !std::isfinite(a->box.tilt[d]))
            return AZP_ERROR_INVALID_ARGUMENT;
    // the tables of one sub-stage of the powers path: SF_SUB rows of ne entries (odd: the rows of the 32 builders then
    // start on different banks)
    const uint64_t ne = ((uint64_t)a->m_max[0] + a->m_max[1] + a->m_max[2] + 3ull) | 1ull;
    const uint64_t lds = ne * SF_SUB * sizeof(double2);
    const bool powers = lds <= AZP_SF_POWERS_LDS_BYTES;
    if (a->path == AZP_SF_PATH_POWERS && !powers)
        return AZP_ERROR_INVALID_ARGUMENT;
    p.path = (a->path == AZP_SF_PATH_POWERS || (a->path == AZP_SF_PATH_AUTO && powers && SF_AUTO_TAKES_POWERS)) ? 2 : 1;
    p.ns = a->same_groups ? 2 : 4;
    p.shape = sf_shape(a->N, a->n_vectors);
    p.ne = (uint32_t)ne;
    p.lds = p.path == 2 ? lds : 0;
    p.bytes = ((uint64_t)p.ns * a->n_vectors + 3) * p.shape.n_chunks * sizeof(double);
    return AZP_SUCCESS;
    }

} // namespace azp

extern "C" int azp_structure_factor_scratch_size(const azp_structure_factor_args* args, uint64_t* bytes)
    {
    using namespace azp;
    if (!bytes)
        return AZP_ERROR_INVALID_ARGUMENT;
    SfPlan p;
    const int rc = sf_plan(args, p);
    if (rc != AZP_SUCCESS)
        return rc;
    *bytes = p.bytes;
    return AZP_SUCCESS;
    }

extern "C" int azp_structure_factor_amplitudes(const azp_structure_factor_args* args, void* stream)
    {
    using namespace azp;
    SfPlan p;
    const int rc = sf_plan(args, p);
    if (rc != AZP_SUCCESS)
        return rc;
    if (!args->d_out || !args->d_vectors || (args->N && !args->d_pos))
        return AZP_ERROR_INVALID_ARGUMENT;
    if (args->N && (!args->d_scratch || args->scratch_bytes < p.bytes))
        return AZP_ERROR_INVALID_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (args->N == 0)
        return (int)hipMemsetAsync(args->d_out, 0, (4ull * args->n_vectors + 4) * sizeof(double), st);
    SfKArgs k = {};
    k.pos = args->d_pos;
    k.mask_a = args->d_type_mask_a;
    k.mask_b = args->same_groups ? args->d_type_mask_a : args->d_type_mask_b;
    k.vectors = args->d_vectors;
    k.scratch = static_cast<double*>(args->d_scratch);
    k.frac = make_frac_dev(args->box);
    k.N = args->N;
    k.ntypes = args->ntypes;
    k.n_vectors = args->n_vectors;
    k.stages = p.shape.stages;
    k.n_chunks = p.shape.n_chunks;
    for (int d = 0; d < 3; ++d)
        k.H[d] = (int32_t)args->m_max[d];
    k.ne = p.ne;
    const dim3 grid((args->n_vectors + SF_BLOCK - 1) / SF_BLOCK, p.shape.n_chunks), block(SF_BLOCK);
    const uint32_t lds = (uint32_t)p.lds;
    if (p.ns == 2 && p.path == 1)
        hipLaunchKernelGGL((sf_partial<2, false>), grid, block, 0, st, k);
    else if (p.ns == 2)
        hipLaunchKernelGGL((sf_partial<2, true>), grid, block, lds, st, k);
    else if (p.path == 1)
        hipLaunchKernelGGL((sf_partial<4, false>), grid, block, 0, st, k);
    else
        hipLaunchKernelGGL((sf_partial<4, true>), grid, block, lds, st, k);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return (int)e;
    const uint64_t items = (uint64_t)p.ns * args->n_vectors + 3;
    const dim3 fgrid((uint32_t)((items + SF_BLOCK / WAVE - 1) / (SF_BLOCK / WAVE)));
    if (p.ns == 2)
        hipLaunchKernelGGL(sf_fold<2>, fgrid, block, 0, st, k.scratch, args->n_vectors, p.shape.n_chunks, static_cast<double*>(args->d_out));
    else
        hipLaunchKernelGGL(sf_fold<4>, fgrid, block, 0, st, k.scratch, args->n_vectors, p.shape.n_chunks, static_cast<double*>(args->d_out));
    return (int)hipGetLastError();
    }
