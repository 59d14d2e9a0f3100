// displacement.hip -- what compute.MeanSquaredDisplacement and compute.SelfIntermediateScattering measure between two
// times (include/azp.h states the contract, DESIGN 4.31 the reasons):
//   azp_displacement_origin   scatters pos and image of every row into one slot of an origin store indexed by TAG, and
//                             builds the reverse-tag table rtag[tag[i]] = i
//   azp_displacement_moments  per origin slot one row: N_g, the sums of d, of the six products d_a d_b and of |d|^4, and
//                             the integer histogram of |d| (the self part of the van Hove function)
//   azp_self_scattering       per origin slot rho_s(m) = sum exp(-2 pi i m . (f - f0)) on the vectors of
//                             compute.structure_factor_vectors
// Everything runs in TAG order: thread t takes a tag, reads the origin of that tag (coalesced: the store is by tag) and
// gathers the current row through rtag. The sums therefore do not depend on the order of the rows: a sort between two
// reads changes no bit. No floating-point atomics anywhere; the integer words are LDS counters per workgroup that are
// added with 64-bit integer atomics (bonded_histogram.hip does the same).
//
// The origins are a grid dimension (blockIdx.y of dm_partial, blockIdx.z of ss_partial): every (workgroup, slot) reads
// the current rows of its tags again. A workgroup of a slot whose bit in active_mask is clear leaves at once; the row
// was zeroed by the memset ahead of the launch. (A loop over the slots inside the workgroup, with the origins no grid
// dimension, was measured and was slower: 0.129 against 0.120 ms at 8 origins, 0.481 against 0.434 ms at 32, N = 2^20;
// profiles/displacement.md.)
//
// Bytes per particle and origin of dm_partial: origin 32 (the position row: 24 are used) + 12 (image), rtag 4, and
// gathered through rtag: pos 32, image 12 (a 32-byte sector or two), tag 4 (a sector): 96 requested, about 160 fetched
// when the rows are in no order relative to the tags.
#include <cmath>

#include "azp_reduce.hpp"
#include "cell_bin.hpp"
#include "sf_shape.hpp"

namespace azp
{
constexpr uint32_t DM_BLOCK = REDUCE_BLOCK;
constexpr uint32_t DM_NS = AZP_DISPLACEMENT_NSUMS;
constexpr uint32_t DM_LIVE = 11;  // slots that are summed (11 is the pad)
constexpr uint32_t DM_INT = 2;    // bad_tags, outside

__global__ void __launch_bounds__(256) displacement_origin_kernel(const azp_displacement_origin_args a)
    {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.N)
        return;
    const uint32_t g = a.d_tag[i];
    if (g >= a.N)
        return;  // (a forged tag: no slot is written, the kernels below report the slot that stays empty)
    if (a.build_rtag)
        a.d_rtag[g] = i;
    if (a.d_origin_pos)
        {
        const uint64_t slot = (uint64_t)a.slot * a.N + g;
        const double4 p = load_scalar4(a.d_pos, i);
        double* out = a.d_origin_pos + 4ull * slot;
        out[0] = p.x; out[1] = p.y; out[2] = p.z; out[3] = p.w;
        int32_t* img = a.d_origin_image + 3ull * slot;
        img[0] = a.d_image[3ull * i]; img[1] = a.d_image[3ull * i + 1]; img[2] = a.d_image[3ull * i + 2];
        }
    }

struct DmKArgs
    {
    const double* pos;
    const int32_t* image;
    const uint32_t* tag;
    const uint32_t* rtag;
    const uint8_t* mask;
    const double* pos0;
    const int32_t* image0;
    double* scratch;
    unsigned long long* out;
    double* disp;
    double Lx, Ly, Lz, hxy, hxz, hyz;
    double r_max, scale;
    uint64_t active;
    uint32_t N, ntypes, per_lane, num_bins, width;
    };

// the row of tag g, or N where the slot is bad (no row, or a row that carries another tag)
__device__ __forceinline__ uint32_t row_of_tag(const uint32_t* rtag, const uint32_t* tag, uint32_t N, uint32_t g)
    {
    const uint32_t i = rtag[g];
    return (i < N && tag[i] == g) ? i : N;
    }

#pragma clang fp contract(off)
__global__ void __launch_bounds__(DM_BLOCK) dm_partial(const DmKArgs a)
    {
    extern __shared__ uint32_t s_hist[];  // num_bins counters
    __shared__ double s_wave[REDUCE_WAVES * DM_LIVE];
    __shared__ uint32_t s_int[DM_INT];
    const uint32_t tid = threadIdx.x, o = blockIdx.y;
    if (!((a.active >> o) & 1ull))
        return;  // (the whole workgroup: nothing below is reached by a part of it)
    for (uint32_t k = tid; k < a.num_bins; k += DM_BLOCK)
        s_hist[k] = 0;
    if (tid < DM_INT)
        s_int[tid] = 0;
    __syncthreads();
    double acc[DM_LIVE];
#pragma unroll
    for (uint32_t k = 0; k < DM_LIVE; ++k)
        acc[k] = 0.0;
    uint32_t bad = 0, outside = 0;
    const double* pos0 = a.pos0 + 4ull * o * a.N;
    const int32_t* image0 = a.image0 + 3ull * o * a.N;
    const bool store = a.disp != nullptr && o == 0;
    const uint64_t base = (uint64_t)blockIdx.x * DM_BLOCK * a.per_lane;
    // (the bound is the same for every thread: all 64 lanes of a wave reach the butterfly)
    for (uint32_t j = 0; j < a.per_lane; ++j)
        {
        const uint64_t g64 = base + (uint64_t)j * DM_BLOCK + tid;
        if (g64 >= a.N)
            continue;
        const uint32_t g = (uint32_t)g64;
        const uint32_t i = row_of_tag(a.rtag, a.tag, a.N, g);
        if (i >= a.N)
            {
            ++bad;
            if (store)
                {
                a.disp[3ull * g] = 0.0; a.disp[3ull * g + 1] = 0.0; a.disp[3ull * g + 2] = 0.0;
                }
            continue;
            }
        const double4 p = load_scalar4(a.pos, i);
        const double3 p0 = load_scalar3_of4(pos0, g);
        // (wrapping subtraction: no undefined overflow whatever the counters hold)
        const double nx = (double)(int32_t)((uint32_t)a.image[3ull * i] - (uint32_t)image0[3ull * g]);
        const double ny = (double)(int32_t)((uint32_t)a.image[3ull * i + 1] - (uint32_t)image0[3ull * g + 1]);
        const double nz = (double)(int32_t)((uint32_t)a.image[3ull * i + 2] - (uint32_t)image0[3ull * g + 2]);
        const double dx = (p.x - p0.x) + ((a.Lx * nx + a.hxy * ny) + a.hxz * nz);
        const double dy = (p.y - p0.y) + (a.Ly * ny + a.hyz * nz);
        const double dz = (p.z - p0.z) + a.Lz * nz;
        if (store)
            {
            a.disp[3ull * g] = dx; a.disp[3ull * g + 1] = dy; a.disp[3ull * g + 2] = dz;
            }
        if (!type_in_mask(a.mask, a.ntypes, p.w))
            continue;
        const double r2 = (dx * dx + dy * dy) + dz * dz;
        acc[0] += 1.0;
        acc[1] += dx; acc[2] += dy; acc[3] += dz;
        acc[4] += dx * dx; acc[5] += dy * dy; acc[6] += dz * dz;
        acc[7] += dx * dy; acc[8] += dx * dz; acc[9] += dy * dz;
        acc[10] += r2 * r2;
        if (a.num_bins)
            {
            const double r = sqrt(r2);
            if (r >= a.r_max)
                ++outside;
            else
                atomicAdd(&s_hist[min((uint32_t)(r * a.scale), a.num_bins - 1u)], 1u);
            }
        }
    if (bad) atomicAdd(&s_int[0], bad);
    if (outside) atomicAdd(&s_int[1], outside);
    reduce_block_store<DM_LIVE>(acc, s_wave, a.scratch + (uint64_t)o * DM_NS * gridDim.x, 0, gridDim.x, blockIdx.x);
    __syncthreads();  // (every LDS counter has been added)
    unsigned long long* row = a.out + (uint64_t)o * a.width;
    if (tid < DM_INT && s_int[tid])
        atomicAdd(&row[DM_NS + tid], (unsigned long long)s_int[tid]);
    for (uint32_t k = tid; k < a.num_bins; k += DM_BLOCK)
        {
        const uint32_t v = s_hist[k];
        if (v)
            atomicAdd(&row[DM_NS + DM_INT + k], (unsigned long long)v);
        }
    }
#pragma clang fp contract(on)

// grid (DM_NS, n_origins), one wave each: the sums of an active slot (the pad is written as zero)
__global__ void __launch_bounds__(WAVE) dm_fold(const double* scratch, uint32_t n_blocks, uint64_t active, uint32_t width, double* out)
    {
    const uint32_t slot = blockIdx.x, o = blockIdx.y;
    if (!((active >> o) & 1ull))
        return;
    double s = 0.0;
    if (slot < DM_LIVE)
        s = fold_partials(scratch + ((uint64_t)o * DM_NS + slot) * n_blocks, n_blocks, threadIdx.x);
    if (threadIdx.x == 0)
        out[(uint64_t)o * width + slot] = s;
    }

struct SsKArgs
    {
    const double* pos;
    const uint32_t* tag;
    const uint32_t* rtag;
    const uint8_t* mask;
    const double* pos0;
    const int32_t* vectors;
    double* scratch;
    FracDev frac;
    uint64_t active;
    uint32_t N, ntypes, n_vectors, stages, n_chunks;
    };

// Grid (ceil(n_vectors / 256), n_chunks, n_origins). The walk over a staged set is that of sf_partial<2, false>
// (structure_factor.hip): one lane per vector, the staged tags in order, broadcast reads of LDS.
__global__ void __launch_bounds__(SF_BLOCK) ss_partial(const SsKArgs a)
    {
    __shared__ double s_fx[SF_BLOCK], s_fy[SF_BLOCK], s_fz[SF_BLOCK];
    __shared__ uint32_t s_flag[SF_BLOCK];
    __shared__ uint32_t s_count[2];
    const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1);
    const uint32_t v = blockIdx.x * SF_BLOCK + tid;
    const uint32_t chunk = blockIdx.y, o = blockIdx.z;
    if (!((a.active >> o) & 1ull))
        return;  // (the whole workgroup)
    int32_t h = 0, k = 0, l = 0;
    if (v < a.n_vectors)
        {
        h = a.vectors[3ull * v];
        k = a.vectors[3ull * v + 1];
        l = a.vectors[3ull * v + 2];
        }
    const double dh = (double)h, dk = (double)k, dl = (double)l;
    if (tid < 2)
        s_count[tid] = 0;
    const double* pos0 = a.pos0 + 4ull * o * a.N;
    double acc[2] = {0.0, 0.0};
    uint32_t n_g = 0, n_bad = 0;
    for (uint32_t stage = 0; stage < a.stages; ++stage)
        {
        const uint64_t base = ((uint64_t)chunk * a.stages + stage) * SF_BLOCK;
        if (base >= a.N)
            break;
        const uint32_t cnt = (uint32_t)std::min<uint64_t>(SF_BLOCK, a.N - base);
        double3 df = make_double3(0.0, 0.0, 0.0);
        uint32_t flag = 0;
        if (tid < cnt)
            {
            const uint32_t g = (uint32_t)(base + tid);
            const uint32_t i = row_of_tag(a.rtag, a.tag, a.N, g);
            if (i >= a.N)
                ++n_bad;
            else
                {
                const double4 p = load_scalar4(a.pos, i);
                const double3 p0 = load_scalar3_of4(pos0, g);
                const double3 f = fractional(a.frac, p.x, p.y, p.z);
                const double3 f0 = fractional(a.frac, p0.x, p0.y, p0.z);
                df = make_double3(f.x - f0.x, f.y - f0.y, f.z - f0.z);
                flag = type_in_mask(a.mask, a.ntypes, p.w) ? 1u : 0u;
                n_g += flag;
                }
            }
        __syncthreads();  // (the previous stage has been read)
        s_fx[tid] = df.x;
        s_fy[tid] = df.y;
        s_fz[tid] = df.z;
        s_flag[tid] = flag;
        __syncthreads();
        double st[2] = {0.0, 0.0};
        for (uint32_t p0 = 0; p0 < cnt; p0 += WAVE)
            {
            // the flags of 64 staged tags as a scalar mask (every wave makes its own copy)
            const uint32_t mine = s_flag[p0 + lane];
            const unsigned long long in_g = __ballot(mine & 1u);
            const uint32_t end = min((uint32_t)WAVE, cnt - p0);
            for (uint32_t j = 0; j < end; ++j)
                {
                if (!((in_g >> j) & 1ull))
                    continue;
                const uint32_t p = p0 + j;
                const double t = dh * s_fx[p] + dk * s_fy[p] + dl * s_fz[p];
                double sn, cs;
                sincospi(2.0 * t, &sn, &cs);
                st[0] += cs;
                st[1] -= sn;
                }
            }
        acc[0] += st[0];
        acc[1] += st[1];
        }
    const uint64_t rows = 2ull * a.n_vectors + 2;
    double* scratch = a.scratch + (uint64_t)o * rows * a.n_chunks;
    if (v < a.n_vectors)
        {
        scratch[(uint64_t)v * a.n_chunks + chunk] = acc[0];
        scratch[((uint64_t)a.n_vectors + v) * a.n_chunks + chunk] = acc[1];
        }
    if (blockIdx.x == 0)
        {
        // the group size and the bad slots of this chunk: integers, whatever the order of the atomics
        __syncthreads();  // (s_count was zeroed)
        if (n_g) atomicAdd(&s_count[0], n_g);
        if (n_bad) atomicAdd(&s_count[1], n_bad);
        __syncthreads();
        if (tid < 2)
            scratch[(2ull * a.n_vectors + tid) * a.n_chunks + chunk] = (double)s_count[tid];
        }
    }

// grid (ceil((2 n + 2) / 4), n_origins): one wave per row of partials of an active slot
__global__ void __launch_bounds__(SF_BLOCK) ss_fold(const double* scratch, uint32_t n_vectors, uint32_t n_chunks, uint64_t active, double* out)
    {
    const uint32_t lane = threadIdx.x & (WAVE - 1), o = blockIdx.y;
    const uint64_t item = (uint64_t)blockIdx.x * (SF_BLOCK / WAVE) + threadIdx.x / WAVE;
    const uint64_t rows = 2ull * n_vectors + 2;
    if (item >= rows || !((active >> o) & 1ull))
        return;
    const double s = fold_partials(scratch + ((uint64_t)o * rows + item) * n_chunks, n_chunks, lane);
    if (lane == 0)
        out[(uint64_t)o * rows + item] = s;
    }

static bool dp_box_ok(const azp_box& b, bool periodic)
    {
    for (int d = 0; d < 3; ++d)
        if (!(b.L[d] > 0.0) || !std::isfinite(b.L[d]) || !std::isfinite(b.tilt[d]) || (periodic && !b.periodic[d]))
            return false;
    return true;
    }

static int dp_check(const azp_displacement_args* a, bool scattering)
    {
    if (!a || a->n_origins < 1 || a->n_origins > AZP_DISPLACEMENT_MAX_ORIGINS)
        return AZP_ERROR_INVALID_ARGUMENT;
    if (a->d_type_mask && a->ntypes == 0)
        return AZP_ERROR_INVALID_ARGUMENT;
    if (!dp_box_ok(a->box, scattering))
        return AZP_ERROR_INVALID_ARGUMENT;
    if (scattering)
        {
        if (a->n_vectors < 1 || a->n_vectors > AZP_SF_MAX_VECTORS)
            return AZP_ERROR_INVALID_ARGUMENT;
        }
    else
        {
        if (a->num_bins > AZP_RDF_MAX_BINS)
            return AZP_ERROR_INVALID_ARGUMENT;
        if (a->num_bins > 0 && !(a->r_max > 0.0 && std::isfinite(a->r_max)))
            return AZP_ERROR_INVALID_ARGUMENT;
        }
    return AZP_SUCCESS;
    }

static uint64_t dm_bytes(const azp_displacement_args* a)
    {
    return (uint64_t)a->n_origins * DM_NS * reduce_shape(a->N).n_blocks * sizeof(double);
    }

static uint64_t ss_bytes(const azp_displacement_args* a)
    {
    return (uint64_t)a->n_origins * (2ull * a->n_vectors + 2) * sf_shape(a->N, a->n_vectors).n_chunks * sizeof(double);
    }

} // namespace azp

extern "C" int azp_displacement_origin(const azp_displacement_origin_args* a, void* stream)
    {
    using namespace azp;
    if (!a || a->n_slots < 1 || a->slot >= a->n_slots)
        return AZP_ERROR_INVALID_ARGUMENT;
    if (!a->d_origin_pos && !a->build_rtag)
        return AZP_ERROR_INVALID_ARGUMENT;
    if (a->N == 0)
        return AZP_SUCCESS;
    if (!a->d_tag || (a->build_rtag && !a->d_rtag))
        return AZP_ERROR_INVALID_ARGUMENT;
    if (a->d_origin_pos && (!a->d_origin_image || !a->d_pos || !a->d_image))
        return AZP_ERROR_INVALID_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (a->build_rtag)
        {
        const hipError_t e = hipMemsetAsync(a->d_rtag, 0xFF, (uint64_t)a->N * sizeof(uint32_t), st);
        if (e != hipSuccess)
            return (int)e;
        }
    hipLaunchKernelGGL(displacement_origin_kernel, dim3((a->N + 255u) / 256u), dim3(256), 0, st, *a);
    return (int)hipGetLastError();
    }

extern "C" int azp_displacement_moments_scratch_size(const azp_displacement_args* args, uint64_t* bytes)
    {
    using namespace azp;
    if (!bytes)
        return AZP_ERROR_INVALID_ARGUMENT;
    const int rc = dp_check(args, false);
    if (rc != AZP_SUCCESS)
        return rc;
    *bytes = dm_bytes(args);
    return AZP_SUCCESS;
    }

extern "C" int azp_displacement_moments(const azp_displacement_args* args, void* stream)
    {
    using namespace azp;
    const int rc = dp_check(args, false);
    if (rc != AZP_SUCCESS)
        return rc;
    if (!args->d_out)
        return AZP_ERROR_INVALID_ARGUMENT;
    const uint32_t width = DM_NS + DM_INT + args->num_bins;
    if (args->N)
        {
        if (!args->d_pos || !args->d_image || !args->d_tag || !args->d_rtag || !args->d_origin_pos || !args->d_origin_image)
            return AZP_ERROR_INVALID_ARGUMENT;
        if (!args->d_scratch || args->scratch_bytes < dm_bytes(args))
            return AZP_ERROR_INVALID_ARGUMENT;
        }
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(args->d_out, 0, (uint64_t)args->n_origins * width * 8ull, st);
    if (e != hipSuccess || args->N == 0)
        return (int)e;
    const uint64_t active = args->n_origins == 64 ? args->active_mask : args->active_mask & ((1ull << args->n_origins) - 1ull);
    if (active == 0)
        return AZP_SUCCESS;
    const ReduceShape s = reduce_shape(args->N);
    DmKArgs k;
    k.pos = args->d_pos;
    k.image = args->d_image;
    k.tag = args->d_tag;
    k.rtag = args->d_rtag;
    k.mask = args->d_type_mask;
    k.pos0 = args->d_origin_pos;
    k.image0 = args->d_origin_image;
    k.scratch = static_cast<double*>(args->d_scratch);
    k.out = static_cast<unsigned long long*>(args->d_out);
    k.disp = (active & 1ull) ? args->d_displacements : nullptr;
    k.Lx = args->box.L[0]; k.Ly = args->box.L[1]; k.Lz = args->box.L[2];
    k.hxy = args->box.tilt[0] * args->box.L[1];
    k.hxz = args->box.tilt[1] * args->box.L[2];
    k.hyz = args->box.tilt[2] * args->box.L[2];
    k.r_max = args->num_bins ? args->r_max : 0.0;
    k.scale = args->num_bins ? (double)args->num_bins / args->r_max : 0.0;
    k.active = active;
    k.N = args->N;
    k.ntypes = args->ntypes;
    k.per_lane = s.per_lane;
    k.num_bins = args->num_bins;
    k.width = width;
    hipLaunchKernelGGL(dm_partial, dim3(s.n_blocks, args->n_origins), dim3(DM_BLOCK), args->num_bins * sizeof(uint32_t), st, k);
    e = hipGetLastError();
    if (e != hipSuccess)
        return (int)e;
    hipLaunchKernelGGL(dm_fold, dim3(DM_NS, args->n_origins), dim3(WAVE), 0, st, k.scratch, s.n_blocks, active, width,
                       static_cast<double*>(args->d_out));
    return (int)hipGetLastError();
    }

extern "C" int azp_self_scattering_scratch_size(const azp_displacement_args* args, uint64_t* bytes)
    {
    using namespace azp;
    if (!bytes)
        return AZP_ERROR_INVALID_ARGUMENT;
    const int rc = dp_check(args, true);
    if (rc != AZP_SUCCESS)
        return rc;
    *bytes = ss_bytes(args);
    return AZP_SUCCESS;
    }

extern "C" int azp_self_scattering(const azp_displacement_args* args, void* stream)
    {
    using namespace azp;
    const int rc = dp_check(args, true);
    if (rc != AZP_SUCCESS)
        return rc;
    if (!args->d_out || !args->d_vectors)
        return AZP_ERROR_INVALID_ARGUMENT;
    if (args->N)
        {
        if (!args->d_pos || !args->d_tag || !args->d_rtag || !args->d_origin_pos)
            return AZP_ERROR_INVALID_ARGUMENT;
        if (!args->d_scratch || args->scratch_bytes < ss_bytes(args))
            return AZP_ERROR_INVALID_ARGUMENT;
        }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint64_t rows = 2ull * args->n_vectors + 2;
    hipError_t e = hipMemsetAsync(args->d_out, 0, (uint64_t)args->n_origins * rows * sizeof(double), st);
    if (e != hipSuccess || args->N == 0)
        return (int)e;
    const uint64_t active = args->n_origins == 64 ? args->active_mask : args->active_mask & ((1ull << args->n_origins) - 1ull);
    if (active == 0)
        return AZP_SUCCESS;
    const SfShape s = sf_shape(args->N, args->n_vectors);
    SsKArgs k;
    k.pos = args->d_pos;
    k.tag = args->d_tag;
    k.rtag = args->d_rtag;
    k.mask = args->d_type_mask;
    k.pos0 = args->d_origin_pos;
    k.vectors = args->d_vectors;
    k.scratch = static_cast<double*>(args->d_scratch);
    k.frac = make_frac_dev(args->box);
    k.active = active;
    k.N = args->N;
    k.ntypes = args->ntypes;
    k.n_vectors = args->n_vectors;
    k.stages = s.stages;
    k.n_chunks = s.n_chunks;
    const dim3 grid((args->n_vectors + SF_BLOCK - 1) / SF_BLOCK, s.n_chunks, args->n_origins), block(SF_BLOCK);
    hipLaunchKernelGGL(ss_partial, grid, block, 0, st, k);
    e = hipGetLastError();
    if (e != hipSuccess)
        return (int)e;
    const dim3 fgrid((uint32_t)((rows + SF_BLOCK / WAVE - 1) / (SF_BLOCK / WAVE)), args->n_origins);
    hipLaunchKernelGGL(ss_fold, fgrid, block, 0, st, k.scratch, args->n_vectors, s.n_chunks, active, static_cast<double*>(args->d_out));
    return (int)hipGetLastError();
    }
