// angle_forces.hip -- three-body bending forces over a per-particle angle table. The reference holds no angle code:
// the semantics are HOOMD's documented md.angle.Harmonic and md.angle.CosineSquared conventions, defined in
// include/azp.h ("angle forces") and DESIGN 4.16.
//
// One lane per particle, no atomics: the lane walks its table entries in order and keeps, of each angle, the force
// on its own position, a third of the energy and a third of the virial. The three lanes of one angle evaluate the
// same expression on the same operands, so their forces add to zero to rounding and two calls give the same bits.
// Table columns are particle-major (entry s of particle i at s * pitch + i): every table read is one coalesced
// 16-byte load; the two partner positions are the only gathers. Per-angle-type parameters are staged in LDS.
#include "azp_device.hpp"
#include "pair_kernel_host.hpp"

namespace azp
{
// U and g = dU/d(cos theta) from c = cos theta (clamped) and s = max(sin theta, 1e-3)
struct EvalAngleHarmonic
    {
    typedef azp_angle_harmonic_params Params;
    static __device__ __forceinline__ void eval(const Params& p, double c, double s, double& U, double& g)
        {
        const double dth = acos(c) - p.t0;
        const double kd = p.k * dth;
        U = 0.5 * kd * dth;
        g = -kd * fast_rcp(s);
        }
    };

struct EvalAngleCosineSquared
    {
    typedef azp_angle_cossq_params Params;
    static __device__ __forceinline__ void eval(const Params& p, double c, double s, double& U, double& g)
        {
        const double dc = c - p.cos_t0;
        g = p.k * dc;
        U = 0.5 * g * dc;
        }
    };

struct AngleKArgs
    {
    double* force;
    double* virial;
    uint64_t virial_pitch;
    const double* pos;
    const azp_angle_entry* anglelist;
    const uint32_t* n_angles;
    uint64_t pitch;
    BoxDev box;
    uint32_t N;
    uint32_t n_angle_types;
    uint32_t compute_virial;
    uint32_t _pad;
    };

__device__ __forceinline__ azp_angle_entry load_angle_entry(const azp_angle_entry* table, uint64_t at)
    {
    const uint4 w = reinterpret_cast<const uint4*>(table)[at];
    azp_angle_entry e;
    e.idx[0] = w.x; e.idx[1] = w.y; e.type = w.z; e.pos = w.w;
    return e;
    }

// component-wise select (a ?: on the structs makes the compiler pick between addresses and park the batch in scratch)
__device__ __forceinline__ double3 select3(bool take_first, const double3& x, const double3& y)
    {
    return make_double3(take_first ? x.x : y.x, take_first ? x.y : y.y, take_first ? x.z : y.z);
    }

template<class E>
__global__ void __launch_bounds__(256) angle_forces_kernel(const AngleKArgs a, const typename E::Params* __restrict__ params)
    {
    typedef typename E::Params Params;
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    Params* s_params = reinterpret_cast<Params*>(s_raw);
    for (uint32_t t = threadIdx.x; t < a.n_angle_types; t += blockDim.x)
        s_params[t] = params[t];
    __syncthreads();

    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.N)
        return;
    const uint32_t na = a.n_angles[idx];
    const double3 p = load_scalar3_of4(a.pos, idx);
    double fx = 0.0, fy = 0.0, fz = 0.0, pe = 0.0;
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    auto one_angle = [&](const azp_angle_entry& ent, const double3& q0, const double3& q1)
        {
        // members in angle order: this lane's own position goes into slot ent.pos, the partners fill the rest
        const bool is_a = ent.pos == 0, is_c = ent.pos == 2;
        const double3 ra = select3(is_a, p, q0);
        const double3 rb = select3(is_a, q0, select3(is_c, q1, p));
        const double3 rc = select3(is_c, p, q1);
        double abx = ra.x - rb.x, aby = ra.y - rb.y, abz = ra.z - rb.z;
        double cbx = rc.x - rb.x, cby = rc.y - rb.y, cbz = rc.z - rb.z;
        min_image(a.box, abx, aby, abz);
        min_image(a.box, cbx, cby, cbz);
        const double rsqab = abx * abx + aby * aby + abz * abz;
        const double rsqcb = cbx * cbx + cby * cby + cbz * cbz;
        const double inv = fast_rsqrt(rsqab * rsqcb); // 1 / (|dab| |dcb|)
        double c = (abx * cbx + aby * cby + abz * cbz) * inv;
        c = fmin(fmax(c, -1.0), 1.0);
        // (1 - c)(1 + c): one of the factors is exact wherever 1 - c * c would cancel
        const double s = fmax(fast_sqrt((1.0 - c) * (1.0 + c)), 1e-3);
        double U, g;
        E::eval(s_params[ent.type], c, s, U, g);
        const double ca = c * fast_rcp(rsqab), cc = c * fast_rcp(rsqcb);
        const double fax = -g * (cbx * inv - ca * abx), fay = -g * (cby * inv - ca * aby), faz = -g * (cbz * inv - ca * abz);
        const double fcx = -g * (abx * inv - cc * cbx), fcy = -g * (aby * inv - cc * cby), fcz = -g * (abz * inv - cc * cbz);
        // F_b = -F_a - F_c
        fx += is_a ? fax : (is_c ? fcx : -(fax + fcx));
        fy += is_a ? fay : (is_c ? fcy : -(fay + fcy));
        fz += is_a ? faz : (is_c ? fcz : -(faz + fcz));
        const double third = 1.0 / 3.0;
        pe += third * U;
        if (a.compute_virial)
            {
            v[0] += third * (abx * fax + cbx * fcx); v[1] += third * (abx * fay + cbx * fcy);
            v[2] += third * (abx * faz + cbx * fcz); v[3] += third * (aby * fay + cby * fcy);
            v[4] += third * (aby * faz + cby * fcz); v[5] += third * (abz * faz + cbz * fcz);
            }
        };
    // As the bond kernel: the first BATCH table columns of every lane are loaded together, then their 2 * BATCH
    // partner positions together -- two dependent round trips per particle instead of two per angle (an interior
    // bead of a linear chain has 3 entries). BATCH = 3 holds that bead in one batch; the harmonic kernel takes 110
    // VGPRs at 2, 3 and 4 alike (acos sets its peak), the cosine-squared one 75 / 89 / 103.
    constexpr uint32_t BATCH = 3;
    azp_angle_entry ent[BATCH];
#pragma unroll
    for (uint32_t b = 0; b < BATCH; ++b)
        {
        ent[b].idx[0] = idx; ent[b].idx[1] = idx; ent[b].type = 0; ent[b].pos = 0;
        if (b < na)
            ent[b] = load_angle_entry(a.anglelist, (uint64_t)b * a.pitch + idx);
        }
    double3 q0[BATCH], q1[BATCH];
#pragma unroll
    for (uint32_t b = 0; b < BATCH; ++b)
        {
        q0[b] = load_scalar3_of4(a.pos, ent[b].idx[0]); // unused slots re-read the lane's own (cached) row
        q1[b] = load_scalar3_of4(a.pos, ent[b].idx[1]);
        }
#pragma unroll
    for (uint32_t b = 0; b < BATCH; ++b)
        if (b < na)
            one_angle(ent[b], q0[b], q1[b]);
    for (uint32_t b = BATCH; b < na; ++b)
        {
        const azp_angle_entry e = load_angle_entry(a.anglelist, (uint64_t)b * a.pitch + idx);
        one_angle(e, load_scalar3_of4(a.pos, e.idx[0]), load_scalar3_of4(a.pos, e.idx[1]));
        }
    store_scalar4(a.force, idx, fx, fy, fz, pe);
    if (a.compute_virial)
        {
#pragma unroll
        for (int c = 0; c < 6; ++c)
            a.virial[(uint64_t)c * a.virial_pitch + idx] = v[c];
        }
    }

template<class E>
static int launch_angle(const azp_angle_args* args, const typename E::Params* d_params, void* stream)
    {
    if (!args)
        return AZP_ERROR_INVALID_ARGUMENT;
    if (args->N == 0)
        return AZP_SUCCESS;
    if (!d_params || !args->d_force || !args->d_pos || !args->d_gpu_anglelist || !args->d_gpu_n_angles
        || args->pitch < args->N || args->n_angle_types == 0)
        return AZP_ERROR_INVALID_ARGUMENT;
    if (args->compute_virial && (!args->d_virial || args->virial_pitch < args->N))
        return AZP_ERROR_INVALID_ARGUMENT;
    const uint32_t bs = args->block_size ? args->block_size : 256u;
    if (bs % 64 || bs > 256)
        return AZP_ERROR_INVALID_ARGUMENT;
    const size_t lds = sizeof(typename E::Params) * (size_t)args->n_angle_types;
    if (lds > 64 * 1024)
        return AZP_ERROR_TOO_MANY_TYPES;
    AngleKArgs k;
    k.force = args->d_force;
    k.virial = args->d_virial;
    k.virial_pitch = args->virial_pitch;
    k.pos = args->d_pos;
    k.anglelist = args->d_gpu_anglelist;
    k.n_angles = args->d_gpu_n_angles;
    k.pitch = args->pitch;
    k.box = make_box_dev(args->box);
    k.N = args->N;
    k.n_angle_types = args->n_angle_types;
    k.compute_virial = args->compute_virial;
    k._pad = 0;
    const uint32_t grid = (args->N + bs - 1) / bs;
    LaunchInfo& li = last_launch();
    li.block_size = bs; li.tpp = 1; li.grid = grid; li.lds_bytes = (uint32_t)lds;
    hipLaunchKernelGGL(angle_forces_kernel<E>, dim3(grid), dim3(bs), lds, static_cast<hipStream_t>(stream), k, d_params);
    return (int)hipGetLastError();
    }
} // namespace azp

extern "C" int azp_angle_forces_harmonic(const azp_angle_args* args, const azp_angle_harmonic_params* d_params, void* stream)
    {
    return azp::launch_angle<azp::EvalAngleHarmonic>(args, d_params, stream);
    }

extern "C" int azp_angle_forces_cosine_squared(const azp_angle_args* args, const azp_angle_cossq_params* d_params,
                                               void* stream)
    {
    return azp::launch_angle<azp::EvalAngleCosineSquared>(args, d_params, stream);
    }
