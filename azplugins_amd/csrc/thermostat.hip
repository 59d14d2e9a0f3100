// thermostat.hip -- the thermostats of ConstantVolume (azplugins_amd.thermostats: Berendsen, Bussi, MTTK; names and
// parameter keys of hoomd.md.methods.thermostats). HOOMD-blue's source is not available here: the scheme is DEFINED
// in include/azp.h and DESIGN 4.18, and tests/thermostat_ref.py restates it in numpy.
//
// A thermostat is a scalar map (K, state, t) -> alpha that acts once per step, on the full-step velocities v(t), ahead
// of step one. It needs the kinetic energy of ALL particles between step two of one step and step one of the next,
// which is where nve_kernel<2> fuses the two: the thermostatted step has kernels of its own and a scale factor that
// never leaves the device.
//
//   thermostat_partial<false>  kinetic pass: per-workgroup partials of K = sum 1/2 m |v|^2 (once per run)
//   thermostat_partial<true>   step two, v += (dt/2) f/m, and the partials of K of the new v in the same pass
//                              (vel 32 B read + 32 B written, force 32 B: 96 B per particle, plus the partials)
//   thermostat_advance         one wave: folds the partials in reduce_fold's order (the sum is bit for bit what
//                              reduce_fold would write), draws the random numbers, computes alpha, updates the
//                              device-resident state
//   thermostat_step_one        reads alpha from the state: v = alpha v, v += (dt/2) f/m, x += dt v, wrap and image as
//                              nve_kernel<1> does (vel 64 B, force 32 B, pos 64 B, image 24 B: 184 B per particle)
//
// The sum is the reproducible two-stage sum of azp_reduce.hpp: nothing is atomic, the order depends on N alone. All
// arithmetic here is plain IEEE in the order written (no contraction), so a host restatement reproduces velocities,
// positions and partials bit for bit; alpha goes through exp / log / cos / sqrt of the device library, which differ
// from a host's by a few ulp (tests/thermostat_ref.ALPHA_REL).
//
// The advance is a kernel of its own and not folded into step one: every workgroup of step one would have to fold the
// up to 2048 partials itself (16 KB from L2 per workgroup, 4096 workgroups at N = 2^20: 64 MB of L2 reads against the
// 193 MB the pass moves) and run the serial Gamma sampler ahead of its first load, to save one launch of one wave.
#include "azp_reduce.hpp"
#include "evaluators.hpp"

namespace azp
{
constexpr uint32_t RNG_THERMOSTAT = 204;      // 201 / 202: the flow methods (flow_methods.hip)
constexpr uint32_t TS_GAMMA_MAX_ATTEMPTS = 32; // a guard, not a path: the acceptance rate exceeds 0.95 for a >= 1

struct TSKArgs
    {
    double* pos;
    double* vel;
    const double* net_force;
    int32_t* image;
    double* partials;
    double* state;
    BoxDev box;
    double dt;
    double kT;
    double tau;
    double ndof;
    uint64_t timestep;
    uint32_t seed;
    uint32_t kind;
    uint32_t N;
    uint32_t per_lane;
    uint32_t n_blocks;
    };

#pragma clang fp contract(off)
// 1/2 m |v|^2 in the order the header states
__device__ __forceinline__ double kinetic_term(const double4& v)
    {
    return 0.5 * ((((v.w * v.x) * v.x) + ((v.w * v.y) * v.y)) + ((v.w * v.z) * v.z));
    }

template<bool STEP_TWO> __global__ void __launch_bounds__(REDUCE_BLOCK) thermostat_partial(const TSKArgs a)
    {
    __shared__ double s_wave[REDUCE_WAVES];
    const uint32_t tid = threadIdx.x;
    double acc[1] = {0.0};
    const double hdt = 0.5 * a.dt;
    const uint64_t base = (uint64_t)blockIdx.x * REDUCE_BLOCK * a.per_lane;
    // (the bound is the same for every thread: all 64 lanes of a wave reach the butterfly)
    for (uint32_t j = 0; j < a.per_lane; ++j)
        {
        const uint64_t i64 = base + (uint64_t)j * REDUCE_BLOCK + tid;
        if (i64 >= a.N)
            continue;
        const uint32_t i = (uint32_t)i64;
        double4 v = load_scalar4(a.vel, i);
        if (STEP_TWO)
            {
            const double4 f = load_scalar4(a.net_force, i);
            const double minv = 1.0 / v.w;
            v.x = v.x + (hdt * f.x) * minv;
            v.y = v.y + (hdt * f.y) * minv;
            v.z = v.z + (hdt * f.z) * minv;
            store_scalar4(a.vel, i, v.x, v.y, v.z, v.w);
            }
        acc[0] += kinetic_term(v);
        }
    reduce_block_store<1>(acc, s_wave, a.partials, 0, gridDim.x, blockIdx.x);
    }

__global__ void __launch_bounds__(256) thermostat_step_one(const TSKArgs a)
    {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.N)
        return;
    const double alpha = a.state[AZP_THERMOSTAT_ALPHA];
    double4 v = load_scalar4(a.vel, idx);
    const double4 f = load_scalar4(a.net_force, idx);
    const double minv = 1.0 / v.w;
    const double hdt = 0.5 * a.dt;
    v.x = alpha * v.x; v.y = alpha * v.y; v.z = alpha * v.z;
    v.x = v.x + (hdt * f.x) * minv;
    v.y = v.y + (hdt * f.y) * minv;
    v.z = v.z + (hdt * f.z) * minv;
    store_scalar4(a.vel, idx, v.x, v.y, v.z, v.w);
    const double4 p = load_scalar4(a.pos, idx);
    double x = p.x + a.dt * v.x, y = p.y + a.dt * v.y, z = p.z + a.dt * v.z;
    wrap_with_image(a.box, x, y, z, a.image, idx);
    store_scalar4(a.pos, idx, x, y, z, p.w);
    }

// draw k of the step's stream: key (id, seed, t) as the flow methods lay it out, counter {k, 0, 0, 0}, u01 as uniform3
__device__ __forceinline__ double ts_u01(uint32_t k0, uint32_t k1, uint32_t k)
    {
    uint32_t c0 = k, c1 = 0, c2 = 0, c3 = 0;
    philox4x32_10(c0, c1, c2, c3, k0, k1);
    const uint64_t u = ((uint64_t)c0 << 32) | (uint64_t)c1;
    return (double)(u >> 11) * (1.0 / 9007199254740992.0) + (0.5 / 9007199254740992.0);
    }

// Box-Muller from the draws k and k + 1
__device__ __forceinline__ double ts_normal(uint32_t k0, uint32_t k1, uint32_t k)
    {
    const double ua = ts_u01(k0, k1, k), ub = ts_u01(k0, k1, k + 1);
    return sqrt(-2.0 * log(ua)) * cos(6.283185307179586 * ub);
    }

// Gamma(shape, 1), shape >= 1 (Marsaglia and Tsang 2000): attempt j takes its normal from the draws 2 + 3 j and
// 3 + 3 j and its uniform from 4 + 3 j
__device__ __forceinline__ double ts_gamma(uint32_t k0, uint32_t k1, double shape, double& attempts)
    {
    const double d = shape - 1.0 / 3.0;
    const double c = 1.0 / sqrt(9.0 * d);
    for (uint32_t j = 0; j < TS_GAMMA_MAX_ATTEMPTS; ++j)
        {
        const double x = ts_normal(k0, k1, 2 + 3 * j);
        const double u = ts_u01(k0, k1, 4 + 3 * j);
        const double t = 1.0 + c * x;
        const double v = (t * t) * t;
        attempts = (double)(j + 1);
        if (v > 0.0 && log(u) < ((0.5 * (x * x) + d) - d * v) + d * log(v))
            return d * v;
        }
    return d;
    }

__device__ __forceinline__ double mttk_g(const TSKArgs& a, double K)
    {
    return ((2.0 * K) / (a.ndof * a.kT) - 1.0) / (a.tau * a.tau);
    }

__global__ void __launch_bounds__(WAVE) thermostat_advance(const TSKArgs a)
    {
    const uint32_t lane = threadIdx.x;
    // reduce_fold's order: lane l adds the partials l, l + 64, ... in turn from +0.0, then the butterfly
    double K = 0.0;
#pragma unroll 8
    for (uint32_t b = lane; b < a.n_blocks; b += WAVE)
        K += a.partials[b];
    K = group_sum<WAVE>(K);
    if (lane != 0)
        return;
    double* s = a.state;
    double alpha = 1.0, attempts = 0.0;
    if (a.kind == AZP_THERMOSTAT_MTTK)
        {
        double xi = s[AZP_THERMOSTAT_XI], eta = s[AZP_THERMOSTAT_ETA];
        const double hdt = 0.5 * a.dt;
        xi = xi + hdt * mttk_g(a, K);
        alpha = exp(-(xi * a.dt));
        eta = eta + xi * a.dt;
        xi = xi + hdt * mttk_g(a, (alpha * alpha) * K);
        s[AZP_THERMOSTAT_XI] = xi;
        s[AZP_THERMOSTAT_ETA] = eta;
        s[AZP_THERMOSTAT_ENERGY] = (a.ndof * a.kT) * (0.5 * ((a.tau * a.tau) * (xi * xi)) + eta);
        }
    else if (K > 0.0)
        {
        if (a.kind == AZP_THERMOSTAT_BERENDSEN)
            {
            const double Kbar = 0.5 * (a.ndof * a.kT);
            alpha = sqrt(1.0 + (a.dt / a.tau) * (Kbar / K - 1.0));
            }
        else
            {
            const uint32_t t_hi = (uint32_t)((a.timestep >> 32) & 0xffu);
            const uint32_t k0 = (RNG_THERMOSTAT << 24) | (t_hi << 16) | (a.seed & 0xffffu);
            const uint32_t k1 = (uint32_t)(a.timestep & 0xffffffffu);
            const double c = a.tau > 0.0 ? exp(-(a.dt / a.tau)) : 0.0;
            const double R1 = ts_normal(k0, k1, 0);
            const double S = 2.0 * ts_gamma(k0, k1, 0.5 * (a.ndof - 1.0), attempts);
            const double w = (1.0 - c) * (0.5 * a.kT);
            const double r = sqrt(c * K) + R1 * sqrt(w);
            const double Knew = r * r + w * S;
            alpha = sqrt(Knew / K);
            }
        s[AZP_THERMOSTAT_ENERGY] = s[AZP_THERMOSTAT_ENERGY] + (K - (alpha * alpha) * K);
        }
    s[AZP_THERMOSTAT_ALPHA] = alpha;
    s[AZP_THERMOSTAT_K] = K;
    s[AZP_THERMOSTAT_ATTEMPTS] = attempts;
    }
#pragma clang fp contract(on)

enum { TS_KINETIC = 0, TS_STEP_TWO = 1, TS_ADVANCE = 2, TS_STEP_ONE = 3 };

static int launch_thermostat(int which, const azp_thermostat_args* args, void* stream)
    {
    if (!args || args->N == 0)
        return AZP_ERROR_INVALID_ARGUMENT;
    const ReduceShape shape = reduce_shape(args->N);
    if (which != TS_STEP_ONE && (!args->d_partials || args->partials_bytes < (uint64_t)shape.n_blocks * sizeof(double)))
        return AZP_ERROR_INVALID_ARGUMENT;
    if ((which == TS_KINETIC || which == TS_STEP_TWO || which == TS_STEP_ONE) && !args->d_vel)
        return AZP_ERROR_INVALID_ARGUMENT;
    if ((which == TS_STEP_TWO || which == TS_STEP_ONE) && (!args->d_net_force || !(args->dt > 0.0)))
        return AZP_ERROR_INVALID_ARGUMENT;
    if (which == TS_STEP_ONE && !args->d_pos)
        return AZP_ERROR_INVALID_ARGUMENT;
    if ((which == TS_ADVANCE || which == TS_STEP_ONE) && !args->d_state)
        return AZP_ERROR_INVALID_ARGUMENT;
    if (which == TS_ADVANCE)
        {
        if (args->kind > AZP_THERMOSTAT_MTTK || !(args->dt > 0.0) || !(args->kT > 0.0) || !(args->ndof >= 3.0))
            return AZP_ERROR_INVALID_ARGUMENT;
        // (Bussi: tau = 0 is the instantaneous canonical resampling; Berendsen below dt gives a negative radicand)
        if (args->kind == AZP_THERMOSTAT_BUSSI ? !(args->tau >= 0.0) : !(args->tau > 0.0))
            return AZP_ERROR_INVALID_ARGUMENT;
        if (args->kind == AZP_THERMOSTAT_BERENDSEN && args->tau < args->dt)
            return AZP_ERROR_INVALID_ARGUMENT;
        }
    TSKArgs k;
    k.pos = args->d_pos;
    k.vel = args->d_vel;
    k.net_force = args->d_net_force;
    k.image = args->d_image;
    k.partials = args->d_partials;
    k.state = args->d_state;
    k.box = make_box_dev(args->box);
    k.dt = args->dt;
    k.kT = args->kT;
    k.tau = args->tau;
    k.ndof = args->ndof;
    k.timestep = args->timestep;
    k.seed = args->seed & 0xffffu;
    k.kind = args->kind;
    k.N = args->N;
    k.per_lane = shape.per_lane;
    k.n_blocks = shape.n_blocks;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    switch (which)
        {
        case TS_KINETIC:
            hipLaunchKernelGGL(thermostat_partial<false>, dim3(shape.n_blocks), dim3(REDUCE_BLOCK), 0, s, k);
            break;
        case TS_STEP_TWO:
            hipLaunchKernelGGL(thermostat_partial<true>, dim3(shape.n_blocks), dim3(REDUCE_BLOCK), 0, s, k);
            break;
        case TS_ADVANCE:
            hipLaunchKernelGGL(thermostat_advance, dim3(1), dim3(WAVE), 0, s, k);
            break;
        default:
            hipLaunchKernelGGL(thermostat_step_one, dim3((args->N + 255u) / 256u), dim3(256), 0, s, k);
            break;
        }
    return (int)hipGetLastError();
    }
} // namespace azp

extern "C" int azp_thermostat_partials_size(uint32_t N, uint64_t* bytes)
    {
    if (!bytes || N == 0)
        return AZP_ERROR_INVALID_ARGUMENT;
    *bytes = (uint64_t)azp::reduce_shape(N).n_blocks * sizeof(double);
    return AZP_SUCCESS;
    }
extern "C" int azp_thermostat_kinetic(const azp_thermostat_args* args, void* stream)
    {
    return azp::launch_thermostat(azp::TS_KINETIC, args, stream);
    }
extern "C" int azp_thermostat_step_two(const azp_thermostat_args* args, void* stream)
    {
    return azp::launch_thermostat(azp::TS_STEP_TWO, args, stream);
    }
extern "C" int azp_thermostat_advance(const azp_thermostat_args* args, void* stream)
    {
    return azp::launch_thermostat(azp::TS_ADVANCE, args, stream);
    }
extern "C" int azp_thermostat_step_one(const azp_thermostat_args* args, void* stream)
    {
    return azp::launch_thermostat(azp::TS_STEP_ONE, args, stream);
    }
