// flow_methods.hip -- Langevin and Brownian dynamics in a flow field (gfx950): the integration methods of the
// reference's flow module, TwoStepLangevinFlow (src/TwoStepLangevinFlow.h) and TwoStepBrownianFlow
// (src/TwoStepBrownianFlow.h), with the ConstantFlow / ParabolicFlow fields (src/ConstantFlow.h,
// src/ParabolicFlow.h). The reference still uses the HOOMD-2 API there; this restates the arithmetic for HOOMD v5.
//
// One thread per particle, Scalar4 rows as two 16-byte loads. The flow kind is a template parameter. No atomics.
//
// Random stream: HOOMD-5's RandomGenerator(Seed(id, timestep, seed), Counter(tag)) as the DPD thermostat restates
// it (evaluators.hpp: philox_key0, philox_u01): key = {id << 24 | (t >> 32 & 0xff) << 16 | seed16, t & 0xffffffff},
// counter {k, tag, 0, 0} for draw k. HOOMD-blue's own source is not available to this project, so this bit layout is
// NOT checked against HOOMD; the Philox core is checked by the golden known answers (philox4x32_10_kat).
#include "azp_device.hpp"
#include "evaluators.hpp"

namespace azp
{
constexpr uint32_t RNG_BROWNIAN_FLOW = 201; // src/RNGIdentifiers.h
constexpr uint32_t RNG_LANGEVIN_FLOW = 202;

struct FlowKArgs
    {
    double* pos;
    double* vel;
    double* accel;
    const double* net_force;
    int32_t* image;
    const uint32_t* tag;
    const double* gamma;
    const uint8_t* type_mask;
    BoxDev box;
    double dt;
    double kT;
    uint64_t timestep;
    double p0, p1, p2;
    uint32_t seed;
    uint32_t noiseless;
    uint32_t N;
    uint32_t ntypes;
    };

// u(r): src/ConstantFlow.h:48-51 (U) and src/ParabolicFlow.h:69-73 (Umax (1 - (y / L)^2), 0, 0)
template<int KIND> __device__ __forceinline__ double3 flow_velocity(const FlowKArgs& a, double /*x*/, double y, double /*z*/)
    {
    if (KIND == AZP_FLOW_CONSTANT)
        return make_double3(a.p0, a.p1, a.p2);
    const double yr = y / a.p1;
    return make_double3(a.p0 * (1. - yr * yr), 0.0, 0.0);
    }

// the three uniform(-c, c) draws of one particle (UniformDistribution: a + (b - a) u01)
__device__ __forceinline__ double3 uniform3(uint32_t id, uint32_t seed, uint32_t tag, uint64_t t, double c)
    {
    const uint32_t k0 = philox_key0(id, t, seed), k1 = (uint32_t)t;
    double r[3];
#pragma unroll
    for (uint32_t k = 0; k < 3; ++k)
        r[k] = -c + 2.0 * c * philox_u01(k0, k1, k, tag, 0, 0);
    return make_double3(r[0], r[1], r[2]);
    }

// the type of row idx if this method integrates it, else -1
__device__ __forceinline__ int selected_type(const FlowKArgs& a, double w)
    {
    const int type = type_from_w(w);
    if ((uint32_t)type >= a.ntypes)
        return -1;
    if (a.type_mask && !a.type_mask[type])
        return -1;
    return type;
    }

// Langevin step two at position p (src/TwoStepLangevinFlow.h:193-245): returns the new acceleration, updates v
template<int KIND>
__device__ __forceinline__ double3 langevin_step_two(const FlowKArgs& a, uint32_t idx, const double4& p, int type, double4& v)
    {
    const double gamma = a.gamma[type];                                // :199-207
    const double3 u = flow_velocity<KIND>(a, p.x, p.y, p.z);         // :210
    double coeff = sqrt(6.0 * gamma * a.kT / a.dt);                   // :213
    if (a.noiseless)                                                   // :214-215
        coeff = 0.0;
    const double3 R = uniform3(RNG_LANGEVIN_FLOW, a.seed, a.tag[idx], a.timestep, coeff); // :216-221
    const double bx = R.x - gamma * (v.x - u.x);                       // :228
    const double by = R.y - gamma * (v.y - u.y);
    const double bz = R.z - gamma * (v.z - u.z);
    const double4 f = load_scalar4(a.net_force, idx);                  // :231-232
    const double minv = 1.0 / v.w;                                     // :234
    const double ax = (f.x + bx) * minv, ay = (f.y + by) * minv, az = (f.z + bz) * minv; // :233-237
    const double hdt = 0.5 * a.dt;                                     // :240
    v.x += hdt * ax; v.y += hdt * ay; v.z += hdt * az;
    return make_double3(ax, ay, az);
    }

// Langevin step one (src/TwoStepLangevinFlow.h:143-150): x += (v + a dt/2) dt, wrap, v += a dt/2
__device__ __forceinline__ void langevin_step_one(const FlowKArgs& a, uint32_t idx, const double4& p, double4& v,
                                                  const double3& acc)
    {
    const double hdt = 0.5 * a.dt;
    double x = p.x + (v.x + hdt * acc.x) * a.dt;                       // :145
    double y = p.y + (v.y + hdt * acc.y) * a.dt;
    double z = p.z + (v.z + hdt * acc.z) * a.dt;
    wrap_with_image(a.box, x, y, z, a.image, idx);                     // :146
    v.x += hdt * acc.x; v.y += hdt * acc.y; v.z += hdt * acc.z;        // :149
    store_scalar4(a.pos, idx, x, y, z, p.w);
    }

// MODE 0: step two. 1: step one. 2: step two of one time step, then step one of the next, in one pass (the
// acceleration of step two stays in registers; same functions, same operation order: bit-identical to 0 then 1).
template<int MODE, int KIND> __global__ void __launch_bounds__(256) langevin_flow_kernel(const FlowKArgs a)
    {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.N)
        return;
    const double4 p = load_scalar4(a.pos, idx);
    const int type = selected_type(a, p.w);
    if (type < 0)
        return;
    double4 v = load_scalar4(a.vel, idx);
    double3 acc;
    if (MODE != 1)
        {
        acc = langevin_step_two<KIND>(a, idx, p, type, v);
        store_scalar4(a.accel, idx, acc.x, acc.y, acc.z, 0.0);         // :244
        }
    else
        {
        const double4 a4 = load_scalar4(a.accel, idx);
        acc = make_double3(a4.x, a4.y, a4.z);
        }
    if (MODE != 0)
        langevin_step_one(a, idx, p, v, acc);
    store_scalar4(a.vel, idx, v.x, v.y, v.z, v.w);
    }

// Brownian step (src/TwoStepBrownianFlow.h:134-178): x += (u(x) + (F_net + R) / gamma) dt, wrap
template<int KIND> __global__ void __launch_bounds__(256) brownian_flow_kernel(const FlowKArgs a)
    {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.N)
        return;
    const double4 p = load_scalar4(a.pos, idx);
    const int type = selected_type(a, p.w);
    if (type < 0)
        return;
    const double gamma = a.gamma[type];                                // :143-150
    const double3 u = flow_velocity<KIND>(a, p.x, p.y, p.z);         // :153
    double coeff = sqrt(6.0 * gamma * a.kT / a.dt);                   // :156
    if (a.noiseless)                                                   // :157-158
        coeff = 0.0;
    const double3 R = uniform3(RNG_BROWNIAN_FLOW, a.seed, a.tag[idx], a.timestep, coeff); // :161-166
    const double4 f = load_scalar4(a.net_force, idx);                  // :169-170
    double x = p.x + (u.x + (f.x + R.x) / gamma) * a.dt;               // :173
    double y = p.y + (u.y + (f.y + R.y) / gamma) * a.dt;
    double z = p.z + (u.z + (f.z + R.z) / gamma) * a.dt;
    wrap_with_image(a.box, x, y, z, a.image, idx);                     // :174
    store_scalar4(a.pos, idx, x, y, z, p.w);
    }

enum { LANGEVIN_TWO = 0, LANGEVIN_ONE = 1, LANGEVIN_TWO_ONE = 2, BROWNIAN = 3 };

template<int KIND> static void launch_kind(int which, uint32_t grid, uint32_t bs, hipStream_t s, const FlowKArgs& k)
    {
    switch (which)
        {
        case LANGEVIN_TWO: hipLaunchKernelGGL((langevin_flow_kernel<0, KIND>), dim3(grid), dim3(bs), 0, s, k); break;
        case LANGEVIN_ONE: hipLaunchKernelGGL((langevin_flow_kernel<1, KIND>), dim3(grid), dim3(bs), 0, s, k); break;
        case LANGEVIN_TWO_ONE: hipLaunchKernelGGL((langevin_flow_kernel<2, KIND>), dim3(grid), dim3(bs), 0, s, k); break;
        default: hipLaunchKernelGGL(brownian_flow_kernel<KIND>, dim3(grid), dim3(bs), 0, s, k); break;
        }
    }

static int launch_flow(int which, const azp_flow_method_args* args, void* stream)
    {
    if (!args)
        return AZP_ERROR_INVALID_ARGUMENT;
    if (args->N == 0)
        return AZP_SUCCESS;
    if (!args->d_pos || args->ntypes == 0)
        return AZP_ERROR_INVALID_ARGUMENT;
    if (args->flow.kind != AZP_FLOW_CONSTANT && args->flow.kind != AZP_FLOW_PARABOLIC)
        return AZP_ERROR_INVALID_ARGUMENT;
    const bool step_two = which != LANGEVIN_ONE; // reads the forces, the tags and gamma
    if (step_two && (!args->d_net_force || !args->d_tag || !args->d_gamma))
        return AZP_ERROR_INVALID_ARGUMENT;
    if (which != BROWNIAN && (!args->d_vel || !args->d_accel))
        return AZP_ERROR_INVALID_ARGUMENT;
    if (!(args->dt > 0.0))
        return AZP_ERROR_INVALID_ARGUMENT;
    const uint32_t bs = args->block_size ? args->block_size : 256u;
    if (bs % 64 || bs > 256)
        return AZP_ERROR_INVALID_ARGUMENT;
    FlowKArgs k;
    k.pos = args->d_pos;
    k.vel = args->d_vel;
    k.accel = args->d_accel;
    k.net_force = args->d_net_force;
    k.image = args->d_image;
    k.tag = args->d_tag;
    k.gamma = args->d_gamma;
    k.type_mask = args->d_type_mask;
    k.box = make_box_dev(args->box);
    k.dt = args->dt;
    k.kT = args->kT;
    k.timestep = args->timestep;
    k.p0 = args->flow.p[0]; k.p1 = args->flow.p[1]; k.p2 = args->flow.p[2];
    k.seed = args->seed & 0xffffu;
    k.noiseless = args->noiseless;
    k.N = args->N;
    k.ntypes = args->ntypes;
    const uint32_t grid = (args->N + bs - 1) / bs;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (args->flow.kind == AZP_FLOW_CONSTANT)
        launch_kind<AZP_FLOW_CONSTANT>(which, grid, bs, s, k);
    else
        launch_kind<AZP_FLOW_PARABOLIC>(which, grid, bs, s, k);
    return (int)hipGetLastError();
    }
} // namespace azp

extern "C" int azp_integrate_langevin_flow_step_one(const azp_flow_method_args* args, void* stream)
    {
    return azp::launch_flow(azp::LANGEVIN_ONE, args, stream);
    }
extern "C" int azp_integrate_langevin_flow_step_two(const azp_flow_method_args* args, void* stream)
    {
    return azp::launch_flow(azp::LANGEVIN_TWO, args, stream);
    }
extern "C" int azp_integrate_langevin_flow_step_two_one(const azp_flow_method_args* args, void* stream)
    {
    return azp::launch_flow(azp::LANGEVIN_TWO_ONE, args, stream);
    }
extern "C" int azp_integrate_brownian_flow_step(const azp_flow_method_args* args, void* stream)
    {
    return azp::launch_flow(azp::BROWNIAN, args, stream);
    }
