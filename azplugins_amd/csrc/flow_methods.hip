// flow_methods.hip -- Langevin and Brownian dynamics in a flow field (gfx950): the integration methods of the
// reference's flow module, TwoStepLangevinFlow (src/TwoStepLangevinFlow.h) and TwoStepBrownianFlow
// (src/TwoStepBrownianFlow.h), with the ConstantFlow / ParabolicFlow fields (src/ConstantFlow.h,
// src/ParabolicFlow.h). The reference still uses the HOOMD-2 API there; this restates the arithmetic for HOOMD v5.
//
// One thread per particle, Scalar4 rows as two 16-byte loads. The flow kind is a template parameter. No atomics.
//
// The random stream, the type selection and the half steps themselves are langevin_device.hpp's, shared with langevin.hip.
#include "langevin_device.hpp"

namespace azp
{
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
    LangevinScalars s;
    double p0, p1, p2;
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

// MODE 0: step two. 1: step one. 2: step two of one time step, then step one of the next, in one pass (the
// acceleration of step two stays in registers; same functions, same operation order: bit-identical to 0 then 1).
template<int MODE, int KIND> __global__ void __launch_bounds__(256) langevin_flow_kernel(const FlowKArgs a)
    {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.N)
        return;
    const double4 p = load_scalar4(a.pos, idx);
    const int type = selected_type(p.w, a.ntypes, a.type_mask);
    if (type < 0)
        return;
    double4 v = load_scalar4(a.vel, idx);
    double3 acc;
    if (MODE != 1)
        {
        acc = langevin_step_two(a.s, a.gamma[type], flow_velocity<KIND>(a, p.x, p.y, p.z), a.tag[idx],
                                load_scalar4(a.net_force, idx), v);
        store_scalar4(a.accel, idx, acc.x, acc.y, acc.z, 0.0);         // :244
        }
    else
        {
        const double4 a4 = load_scalar4(a.accel, idx);
        acc = make_double3(a4.x, a4.y, a4.z);
        }
    if (MODE != 0)
        langevin_step_one(a.box, a.s.dt, a.pos, a.image, idx, p, v, acc);
    store_scalar4(a.vel, idx, v.x, v.y, v.z, v.w);
    }

// Brownian step (src/TwoStepBrownianFlow.h:134-178): x += (u(x) + (F_net + R) / gamma) dt, wrap
template<int KIND> __global__ void __launch_bounds__(256) brownian_flow_kernel(const FlowKArgs a)
    {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.N)
        return;
    const double4 p = load_scalar4(a.pos, idx);
    const int type = selected_type(p.w, a.ntypes, a.type_mask);
    if (type < 0)
        return;
    brownian_step(a.s, a.box, a.gamma[type], flow_velocity<KIND>(a, p.x, p.y, p.z), a.tag[idx], load_scalar4(a.net_force, idx),
                  a.pos, a.image, idx, p);
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
    k.s.dt = args->dt;
    k.s.kT = args->kT;
    k.s.timestep = args->timestep;
    k.p0 = args->flow.p[0]; k.p1 = args->flow.p[1]; k.p2 = args->flow.p[2];
    k.s.seed = args->seed & 0xffffu;
    k.s.noiseless = args->noiseless;
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
