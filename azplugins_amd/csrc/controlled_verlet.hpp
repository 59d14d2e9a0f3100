// controlled_verlet.hpp -- the kernels and the launcher of every velocity-Verlet scheme whose step is controlled by sums
// over all particles: the thermostats (thermostat.hip) and FIRE (fire.hip). DESIGN 4.18.
//
// Such a scheme needs its sums between step two of one step and step one of the next, which is where nve_kernel<2>
// fuses the two, so it has four passes of its own and a control state that never leaves the device:
//
//   cv_partial_kernel<P, false>  measure pass: per-workgroup partials of the P::NS sums of the particles as they stand
//                                (once per run)
//   cv_partial_kernel<P, true>   step two, v += (dt/2) f/m, and the partials of the new v in the same pass (vel 32 B
//                                read + 32 B written, force 32 B: 96 B per particle, plus NS partials per workgroup)
//   cv_advance_kernel<P>         one wave: fold_partials of each slot (bit for bit what reduce_fold would write), then
//                                lane 0 runs P::advance on the device-resident state
//   cv_step_one_kernel<P>        P::steer on v, v += (dt/2) f/m, x += dt v, wrap and image as nve_kernel<1> does (vel
//                                64 B, force 32 B, pos 64 B, image 24 B: 184 B per particle)
//
// A policy P holds what differs between the schemes:
//   Args, Consts              its argument struct of include/azp.h; its own constants as its kernels take them
//   NS                        the number of sums
//   SUMS_READ_FORCE           whether a term reads the force: if not, the measure pass loads (and requires) none
//   STATE_HOLDS_DT            whether step two reads the state (dt and the halt flags live there) and so requires it
//   Control                   dt and the steer's coefficients, as one thread holds them
//   control<STEER>(state, k, c)  device: fills c (the coefficients only with STEER, for step one); false: the scheme has
//                             halted and the whole grid returns, ahead of any barrier
//   add_terms(acc, v, f)      device: one particle's terms, added to the accumulators in slot order
//   steer(c, v, f)            device: what step one does to v ahead of the half kick
//   advance(state, k, N, sum) device, lane 0 alone: the sums to the next step's control state
//   valid(which, args)        host: the parameter checks of the pass `which`
//   constants(args, k)        host: its own constants into Consts
// A policy gets the state pointer and its constants, never the CVKArgs of the kernel: binding that struct to a function
// parameter keeps the compiler from proving the loads through its pointers unclobbered, and the advance's loads of the
// state turn from scalar into vector loads (profiles/controlled_verlet.md).
//
// The sums are the reproducible two-stage sum of azp_reduce.hpp: nothing is atomic, the order depends on N alone. All
// arithmetic here and in the policies is plain IEEE in the order written (no contraction), so a host restatement
// reproduces velocities, positions and partials bit for bit. nve_kernel (external_forces.hip) and the Langevin and
// Brownian kernels (flow_methods.hip) are compiled with contraction and their kicks and drifts are FMAs: sharing
// kick() or the drift with them would change the bits of one side or the other, so they stay where they are.
//
// The advance is a kernel of its own and not folded into step one: every workgroup of step one would have to fold the
// up to NS x 2048 partials itself (16 KB from L2 per slot and workgroup, 4096 workgroups at N = 2^20: 64 MB of L2 reads
// per slot against the 193 MB the pass moves) and run the serial control logic ahead of its first load; and where the
// advance reads AND writes the state (FIRE), all workgroups would have to read the old state before any wrote the new
// one. All that to save one launch of one wave.
#pragma once
#include "azp_reduce.hpp"

namespace azp
{
enum { CV_MEASURE = 0, CV_STEP_TWO = 1, CV_ADVANCE = 2, CV_STEP_ONE = 3 };

struct CVKArgs
    {
    double* pos;
    double* vel;
    const double* net_force;
    int32_t* image;
    double* partials;
    double* state;
    BoxDev box;
    uint32_t N;
    uint32_t per_lane;
    uint32_t n_blocks;
    };

#pragma clang fp contract(off)
// the half kick v += ((dt/2) f) (1/m)
__device__ __forceinline__ void kick(double4& v, const double4& f, double hdt, double minv)
    {
    v.x = v.x + (hdt * f.x) * minv;
    v.y = v.y + (hdt * f.y) * minv;
    v.z = v.z + (hdt * f.z) * minv;
    }

template<class P, bool STEP_TWO> __global__ void __launch_bounds__(REDUCE_BLOCK) cv_partial_kernel(const CVKArgs a, const typename P::Consts k)
    {
    __shared__ double s_wave[REDUCE_WAVES * P::NS];
    const uint32_t tid = threadIdx.x;
    typename P::Control c;
    if (STEP_TWO && !P::template control<false>(a.state, k, c))
        return;
    const double hdt = STEP_TWO ? 0.5 * c.dt : 0.0;
    double acc[P::NS] = {}; // +0.0
    const uint64_t base = (uint64_t)blockIdx.x * REDUCE_BLOCK * a.per_lane;
    // (the bound is the same for every thread: all 64 lanes of a wave reach the butterfly)
    for (uint32_t j = 0; j < a.per_lane; ++j)
        {
        const uint64_t i64 = base + (uint64_t)j * REDUCE_BLOCK + tid;
        if (i64 >= a.N)
            continue;
        const uint32_t i = (uint32_t)i64;
        double4 v = load_scalar4(a.vel, i);
        double4 f = make_double4(0.0, 0.0, 0.0, 0.0);
        if (STEP_TWO || P::SUMS_READ_FORCE)
            f = load_scalar4(a.net_force, i);
        if (STEP_TWO)
            {
            kick(v, f, hdt, 1.0 / v.w);
            store_scalar4(a.vel, i, v.x, v.y, v.z, v.w);
            }
        P::add_terms(acc, v, f);
        }
    reduce_block_store<P::NS>(acc, s_wave, a.partials, 0, gridDim.x, blockIdx.x);
    }

template<class P> __global__ void __launch_bounds__(256) cv_step_one_kernel(const CVKArgs a, const typename P::Consts k)
    {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.N)
        return;
    typename P::Control c;
    if (!P::template control<true>(a.state, k, c))
        return;
    double4 v = load_scalar4(a.vel, idx);
    const double4 f = load_scalar4(a.net_force, idx);
    const double minv = 1.0 / v.w; // (ahead of the steer: the division starts as soon as the mass has arrived)
    P::steer(c, v, f);
    kick(v, f, 0.5 * c.dt, minv);
    store_scalar4(a.vel, idx, v.x, v.y, v.z, v.w);
    const double4 p = load_scalar4(a.pos, idx);
    double x = p.x + c.dt * v.x, y = p.y + c.dt * v.y, z = p.z + c.dt * v.z;
    wrap_with_image(a.box, x, y, z, a.image, idx);
    store_scalar4(a.pos, idx, x, y, z, p.w);
    }

template<class P> __global__ void __launch_bounds__(WAVE) cv_advance_kernel(const CVKArgs a, const typename P::Consts k)
    {
    double sum[P::NS];
#pragma unroll
    for (uint32_t k = 0; k < P::NS; ++k)
        sum[k] = fold_partials(a.partials + (uint64_t)k * a.n_blocks, a.n_blocks, threadIdx.x);
    if (threadIdx.x == 0)
        P::advance(a.state, k, a.N, sum);
    }
#pragma clang fp contract(on)

// Every refusal is AZP_ERROR_INVALID_ARGUMENT. The image array may be null (wrap_with_image).
template<class P> static int launch_cv(int which, const typename P::Args* args, void* stream)
    {
    if (!args || args->N == 0)
        return AZP_ERROR_INVALID_ARGUMENT;
    const ReduceShape shape = reduce_shape(args->N);
    const bool kicks = which == CV_STEP_TWO || which == CV_STEP_ONE;
    if (which != CV_STEP_ONE && (!args->d_partials || args->partials_bytes < (uint64_t)P::NS * shape.n_blocks * sizeof(double)))
        return AZP_ERROR_INVALID_ARGUMENT;
    if (which != CV_ADVANCE && !args->d_vel)
        return AZP_ERROR_INVALID_ARGUMENT;
    if ((kicks || (which == CV_MEASURE && P::SUMS_READ_FORCE)) && !args->d_net_force)
        return AZP_ERROR_INVALID_ARGUMENT;
    if (which == CV_STEP_ONE && !args->d_pos)
        return AZP_ERROR_INVALID_ARGUMENT;
    if ((which == CV_ADVANCE || which == CV_STEP_ONE || (which == CV_STEP_TWO && P::STATE_HOLDS_DT)) && !args->d_state)
        return AZP_ERROR_INVALID_ARGUMENT;
    if (!P::valid(which, *args))
        return AZP_ERROR_INVALID_ARGUMENT;
    CVKArgs k;
    k.pos = args->d_pos;
    k.vel = args->d_vel;
    k.net_force = args->d_net_force;
    k.image = args->d_image;
    k.partials = args->d_partials;
    k.state = args->d_state;
    k.box = make_box_dev(args->box);
    k.N = args->N;
    k.per_lane = shape.per_lane;
    k.n_blocks = shape.n_blocks;
    typename P::Consts c;
    P::constants(*args, c);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    switch (which)
        {
        case CV_MEASURE:
            hipLaunchKernelGGL((cv_partial_kernel<P, false>), dim3(shape.n_blocks), dim3(REDUCE_BLOCK), 0, s, k, c);
            break;
        case CV_STEP_TWO:
            hipLaunchKernelGGL((cv_partial_kernel<P, true>), dim3(shape.n_blocks), dim3(REDUCE_BLOCK), 0, s, k, c);
            break;
        case CV_ADVANCE:
            hipLaunchKernelGGL(cv_advance_kernel<P>, dim3(1), dim3(WAVE), 0, s, k, c);
            break;
        default:
            hipLaunchKernelGGL(cv_step_one_kernel<P>, dim3((args->N + 255u) / 256u), dim3(256), 0, s, k, c);
            break;
        }
    return (int)hipGetLastError();
    }

template<class P> static int cv_partials_size(uint32_t N, uint64_t* bytes)
    {
    if (!bytes || N == 0)
        return AZP_ERROR_INVALID_ARGUMENT;
    *bytes = (uint64_t)P::NS * reduce_shape(N).n_blocks * sizeof(double);
    return AZP_SUCCESS;
    }
} // namespace azp
