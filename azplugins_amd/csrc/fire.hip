// fire.hip -- energy minimization (azplugins_amd.minimize.FIRE; name and parameter keys of hoomd.md.minimize.FIRE).
// HOOMD-blue's source is not available here: the scheme is DEFINED in include/azp.h and DESIGN 4.19, and
// tests/fire_ref.py restates it in numpy.
//
// FIRE is velocity Verlet whose velocities are mixed with the force direction ahead of step one and whose time step
// adapts to the sign of the power P = f . v. It has the shape of the thermostatted step (thermostat.hip) with more in
// it: four sums (P, |v|^2, |f|^2, U) instead of one, and a device-resident control state that holds the time step
// itself, so dt does not travel by value in the argument struct as it does in every other integrator here.
//
//   fire_partial<false>  measure pass: per-workgroup partials of the four sums of v and f as they stand (once per run;
//                        vel 32 B + force 32 B read: 64 B per particle, plus the partials)
//   fire_partial<true>   step two, v += (DT/2) f/m with DT from the state, and the partials of the new v and of f in
//                        the same pass (vel 32 B read + 32 B written, force 32 B: 96 B per particle, plus 4 partials
//                        per workgroup)
//   fire_advance         one wave: folds the four slots in reduce_fold's order, tests for convergence, computes the
//                        two velocity coefficients and the next DT and ALPHA, updates the device-resident state
//   fire_step_one        reads DT, KEEP, MIX from the state: v = KEEP v + MIX f, v += (DT/2) f/m, x += DT v, wrap and
//                        image as nve_kernel<1> does (vel 64 B, force 32 B, pos 64 B, image 24 B: 184 B per particle)
//
// Once the state says converged (or that a sum was not finite) every kernel returns at its first instruction after
// reading the flags: positions stop moving, and a run that goes on costs launches alone.
//
// The sums are the reproducible two-stage sum of azp_reduce.hpp: nothing is atomic, the order depends on N alone. All
// arithmetic here is plain IEEE in the order written (no contraction), and the advance uses + * / sqrt min alone, all
// correctly rounded: a host restatement reproduces every bit.
//
// The advance is a kernel of its own and not folded into step one, for the reason given in thermostat.hip with four
// times the weight: every workgroup of step one would fold up to 4 x 2048 partials itself (64 KB from L2 per
// workgroup, 4096 workgroups at N = 2^20: 256 MB of L2 reads against the 193 MB the pass moves), and all of them would
// have to agree on who writes the new state after the last one has read the old, to save one launch of one wave.
#include <cmath>

#include "azp_reduce.hpp"

namespace azp
{
struct FireKArgs
    {
    double* pos;
    double* vel;
    const double* net_force;
    int32_t* image;
    double* partials;
    double* state;
    BoxDev box;
    double dt_max;
    double force_tol;
    double energy_tol;
    double finc_dt;
    double fdec_dt;
    double alpha_start;
    double fdec_alpha;
    double min_steps_adapt;
    double min_steps_conv;
    uint32_t N;
    uint32_t per_lane;
    uint32_t n_blocks;
    };

#pragma clang fp contract(off)
template<bool STEP_TWO> __global__ void __launch_bounds__(REDUCE_BLOCK) fire_partial(const FireKArgs a)
    {
    __shared__ double s_wave[REDUCE_WAVES * AZP_FIRE_NSLOTS];
    const uint32_t tid = threadIdx.x;
    double hdt = 0.0;
    if (STEP_TWO)
        {
        // (the same for every thread of the grid: all leave together, ahead of the barrier)
        if (a.state[AZP_FIRE_CONVERGED] != 0.0 || a.state[AZP_FIRE_NONFINITE] != 0.0)
            return;
        hdt = 0.5 * a.state[AZP_FIRE_DT];
        }
    double acc[AZP_FIRE_NSLOTS] = {0.0, 0.0, 0.0, 0.0};
    const uint64_t base = (uint64_t)blockIdx.x * REDUCE_BLOCK * a.per_lane;
    // (the bound is the same for every thread: all 64 lanes of a wave reach the butterfly)
    for (uint32_t j = 0; j < a.per_lane; ++j)
        {
        const uint64_t i64 = base + (uint64_t)j * REDUCE_BLOCK + tid;
        if (i64 >= a.N)
            continue;
        const uint32_t i = (uint32_t)i64;
        double4 v = load_scalar4(a.vel, i);
        const double4 f = load_scalar4(a.net_force, i);
        if (STEP_TWO)
            {
            const double minv = 1.0 / v.w;
            v.x = v.x + (hdt * f.x) * minv;
            v.y = v.y + (hdt * f.y) * minv;
            v.z = v.z + (hdt * f.z) * minv;
            store_scalar4(a.vel, i, v.x, v.y, v.z, v.w);
            }
        acc[0] += ((f.x * v.x) + (f.y * v.y)) + (f.z * v.z);
        acc[1] += ((v.x * v.x) + (v.y * v.y)) + (v.z * v.z);
        acc[2] += ((f.x * f.x) + (f.y * f.y)) + (f.z * f.z);
        acc[3] += f.w;
        }
    reduce_block_store<AZP_FIRE_NSLOTS>(acc, s_wave, a.partials, 0, gridDim.x, blockIdx.x);
    }

__global__ void __launch_bounds__(256) fire_step_one(const FireKArgs a)
    {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.N)
        return;
    if (a.state[AZP_FIRE_CONVERGED] != 0.0 || a.state[AZP_FIRE_NONFINITE] != 0.0)
        return;
    const double dt = a.state[AZP_FIRE_DT], keep = a.state[AZP_FIRE_KEEP], mix = a.state[AZP_FIRE_MIX];
    double4 v = load_scalar4(a.vel, idx);
    const double4 f = load_scalar4(a.net_force, idx);
    const double minv = 1.0 / v.w;
    const double hdt = 0.5 * dt;
    v.x = (keep * v.x) + (mix * f.x);
    v.y = (keep * v.y) + (mix * f.y);
    v.z = (keep * v.z) + (mix * f.z);
    v.x = v.x + (hdt * f.x) * minv;
    v.y = v.y + (hdt * f.y) * minv;
    v.z = v.z + (hdt * f.z) * minv;
    store_scalar4(a.vel, idx, v.x, v.y, v.z, v.w);
    const double4 p = load_scalar4(a.pos, idx);
    double x = p.x + dt * v.x, y = p.y + dt * v.y, z = p.z + dt * v.z;
    wrap_with_image(a.box, x, y, z, a.image, idx);
    store_scalar4(a.pos, idx, x, y, z, p.w);
    }

__global__ void __launch_bounds__(WAVE) fire_advance(const FireKArgs a)
    {
    const uint32_t lane = threadIdx.x;
    // reduce_fold's order, slot-major: lane l adds the partials l, l + 64, ... in turn from +0.0, then the butterfly
    double sum[AZP_FIRE_NSLOTS];
#pragma unroll
    for (uint32_t k = 0; k < AZP_FIRE_NSLOTS; ++k)
        {
        const double* row = a.partials + (uint64_t)k * a.n_blocks;
        double s = 0.0;
#pragma unroll 8
        for (uint32_t b = lane; b < a.n_blocks; b += WAVE)
            s += row[b];
        sum[k] = group_sum<WAVE>(s);
        }
    if (lane != 0)
        return;
    double* s = a.state;
    if (s[AZP_FIRE_CONVERGED] != 0.0 || s[AZP_FIRE_NONFINITE] != 0.0)
        return;
    const double P = sum[0], VV = sum[1], FF = sum[2], U = sum[3];
    if (!(isfinite(P) && isfinite(VV) && isfinite(FF) && isfinite(U)))
        {
        s[AZP_FIRE_NONFINITE] = 1.0;
        s[AZP_FIRE_KEEP] = 0.0;
        s[AZP_FIRE_MIX] = 0.0;
        return;
        }
    s[AZP_FIRE_P] = P;
    s[AZP_FIRE_VV] = VV;
    s[AZP_FIRE_FF] = FF;
    s[AZP_FIRE_U] = U;
    const double n = (double)a.N;
    const double n_steps = s[AZP_FIRE_N_STEPS];
    const double conv_after = a.min_steps_conv > 1.0 ? a.min_steps_conv : 1.0;
    if (n_steps >= conv_after && sqrt(FF / (3.0 * n)) < a.force_tol && fabs(U - s[AZP_FIRE_U_PREV]) / n < a.energy_tol)
        {
        s[AZP_FIRE_CONVERGED] = 1.0;
        s[AZP_FIRE_KEEP] = 0.0;
        s[AZP_FIRE_MIX] = 0.0;
        return;
        }
    double dt = s[AZP_FIRE_DT], alpha = s[AZP_FIRE_ALPHA], n_pos = s[AZP_FIRE_N_POS];
    double keep = 1.0 - alpha;
    double mix = FF > 0.0 ? alpha * (sqrt(VV) / sqrt(FF)) : 0.0;
    if (P > 0.0)
        {
        n_pos = n_pos + 1.0;
        if (n_pos > a.min_steps_adapt)
            {
            const double grown = dt * a.finc_dt;
            dt = grown < a.dt_max ? grown : a.dt_max;
            alpha = alpha * a.fdec_alpha;
            }
        }
    else
        {
        dt = dt * a.fdec_dt;
        alpha = a.alpha_start;
        n_pos = 0.0;
        keep = 0.0;
        mix = 0.0;
        }
    s[AZP_FIRE_DT] = dt;
    s[AZP_FIRE_ALPHA] = alpha;
    s[AZP_FIRE_KEEP] = keep;
    s[AZP_FIRE_MIX] = mix;
    s[AZP_FIRE_N_POS] = n_pos;
    s[AZP_FIRE_U_PREV] = U;
    s[AZP_FIRE_N_STEPS] = n_steps + 1.0;
    }
#pragma clang fp contract(on)

enum { FIRE_MEASURE = 0, FIRE_STEP_TWO = 1, FIRE_ADVANCE = 2, FIRE_STEP_ONE = 3 };

static bool fire_in_unit_interval(double x) { return x > 0.0 && x < 1.0; }

static int launch_fire(int which, const azp_fire_args* args, void* stream)
    {
    if (!args || args->N == 0)
        return AZP_ERROR_INVALID_ARGUMENT;
    const ReduceShape shape = reduce_shape(args->N);
    const uint64_t need = (uint64_t)AZP_FIRE_NSLOTS * shape.n_blocks * sizeof(double);
    if (which != FIRE_STEP_ONE && (!args->d_partials || args->partials_bytes < need))
        return AZP_ERROR_INVALID_ARGUMENT;
    if (which != FIRE_ADVANCE && (!args->d_vel || !args->d_net_force))
        return AZP_ERROR_INVALID_ARGUMENT;
    if (which == FIRE_STEP_ONE && !args->d_pos)
        return AZP_ERROR_INVALID_ARGUMENT;
    if (which != FIRE_MEASURE && !args->d_state)
        return AZP_ERROR_INVALID_ARGUMENT;
    if (which == FIRE_ADVANCE)
        {
        // (a comparison with a NaN is false, and an infinite value is refused by name)
        if (!(args->dt_max > 0.0) || !(args->force_tol > 0.0) || !(args->energy_tol > 0.0) || !(args->finc_dt > 1.0))
            return AZP_ERROR_INVALID_ARGUMENT;
        if (std::isinf(args->dt_max) || std::isinf(args->force_tol) || std::isinf(args->energy_tol) || std::isinf(args->finc_dt))
            return AZP_ERROR_INVALID_ARGUMENT;
        if (!fire_in_unit_interval(args->fdec_dt) || !fire_in_unit_interval(args->alpha_start) || !fire_in_unit_interval(args->fdec_alpha))
            return AZP_ERROR_INVALID_ARGUMENT;
        }
    FireKArgs k;
    k.pos = args->d_pos;
    k.vel = args->d_vel;
    k.net_force = args->d_net_force;
    k.image = args->d_image;
    k.partials = args->d_partials;
    k.state = args->d_state;
    k.box = make_box_dev(args->box);
    k.dt_max = args->dt_max;
    k.force_tol = args->force_tol;
    k.energy_tol = args->energy_tol;
    k.finc_dt = args->finc_dt;
    k.fdec_dt = args->fdec_dt;
    k.alpha_start = args->alpha_start;
    k.fdec_alpha = args->fdec_alpha;
    k.min_steps_adapt = (double)args->min_steps_adapt;
    k.min_steps_conv = (double)args->min_steps_conv;
    k.N = args->N;
    k.per_lane = shape.per_lane;
    k.n_blocks = shape.n_blocks;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    switch (which)
        {
        case FIRE_MEASURE:
            hipLaunchKernelGGL(fire_partial<false>, dim3(shape.n_blocks), dim3(REDUCE_BLOCK), 0, s, k);
            break;
        case FIRE_STEP_TWO:
            hipLaunchKernelGGL(fire_partial<true>, dim3(shape.n_blocks), dim3(REDUCE_BLOCK), 0, s, k);
            break;
        case FIRE_ADVANCE:
            hipLaunchKernelGGL(fire_advance, dim3(1), dim3(WAVE), 0, s, k);
            break;
        default:
            hipLaunchKernelGGL(fire_step_one, dim3((args->N + 255u) / 256u), dim3(256), 0, s, k);
            break;
        }
    return (int)hipGetLastError();
    }
} // namespace azp

extern "C" int azp_fire_partials_size(uint32_t N, uint64_t* bytes)
    {
    if (!bytes || N == 0)
        return AZP_ERROR_INVALID_ARGUMENT;
    *bytes = (uint64_t)AZP_FIRE_NSLOTS * azp::reduce_shape(N).n_blocks * sizeof(double);
    return AZP_SUCCESS;
    }
extern "C" int azp_fire_measure(const azp_fire_args* args, void* stream)
    {
    return azp::launch_fire(azp::FIRE_MEASURE, args, stream);
    }
extern "C" int azp_fire_step_two(const azp_fire_args* args, void* stream)
    {
    return azp::launch_fire(azp::FIRE_STEP_TWO, args, stream);
    }
extern "C" int azp_fire_advance(const azp_fire_args* args, void* stream)
    {
    return azp::launch_fire(azp::FIRE_ADVANCE, args, stream);
    }
extern "C" int azp_fire_step_one(const azp_fire_args* args, void* stream)
    {
    return azp::launch_fire(azp::FIRE_STEP_ONE, args, stream);
    }
