// langevin.hip -- methods.Langevin and methods.Brownian (gfx950): Langevin and Brownian dynamics of the translational and,
// where the integrator integrates them, the rotational degrees of freedom. The scheme is this project's own (include/azp.h:
// azp_langevin_args); the translation is flow_methods.hip's at zero flow, through the same device functions
// (langevin_device.hpp), the quaternion arithmetic is the NVE step's (rotation.hpp).
//
// One thread per particle moves it and rotates it: type, tag and kT are read once, q, p, I and the torque once per kernel,
// also in the fused form. Scalar4 rows as two 16-byte loads. No atomics, no shared memory.
#include "langevin_device.hpp"
#include "rotation.hpp"

namespace azp
{
struct LangevinKArgs
    {
    double* pos;
    double* vel;
    double* accel;
    const double* net_force;
    int32_t* image;
    const uint32_t* tag;
    const double* gamma;
    const uint8_t* type_mask;
    double* orientation;
    double* angmom;
    const double* inertia;
    const double* net_torque;
    double* langevin_torque;
    const double* gamma_r;
    BoxDev box;
    LangevinScalars s;
    uint32_t N;
    uint32_t ntypes;
    };

enum { LANGEVIN_TWO = 0, LANGEVIN_ONE = 1, LANGEVIN_TWO_ONE = 2, BROWNIAN = 3 };

// uniform(-c_k, c_k) draws 3, 4, 5 of the particle's stream, c_k = sqrt(6 gamma_r,k kT / dt); an axis without a moment
// of inertia draws nothing (the stream is counter-based: skipping a draw moves no other)
__device__ __forceinline__ double3 rotational_draws(const LangevinScalars& s, uint32_t id, uint32_t tag, const double3& g,
                                                    const double3& I)
    {
    const uint32_t k0 = philox_key0(id, s.timestep, s.seed), k1 = (uint32_t)s.timestep;
    double3 R = make_double3(0.0, 0.0, 0.0);
    if (I.x != 0.0) R.x = uniform_draw(k0, k1, 3, tag, sqrt(6.0 * g.x * s.kT / s.dt));
    if (I.y != 0.0) R.y = uniform_draw(k0, k1, 4, tag, sqrt(6.0 * g.y * s.kT / s.dt));
    if (I.z != 0.0) R.z = uniform_draw(k0, k1, 5, tag, sqrt(6.0 * g.z * s.kT / s.dt));
    return R;
    }

// MODE LANGEVIN_TWO: step two. LANGEVIN_ONE: step one. LANGEVIN_TWO_ONE: step two of one time step, then step one of the
// next (the acceleration and the Langevin torque of step two stay in registers, q and the torque do not change between
// the halves; same functions, same operation order: bit-identical to TWO then ONE). BROWNIAN: the whole Brownian step.
template<int MODE, bool ROT> __global__ void __launch_bounds__(256) langevin_kernel(const LangevinKArgs a)
    {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.N)
        return;
    const double4 r = load_scalar4(a.pos, idx);
    const int type = selected_type(r.w, a.ntypes, a.type_mask);
    if (type < 0)
        return;
    constexpr bool DRAWS = MODE != LANGEVIN_ONE; // step two and the Brownian step read the forces, the tag and gamma
    const uint32_t tag = DRAWS ? a.tag[idx] : 0u;
    const double3 u = make_double3(0.0, 0.0, 0.0);

    // ---- translation: flow.Langevin / flow.Brownian at u = 0
    if (MODE == BROWNIAN)
        brownian_step(a.s, a.box, a.gamma[type], u, tag, load_scalar4(a.net_force, idx), a.pos, a.image, idx, r);
    else
        {
        double4 v = load_scalar4(a.vel, idx);
        double3 acc;
        if (MODE != LANGEVIN_ONE)
            {
            acc = langevin_step_two(a.s, a.gamma[type], u, tag, load_scalar4(a.net_force, idx), v);
            store_scalar4(a.accel, idx, acc.x, acc.y, acc.z, 0.0);
            }
        else
            {
            const double4 a4 = load_scalar4(a.accel, idx);
            acc = make_double3(a4.x, a4.y, a4.z);
            }
        if (MODE != LANGEVIN_TWO)
            langevin_step_one(a.box, a.s.dt, a.pos, a.image, idx, r, v, acc);
        store_scalar4(a.vel, idx, v.x, v.y, v.z, v.w);
        }
    if (!ROT)
        return;

    // ---- rotation
    const double3 I = make_double3(a.inertia[3ull * idx], a.inertia[3ull * idx + 1], a.inertia[3ull * idx + 2]);
    const double4 t4 = load_scalar4(a.net_torque, idx);
    Quat q = load_quat(a.orientation, idx);
    const double3 tb = zero_free_axes(to_body(q, t4.x, t4.y, t4.z), I);
    double3 g = make_double3(0.0, 0.0, 0.0);
    if (DRAWS)
        g = make_double3(a.gamma_r[3u * type], a.gamma_r[3u * type + 1], a.gamma_r[3u * type + 2]);
    if (MODE == BROWNIAN)
        {
        const double3 R = rotational_draws(a.s, RNG_BROWNIAN_FLOW, tag, g, I);
        const double dx = I.x != 0.0 ? (tb.x + R.x) * a.s.dt / g.x : 0.0;
        const double dy = I.y != 0.0 ? (tb.y + R.y) * a.s.dt / g.y : 0.0;
        const double dz = I.z != 0.0 ? (tb.z + R.z) * a.s.dt / g.z : 0.0;
        const double th = sqrt(dx * dx + dy * dy + dz * dz);
        if (th == 0.0)
            return; // (the identity: q keeps its bits)
        const double sn = sin(0.5 * th) / th, c = cos(0.5 * th);
        const double ex = sn * dx, ey = sn * dy, ez = sn * dz;
        // q (c, e)
        Quat n;
        n.s = q.s * c - (q.x * ex + q.y * ey + q.z * ez);
        n.x = q.s * ex + c * q.x + (q.y * ez - q.z * ey);
        n.y = q.s * ey + c * q.y + (q.z * ex - q.x * ez);
        n.z = q.s * ez + c * q.z + (q.x * ey - q.y * ex);
        const double inv = 1.0 / sqrt(n.s * n.s + n.x * n.x + n.y * n.y + n.z * n.z);
        store_scalar4(a.orientation, idx, n.s * inv, n.x * inv, n.y * inv, n.z * inv);
        return;
        }
    Quat p = load_quat(a.angmom, idx);
    double3 b;
    if (MODE != LANGEVIN_ONE)
        {
        const double3 R = rotational_draws(a.s, RNG_LANGEVIN_FLOW, tag, g, I);
        const double3 S = body_angmom(q, p);
        b.x = I.x != 0.0 ? R.x - g.x * S.x / I.x : 0.0;
        b.y = I.y != 0.0 ? R.y - g.y * S.y / I.y : 0.0;
        b.z = I.z != 0.0 ? R.z - g.z * S.z / I.z : 0.0;
        store_scalar4(a.langevin_torque, idx, b.x, b.y, b.z, 0.0);
        const double3 T = zero_free_axes(make_double3(tb.x + b.x, tb.y + b.y, tb.z + b.z), I);
        kick(p, q, T, a.s.dt);
        }
    else
        {
        const double4 b4 = load_scalar4(a.langevin_torque, idx);
        b = make_double3(b4.x, b4.y, b4.z);
        }
    if (MODE != LANGEVIN_TWO)
        {
        const double3 T = zero_free_axes(make_double3(tb.x + b.x, tb.y + b.y, tb.z + b.z), I);
        kick(p, q, T, a.s.dt);
        free_rotations(p, q, I, a.s.dt);
        store_quat(a.orientation, idx, q);
        }
    store_quat(a.angmom, idx, p);
    }

template<int MODE> static void launch_mode(bool rot, uint32_t grid, uint32_t bs, hipStream_t s, const LangevinKArgs& k)
    {
    if (rot)
        hipLaunchKernelGGL((langevin_kernel<MODE, true>), dim3(grid), dim3(bs), 0, s, k);
    else
        hipLaunchKernelGGL((langevin_kernel<MODE, false>), dim3(grid), dim3(bs), 0, s, k);
    }

static int launch_langevin(int which, const azp_langevin_args* args, void* stream)
    {
    if (!args)
        return AZP_ERROR_INVALID_ARGUMENT;
    if (args->N == 0)
        return AZP_SUCCESS;
    if (!args->d_pos || args->ntypes == 0)
        return AZP_ERROR_INVALID_ARGUMENT;
    const bool draws = which != LANGEVIN_ONE; // reads the forces, the tags and the gammas
    const bool rot = args->rotational != 0;
    if (draws && (!args->d_net_force || !args->d_tag || !args->d_gamma))
        return AZP_ERROR_INVALID_ARGUMENT;
    if (which != BROWNIAN && (!args->d_vel || !args->d_accel))
        return AZP_ERROR_INVALID_ARGUMENT;
    if (rot && (!args->d_orientation || !args->d_inertia || !args->d_net_torque || (draws && !args->d_gamma_r)))
        return AZP_ERROR_INVALID_ARGUMENT;
    if (rot && which != BROWNIAN && (!args->d_angmom || !args->d_langevin_torque))
        return AZP_ERROR_INVALID_ARGUMENT;
    if (!(args->dt > 0.0))
        return AZP_ERROR_INVALID_ARGUMENT;
    const uint32_t bs = args->block_size ? args->block_size : 256u;
    if (bs != 64 && bs != 128 && bs != 192 && bs != 256)
        return AZP_ERROR_INVALID_ARGUMENT;
    LangevinKArgs k;
    k.pos = args->d_pos;
    k.vel = args->d_vel;
    k.accel = args->d_accel;
    k.net_force = args->d_net_force;
    k.image = args->d_image;
    k.tag = args->d_tag;
    k.gamma = args->d_gamma;
    k.type_mask = args->d_type_mask;
    k.orientation = args->d_orientation;
    k.angmom = args->d_angmom;
    k.inertia = args->d_inertia;
    k.net_torque = args->d_net_torque;
    k.langevin_torque = args->d_langevin_torque;
    k.gamma_r = args->d_gamma_r;
    k.box = make_box_dev(args->box);
    k.s.dt = args->dt;
    k.s.kT = args->kT;
    k.s.timestep = args->timestep;
    k.s.seed = args->seed & 0xffffu;
    k.s.noiseless = 0;
    k.N = args->N;
    k.ntypes = args->ntypes;
    const uint32_t grid = (args->N + bs - 1) / bs;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    switch (which)
        {
        case LANGEVIN_TWO: launch_mode<LANGEVIN_TWO>(rot, grid, bs, s, k); break;
        case LANGEVIN_ONE: launch_mode<LANGEVIN_ONE>(rot, grid, bs, s, k); break;
        case LANGEVIN_TWO_ONE: launch_mode<LANGEVIN_TWO_ONE>(rot, grid, bs, s, k); break;
        default: launch_mode<BROWNIAN>(rot, grid, bs, s, k); break;
        }
    return (int)hipGetLastError();
    }
} // namespace azp

extern "C" int azp_integrate_langevin_step_one(const azp_langevin_args* args, void* stream)
    {
    return azp::launch_langevin(azp::LANGEVIN_ONE, args, stream);
    }
extern "C" int azp_integrate_langevin_step_two(const azp_langevin_args* args, void* stream)
    {
    return azp::launch_langevin(azp::LANGEVIN_TWO, args, stream);
    }
extern "C" int azp_integrate_langevin_step_two_one(const azp_langevin_args* args, void* stream)
    {
    return azp::launch_langevin(azp::LANGEVIN_TWO_ONE, args, stream);
    }
extern "C" int azp_integrate_brownian_step(const azp_langevin_args* args, void* stream)
    {
    return azp::launch_langevin(azp::BROWNIAN, args, stream);
    }
