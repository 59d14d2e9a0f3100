// aniso_forces.hip -- anisotropic pair force + torque for the two-patch Morse
// potential. Replaces HOOMD's
// gpu_compute_pair_aniso_forces<AnisoPairEvaluatorTwoPatchMorse>, requested by
// the reference at src/AnisoPotentialPairGPUKernel.cu.inc:21-25; per-pair
// arithmetic restated from src/AnisoPairEvaluatorTwoPatchMorse.h:127-216.
//
// The policy XTPM drives the tile-staged xtiled_kernel (xtiled.hpp) and the generic
// pair_forces_kernel (pair_kernel.hpp).
// The patch director n = rotate(q, x^) of particle i is computed once per
// particle, that of a neighbor once per tile (tile kernel) or per in-range pair
// (generic kernel). Outputs: force (fx, fy, fz, e) and torque (tx, ty, tz, 0),
// both N x 4.
#include "pair_auto.hpp"

namespace azp
{
struct TPMCoeff
    {
    double rcutsq, M_d, M_rinv, r_eq, omega, alpha, U_shift; // U_shift = U_Morse(r_cut) when mode == shift
    int repulsion, _pad;
    };

__device__ __forceinline__ TPMCoeff tpm_prepare(const azp_tpm_params& p, double rcutsq, bool energy_shift)
    {
    TPMCoeff c;
    c.rcutsq = rcutsq;
    c.M_d = p.M_d;
    c.M_rinv = p.M_rinv;
    c.r_eq = p.r_eq;
    c.omega = p.omega;
    c.alpha = p.alpha;
    c.repulsion = p.repulsion ? 1 : 0;
    c._pad = 0;
    c.U_shift = 0.0;
    if (energy_shift)
        {
        const double rcut = sqrt(rcutsq);
        const double ex = exp(-(rcut - p.r_eq) * p.M_rinv);
        const double om = 1.0 - ex;
        c.U_shift = p.M_d * (om * om - 1.0);
        }
    return c;
    }

// rotate(q, (1,0,0)) with q = (s, u): (s^2 - |u|^2) x^ + 2 s (u x x^) + 2 u_x u
__device__ __forceinline__ double3 patch_director(const double4& q)
    {
    const double s = q.x, ux = q.y, uy = q.z, uz = q.w;
    const double c = s * s - (ux * ux + uy * uy + uz * uz);
    return make_double3(c + 2.0 * ux * ux, 2.0 * s * uz + 2.0 * ux * uy, -2.0 * s * uy + 2.0 * ux * uz);
    }

// One TwoPatchMorse pair (src/AnisoPairEvaluatorTwoPatchMorse.h:127-215): force on i, the torque on i (before its
// accumulation), the pair energy. U = (U_Morse(r) - U_shift) Omega(gamma_i) Omega(gamma_j), gamma = u . n, u = dr / r,
// Omega(g) = 1 / (1 + exp(-omega (g^2 - alpha))). Written for the FP64 issue rate of gfx950: one reciprocal square
// root gives r and 1 / r; the reciprocals of the two sigmoid denominators are Newton-refined v_rcp_f64; and the
// perpendicular directors n_perp = -u x (u x n) = n - gamma u are never formed -- the force is assembled as
// F = a u + b_i n_i + b_j n_j with three scalar coefficients (9 FMAs instead of two double cross products).
__device__ __forceinline__ void tpm_pair(const TPMCoeff& c, const double3& n_i, const double3& n_j, double dx, double dy, double dz,
                                         double rsq, double (&F)[3], double (&T)[3], double& e)
    {
    const double rinv = fast_rsqrt(rsq);
    const double r = rsq * rinv;
    const double ux = dx * rinv, uy = dy * rinv, uz = dz * rinv;
    double UMorse = -c.M_d;
    double dUMorse_dr = 0.0;
    if (r > c.r_eq || c.repulsion)
        {
        const double Morse_exp = exp(-(r - c.r_eq) * c.M_rinv);
        const double one_minus_exp = 1.0 - Morse_exp;
        UMorse = c.M_d * __builtin_fma(one_minus_exp, one_minus_exp, -1.0);
        dUMorse_dr = 2.0 * c.M_d * c.M_rinv * Morse_exp * one_minus_exp;
        }
    const double gi = __builtin_fma(uz, n_i.z, __builtin_fma(uy, n_i.y, ux * n_i.x));
    const double gj = __builtin_fma(uz, n_j.z, __builtin_fma(uy, n_j.y, ux * n_j.x));
    const double ei = exp(-c.omega * __builtin_fma(gi, gi, -c.alpha));
    const double ej = exp(-c.omega * __builtin_fma(gj, gj, -c.alpha));
    const double Oi = fast_rcp(1.0 + ei), Oj = fast_rcp(1.0 + ej);
    const double OO = Oi * Oj;
    e = (UMorse - c.U_shift) * OO;
    const double w2 = 2.0 * c.omega * UMorse * OO;   // dU/dgamma_i = w2 gamma_i e_i Omega_i, likewise j
    const double dU_dgi = w2 * gi * ei * Oi;
    const double dU_dgj = w2 * gj * ej * Oj;
    const double bi = -rinv * dU_dgi, bj = -rinv * dU_dgj;
    const double a = -__builtin_fma(bi, gi, __builtin_fma(bj, gj, dUMorse_dr * OO));
    F[0] = __builtin_fma(a, ux, __builtin_fma(bi, n_i.x, bj * n_j.x));
    F[1] = __builtin_fma(a, uy, __builtin_fma(bi, n_i.y, bj * n_j.y));
    F[2] = __builtin_fma(a, uz, __builtin_fma(bi, n_i.z, bj * n_j.z));
    // torque on i: dU/dgamma_i (u x n_i)
    T[0] = dU_dgi * __builtin_fma(uy, n_i.z, -uz * n_i.y);
    T[1] = dU_dgi * __builtin_fma(uz, n_i.x, -ux * n_i.z);
    T[2] = dU_dgi * __builtin_fma(ux, n_i.y, -uy * n_i.x);
    }

// TwoPatchMorse as a policy: the tile kernel computes the patch director n_j = rotate(q_j, x^) of
// every staged particle ONCE per tile and keeps it in LDS next to its position (the reference rotates per pair,
// src/AnisoPairEvaluatorTwoPatchMorse.h:145-146); the generic kernel computes it per in-range pair
struct XTPM
    {
    typedef azp_tpm_params Params;
    typedef TPMCoeff Coeff;
    struct KExtra
        {
        const double* orientation;
        double* torque;
        };
    static constexpr int kExtra = 3; // n_j
    static constexpr bool kTag = false;
    static constexpr int kMinWaves = 3; // 48 B per slot: three workgroups per CU at 1,024 slots, <= 168 VGPRs
    struct Own
        {
        double3 n;
        };
    struct Acc
        {
        double f[3], t[3], pe;
        };
    static __device__ __forceinline__ Coeff prepare(const Params* params, const PairKArgs& a, uint32_t t, const KExtra&)
        {
        return tpm_prepare(params[t], a.rcutsq[t], a.shift_mode == AZP_SHIFT_SHIFT);
        }
    static __device__ __forceinline__ void load_extra(const KExtra& x, uint32_t j, double (&e)[3], uint32_t&)
        {
        const double3 n = patch_director(load_scalar4(x.orientation, j));
        e[0] = n.x; e[1] = n.y; e[2] = n.z;
        }
    static __device__ __forceinline__ void load_own(const KExtra& x, uint32_t idx, Own& o)
        {
        o.n = patch_director(load_scalar4(x.orientation, idx));
        }
    static __device__ __forceinline__ void zero(Acc& a)
        {
        a.f[0] = a.f[1] = a.f[2] = a.t[0] = a.t[1] = a.t[2] = a.pe = 0.0;
        }
    template<int TPP> static __device__ __forceinline__ void reduce(Acc& a)
        {
#pragma unroll
        for (int c = 0; c < 3; ++c)
            {
            a.f[c] = group_sum<TPP>(a.f[c]);
            a.t[c] = group_sum<TPP>(a.t[c]);
            }
        a.pe = group_sum<TPP>(a.pe);
        }
    static __device__ __forceinline__ bool in_range(const Coeff& c, double rsq) { return !(rsq > c.rcutsq); } // (:135-136)
    template<bool VIRIAL>
    static __device__ __forceinline__ void pair(const Coeff& c, const KExtra&, const Own& o, double dx, double dy, double dz, double rsq,
                                                const double (&nj)[3], uint32_t, Acc& a, double (&v)[6])
        {
        const double3 n_i = o.n;
        const double3 n_j = make_double3(nj[0], nj[1], nj[2]);
        double F[3], T[3], e;
        tpm_pair(c, n_i, n_j, dx, dy, dz, rsq, F, T, e);
        const double Fx = F[0], Fy = F[1], Fz = F[2];
        a.f[0] += Fx; a.f[1] += Fy; a.f[2] += Fz;
        a.t[0] += T[0]; a.t[1] += T[1]; a.t[2] += T[2];
        a.pe += e;
        if (VIRIAL)
            {
            v[0] = __builtin_fma(dx, Fx, v[0]);
            v[1] = __builtin_fma(dy, Fx, v[1]);
            v[2] = __builtin_fma(dz, Fx, v[2]);
            v[3] = __builtin_fma(dy, Fy, v[3]);
            v[4] = __builtin_fma(dz, Fy, v[4]);
            v[5] = __builtin_fma(dz, Fz, v[5]);
            }
        }
    static __device__ __forceinline__ void store(const Acc& a, const PairKArgs& p, const KExtra& x, uint32_t idx)
        {
        store_scalar4(p.force, idx, a.f[0], a.f[1], a.f[2], 0.5 * a.pe);
        store_scalar4(x.torque, idx, a.t[0], a.t[1], a.t[2], 0.0);
        }
    static int validate(const azp_aniso_args* args, const azp_tpm_params* d_params)
        {
        if (!args)
            return AZP_ERROR_INVALID_ARGUMENT;
        const int bad = validate_pair_args(&args->pair, d_params);
        if (bad != 0)
            return bad;
        if (!args->d_orientation || !args->d_torque || args->pair.shift_mode == AZP_SHIFT_XPLOR)
            return AZP_ERROR_INVALID_ARGUMENT; // HOOMD aniso pairs accept "none" / "shift"
        return 0;
        }
    static KExtra extra(const azp_aniso_args& args)
        {
        KExtra x;
        x.orientation = args.d_orientation;
        x.torque = args.d_torque;
        return x;
        }
    };
} // namespace azp

extern "C" int azp_aniso_forces_planned_two_patch_morse(azp_pair_plan* plan, const azp_aniso_args* args, const azp_tpm_params* d_params,
                                                        void* stream)
    {
    return azp::launch_policy_planned<azp::XTPM>(plan, args, d_params, stream);
    }

// what gpu_compute_pair_aniso_forces<E> forwards to (src/AnisoPotentialPairGPUKernel.cu.inc:21-25)
extern "C" int azp_aniso_forces_two_patch_morse(const azp_aniso_args* args, const azp_tpm_params* d_params, void* stream)
    {
    return azp::launch_policy_entry<azp::XTPM>(args, d_params, stream);
    }
