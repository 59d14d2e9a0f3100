// dpd_forces.hip -- DPD thermostat pair force (conservative + drag + random),
// generalized weight (1 - r/rc)^s. Replaces HOOMD's
// gpu_compute_dpd_forces<DPDPairEvaluatorGeneralWeight>, requested by the
// reference at src/PotentialPairDPDThermoGPUKernel.cu.inc:21-24; per-pair
// arithmetic restated from src/DPDPairEvaluatorGeneralWeight.h:198-255.
//
// The policy XDPD drives the tile-staged xtiled_kernel (xtiled.hpp) and the generic
// pair_forces_kernel (pair_kernel.hpp).
// Per neighbor: velocity (24 B) and tag (4 B). One Philox4x32-10 block per
// in-range pair, computed in registers, keyed by (seed, timestep, min tag,
// max tag) so both owners of a pair draw the same number (cross-rank
// consistency relies on this: :213-231).
#include "pair_auto.hpp"

namespace azp
{
struct DPDCoeff
    {
    double rcutsq, A, gamma, half_s, rcut, rcutinv, noise; // noise = rsqrt(dt / (6 kT gamma))
    };

__device__ __forceinline__ DPDCoeff dpd_prepare(const azp_dpd_params& p, double rcutsq, double deltaT, double T)
    {
    DPDCoeff c;
    c.rcutsq = rcutsq;
    c.A = p.A;
    c.gamma = p.gamma;
    c.half_s = 0.5 * p.s;
    c.rcutinv = 1.0 / sqrt(rcutsq);
    c.rcut = 1.0 / c.rcutinv;
    // fast::rsqrt(m_deltaT / (m_T * gamma * 6)) (:246); T == 0 -> rsqrt(inf) = 0
    c.noise = 1.0 / sqrt(deltaT / (T * p.gamma * 6.0));
    return c;
    }

// (1 - r/rc)^(s/2): the common exponents avoid the generic pow()
__device__ __forceinline__ double weight_pow(double x, double half_s)
    {
    if (half_s == 1.0) return x;
    if (half_s == 0.5) return fast_sqrt(x);
    if (half_s == 0.25) return fast_sqrt(fast_sqrt(x));
    return pow(x, half_s);
    }

// the DPD thermostat as a policy: the tile kernel stages positions, velocities and tags of a tile's neighbors once in
// LDS, the generic kernel loads a neighbor's velocity and tag per in-range pair
struct XDPD : ForceEnergy
    {
    typedef azp_dpd_params Params;
    typedef DPDCoeff Coeff;
    struct KExtra
        {
        const double* vel;
        const uint32_t* tag;
        uint64_t timestep;
        double deltaT, T;
        uint32_t seed, _pad;
        };
    static constexpr int kExtra = 3; // vx, vy, vz
    static constexpr bool kTag = true;
    static constexpr int kMinWaves = 2; // 52 B per slot: two workgroups per CU at 1,536 slots (80 KiB of LDS each)
    struct Own
        {
        double3 v;
        uint32_t tag;
        };
    static __device__ __forceinline__ Coeff prepare(const Params* params, const PairKArgs& a, uint32_t t, const KExtra& x)
        {
        return dpd_prepare(params[t], a.rcutsq[t], x.deltaT, x.T);
        }
    static __device__ __forceinline__ void load_extra(const KExtra& x, uint32_t j, double (&e)[3], uint32_t& tag)
        {
        const double3 vj = load_scalar3_of4(x.vel, j);
        e[0] = vj.x; e[1] = vj.y; e[2] = vj.z;
        tag = x.tag[j];
        }
    static __device__ __forceinline__ void load_own(const KExtra& x, uint32_t idx, Own& o)
        {
        o.v = load_scalar3_of4(x.vel, idx);
        o.tag = x.tag[idx];
        }
    static __device__ __forceinline__ bool in_range(const Coeff& c, double rsq) { return rsq < c.rcutsq; }
    template<bool VIRIAL>
    static __device__ __forceinline__ void pair(const Coeff& c, const KExtra& x, const Own& o, double dx, double dy, double dz, double rsq,
                                                const double (&vj)[3], uint32_t tagj, Acc& a, double (&v)[6])
        {
        const double rdotv = dx * (o.v.x - vj[0]) + dy * (o.v.y - vj[1]) + dz * (o.v.z - vj[2]);
        const double alpha = dpd_alpha((uint16_t)x.seed, o.tag, tagj, x.timestep);
        const double rinv = fast_rsqrt(rsq);
        const double r = rsq * rinv;
        const double force_divr_cons = c.A * (rinv - c.rcutinv);
        const double wR = weight_pow(1.0 - r * c.rcutinv, c.half_s) * rinv;
        double force_divr = force_divr_cons - c.gamma * wR * wR * rdotv;
        force_divr += c.noise * wR * alpha;
        a.fx = __builtin_fma(dx, force_divr, a.fx);
        a.fy = __builtin_fma(dy, force_divr, a.fy);
        a.fz = __builtin_fma(dz, force_divr, a.fz);
        a.pe += c.A * (c.rcut - r) - 0.5 * c.A * c.rcutinv * (c.rcutsq - rsq);
        if (VIRIAL)
            {
            const double fxx = force_divr_cons * dx, fyy = force_divr_cons * dy;
            v[0] = __builtin_fma(fxx, dx, v[0]);
            v[1] = __builtin_fma(fxx, dy, v[1]);
            v[2] = __builtin_fma(fxx, dz, v[2]);
            v[3] = __builtin_fma(fyy, dy, v[3]);
            v[4] = __builtin_fma(fyy, dz, v[4]);
            v[5] = __builtin_fma(force_divr_cons * dz, dz, v[5]);
            }
        }
    static int validate(const azp_dpd_args* args, const azp_dpd_params* d_params)
        {
        if (!args)
            return AZP_ERROR_INVALID_ARGUMENT;
        const int bad = validate_pair_args(&args->pair, d_params);
        if (bad != 0)
            return bad;
        if (!args->d_vel || !args->d_tag || args->pair.shift_mode != AZP_SHIFT_NONE)
            return AZP_ERROR_INVALID_ARGUMENT; // DPD accepts mode "none" only (src/pair.py:215)
        return 0;
        }
    static KExtra extra(const azp_dpd_args& args)
        {
        KExtra x;
        x.vel = args.d_vel; x.tag = args.d_tag; x.timestep = args.timestep; x.deltaT = args.deltaT; x.T = args.T;
        x.seed = args.seed; x._pad = 0;
        return x;
        }
    };
} // namespace azp

extern "C" int azp_dpd_forces_planned_general_weight(azp_pair_plan* plan, const azp_dpd_args* args, const azp_dpd_params* d_params,
                                                     void* stream)
    {
    return azp::launch_policy_planned<azp::XDPD>(plan, args, d_params, stream);
    }

// what gpu_compute_dpd_forces<E> forwards to (src/PotentialPairDPDThermoGPUKernel.cu.inc:21-24)
extern "C" int azp_dpd_forces_general_weight(const azp_dpd_args* args, const azp_dpd_params* d_params, void* stream)
    {
    return azp::launch_policy_entry<azp::XDPD>(args, d_params, stream);
    }
