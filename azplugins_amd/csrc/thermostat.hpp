// thermostat.hpp -- the thermostat policy of controlled_verlet.hpp: Berendsen, Bussi and MTTK as a scalar map
// (K, state, t) -> alpha on the device-resident state of include/azp.h (AZP_THERMOSTAT_* slots). thermostat.hip runs it
// under ConstantVolume; barostat.hip calls Thermostat::advance from the open phase of its own advance, on the
// thermostat's own state. The scheme: include/azp.h, DESIGN 4.18.
#pragma once
#include "controlled_verlet.hpp"
#include "evaluators.hpp"

namespace azp
{
constexpr uint32_t RNG_THERMOSTAT = 204;      // 201 / 202: the flow methods (flow_methods.hip)
constexpr uint32_t TS_GAMMA_MAX_ATTEMPTS = 32; // a guard, not a path: the acceptance rate exceeds 0.95 for a >= 1

struct TSConsts
    {
    double dt;
    double kT;
    double tau;
    double ndof;
    uint64_t timestep;
    uint32_t seed;
    uint32_t kind;
    };

#pragma clang fp contract(off)
// draw k of the step's stream: key (id, seed, t) as the flow methods lay it out, counter {k, 0, 0, 0}
__device__ __forceinline__ double ts_u01(uint32_t k0, uint32_t k1, uint32_t k) { return philox_u01(k0, k1, k, 0, 0, 0); }

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

__device__ __forceinline__ double mttk_g(const TSConsts& a, double K)
    {
    return ((2.0 * K) / (a.ndof * a.kT) - 1.0) / (a.tau * a.tau);
    }

struct Thermostat
    {
    typedef azp_thermostat_args Args;
    typedef TSConsts Consts;
    static constexpr uint32_t NS = 1;
    static constexpr bool SUMS_READ_FORCE = false, STATE_HOLDS_DT = false;
    struct Control
        {
        double dt, alpha;
        };

    template<bool STEER> static __device__ __forceinline__ bool control(const double* state, const Consts& k, Control& c)
        {
        c.dt = k.dt;
        if (STEER)
            c.alpha = state[AZP_THERMOSTAT_ALPHA];
        return true;
        }

    // 1/2 m |v|^2 in the order DESIGN 4.18 states
    static __device__ __forceinline__ void add_terms(double (&acc)[NS], const double4& v, const double4&)
        {
        acc[0] += 0.5 * ((((v.w * v.x) * v.x) + ((v.w * v.y) * v.y)) + ((v.w * v.z) * v.z));
        }

    // (not FIRE's steer with mix = 0: 0 * inf is NaN, and -0.0 + 0.0 is +0.0)
    static __device__ __forceinline__ void steer(const Control& c, double4& v, const double4&)
        {
        v.x = c.alpha * v.x; v.y = c.alpha * v.y; v.z = c.alpha * v.z;
        }

    static __device__ __forceinline__ void advance(double* s, const Consts& a, uint32_t, const double (&sum)[NS])
        {
        const double K = sum[0];
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
                const uint32_t k0 = philox_key0(RNG_THERMOSTAT, a.timestep, a.seed), k1 = (uint32_t)a.timestep;
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

    static bool valid(int which, const Args& a)
        {
        if (which == CV_MEASURE)
            return true;
        if (!(a.dt > 0.0))
            return false;
        if (which != CV_ADVANCE)
            return true;
        if (a.kind > AZP_THERMOSTAT_MTTK || !(a.kT > 0.0) || !(a.ndof >= 3.0))
            return false;
        // (Bussi: tau = 0 is the instantaneous canonical resampling; Berendsen below dt gives a negative radicand)
        if (a.kind == AZP_THERMOSTAT_BUSSI ? !(a.tau >= 0.0) : !(a.tau > 0.0))
            return false;
        return !(a.kind == AZP_THERMOSTAT_BERENDSEN && a.tau < a.dt);
        }

    static void constants(const Args& a, Consts& k)
        {
        k.dt = a.dt;
        k.kT = a.kT;
        k.tau = a.tau;
        k.ndof = a.ndof;
        k.timestep = a.timestep;
        k.seed = a.seed & 0xffffu;
        k.kind = a.kind;
        }
    };
#pragma clang fp contract(on)
} // namespace azp
