// fire.hip -- energy minimization (azplugins_amd.minimize.FIRE; name and parameter keys of hoomd.md.minimize.FIRE).
// HOOMD-blue's source is not available here: the scheme is DEFINED in include/azp.h and DESIGN 4.19, and
// tests/fire_ref.py restates it in numpy.
//
// FIRE is velocity Verlet whose velocities are mixed with the force direction ahead of step one and whose time step
// adapts to the sign of the power P = f . v. The kernels, their bytes and why the advance is a kernel of its own:
// controlled_verlet.hpp. This file is the policy: four sums (P, |v|^2, |f|^2, U), which read the force (the measure
// pass moves 64 B per particle); a control state that holds the time step itself, so dt does not travel by value in the
// argument struct as it does in every other integrator here; the steer v = KEEP v + MIX f; the advance that tests for
// convergence and computes the two coefficients and the next DT and ALPHA.
//
// Once the state says converged (or that a sum was not finite) step two, the advance and step one return after reading
// the flags: positions stop moving, and a run that goes on costs launches alone. The advance uses + * / sqrt min
// alone, all correctly rounded: a host restatement reproduces every bit of it too.
#include <cmath>

#include "controlled_verlet.hpp"

namespace azp
{
struct FireConsts
    {
    double dt_max;
    double force_tol;
    double energy_tol;
    double finc_dt;
    double fdec_dt;
    double alpha_start;
    double fdec_alpha;
    double min_steps_adapt;
    double min_steps_conv;
    };

static bool fire_in_unit_interval(double x) { return x > 0.0 && x < 1.0; }

#pragma clang fp contract(off)
struct Fire
    {
    typedef azp_fire_args Args;
    typedef FireConsts Consts;
    static constexpr uint32_t NS = AZP_FIRE_NSLOTS;
    static constexpr bool SUMS_READ_FORCE = true, STATE_HOLDS_DT = true;
    struct Control
        {
        double dt, keep, mix;
        };

    // (the flags are the same for every thread of the grid: all leave together)
    template<bool STEER> static __device__ __forceinline__ bool control(const double* state, const Consts&, Control& c)
        {
        if (state[AZP_FIRE_CONVERGED] != 0.0 || state[AZP_FIRE_NONFINITE] != 0.0)
            return false;
        c.dt = state[AZP_FIRE_DT];
        if (STEER)
            {
            c.keep = state[AZP_FIRE_KEEP];
            c.mix = state[AZP_FIRE_MIX];
            }
        return true;
        }

    static __device__ __forceinline__ void add_terms(double (&acc)[NS], const double4& v, const double4& f)
        {
        acc[0] += ((f.x * v.x) + (f.y * v.y)) + (f.z * v.z);
        acc[1] += ((v.x * v.x) + (v.y * v.y)) + (v.z * v.z);
        acc[2] += ((f.x * f.x) + (f.y * f.y)) + (f.z * f.z);
        acc[3] += f.w;
        }

    static __device__ __forceinline__ void steer(const Control& c, double4& v, const double4& f)
        {
        v.x = (c.keep * v.x) + (c.mix * f.x);
        v.y = (c.keep * v.y) + (c.mix * f.y);
        v.z = (c.keep * v.z) + (c.mix * f.z);
        }

    static __device__ __forceinline__ void advance(double* s, const Consts& a, uint32_t N, const double (&sum)[NS])
        {
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
        const double n = (double)N;
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

    static bool valid(int which, const Args& a)
        {
        if (which != CV_ADVANCE)
            return true;
        // (a comparison with a NaN is false, and an infinite value is refused by name)
        if (!(a.dt_max > 0.0) || !(a.force_tol > 0.0) || !(a.energy_tol > 0.0) || !(a.finc_dt > 1.0))
            return false;
        if (std::isinf(a.dt_max) || std::isinf(a.force_tol) || std::isinf(a.energy_tol) || std::isinf(a.finc_dt))
            return false;
        return fire_in_unit_interval(a.fdec_dt) && fire_in_unit_interval(a.alpha_start) && fire_in_unit_interval(a.fdec_alpha);
        }

    static void constants(const Args& a, Consts& k)
        {
        k.dt_max = a.dt_max;
        k.force_tol = a.force_tol;
        k.energy_tol = a.energy_tol;
        k.finc_dt = a.finc_dt;
        k.fdec_dt = a.fdec_dt;
        k.alpha_start = a.alpha_start;
        k.fdec_alpha = a.fdec_alpha;
        k.min_steps_adapt = (double)a.min_steps_adapt;
        k.min_steps_conv = (double)a.min_steps_conv;
        }
    };
#pragma clang fp contract(on)
} // namespace azp

extern "C" int azp_fire_partials_size(uint32_t N, uint64_t* bytes) { return azp::cv_partials_size<azp::Fire>(N, bytes); }
extern "C" int azp_fire_measure(const azp_fire_args* args, void* stream)
    {
    return azp::launch_cv<azp::Fire>(azp::CV_MEASURE, args, stream);
    }
extern "C" int azp_fire_step_two(const azp_fire_args* args, void* stream)
    {
    return azp::launch_cv<azp::Fire>(azp::CV_STEP_TWO, args, stream);
    }
extern "C" int azp_fire_advance(const azp_fire_args* args, void* stream)
    {
    return azp::launch_cv<azp::Fire>(azp::CV_ADVANCE, args, stream);
    }
extern "C" int azp_fire_step_one(const azp_fire_args* args, void* stream)
    {
    return azp::launch_cv<azp::Fire>(azp::CV_STEP_ONE, args, stream);
    }
