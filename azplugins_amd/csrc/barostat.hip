// barostat.hip -- ConstantPressure (azplugins_amd.ConstantPressure; name and parameter keys of
// hoomd.md.methods.ConstantPressure). HOOMD-blue's source is not available here: the scheme, a Martyna-Tobias-Klein
// barostat on the three lengths of an orthorhombic box, is DEFINED in include/azp.h and DESIGN 4.23, and
// tests/barostat_ref.py restates it in numpy.
//
//   barostat_advance_kernel   one wave, lane 0 working: the 20 sums of azp_thermo_sums (thermo.hip), the box lengths and
//                             S to nu, alpha, lambda, b and alpha_T in the device-resident state; close and / or open by
//                             a phase mask. With a thermostat the open phase runs Thermostat::advance (thermostat.hpp) on
//                             the thermostat's own state.
//   barostat_step_one_kernel  v_a = (alpha_T alpha_a) v_a, half kick, r_a = lambda_a r_a + b_a v_a, wrap with images
//                             into the new box (vel 64 B, force 32 B, pos 64 B, image 24 B: 184 B per particle, the
//                             bytes of cv_step_one_kernel)
//   barostat_step_two_kernel  half kick, v_a = alpha_a v_a (vel 64 B, force 32 B: 96 B per particle)
//
// The kernels are this file's own and not a policy of controlled_verlet.hpp: the sums come from thermo.hip and not from
// cv_partial_kernel, the drift is not x += dt v, and step two scales after its kick. kick(), the 16-byte row loads and
// wrap_with_image are shared. One row per lane, 256 threads, no LDS, no atomics; the ten coefficients are the same for
// every lane and are loaded from the state ahead of any store. All arithmetic is plain IEEE in the order written (no
// contraction), so the per-particle kernels can be restated bit for bit; the advance goes through the device library's
// exp, which may differ from a host's by an ulp (tests/barostat_ref.BARO_REL).
#include "thermostat.hpp"

namespace azp
{
struct BaroConsts
    {
    double L[3];
    double S[3];
    double dt;
    double tauS;
    double ndof;
    uint32_t couple;
    uint32_t box_dof;
    uint32_t phase;
    uint32_t has_thermostat;
    };

#pragma clang fp contract(off)
__device__ __forceinline__ double baro_sinhc(double x)
    {
    const double x2 = x * x;
    return 1.0 + x2 * (1.0 / 6.0 + x2 * (1.0 / 120.0 + x2 * (1.0 / 5040.0 + x2 * (1.0 / 362880.0))));
    }

__global__ void __launch_bounds__(WAVE) barostat_advance_kernel(double* state, const double* sums, double* ts_state,
                                                                const BaroConsts c, const TSConsts tc)
    {
    if (threadIdx.x != 0)
        return;
    const double Kaa[3] = {sums[4], sums[7], sums[9]};
    const double Waa[3] = {sums[10], sums[13], sums[15]};
    const double K = 0.5 * ((Kaa[0] + Kaa[1]) + Kaa[2]);
    const double V = (c.L[0] * c.L[1]) * c.L[2];
    double kT = tc.kT;
    if (!c.has_thermostat)
        {
        kT = state[AZP_BAROSTAT_REF_KT];
        if (!(kT > 0.0))
            {
            kT = (2.0 * K) / c.ndof;
            state[AZP_BAROSTAT_REF_KT] = kT;
            }
        }
    const double W = ((c.ndof + 3.0) * kT) * (c.tauS * c.tauS);
    const double twoK_ndof = (2.0 * K) / c.ndof;
    double G[3];
    bool is_free[3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
        {
        is_free[a] = (c.box_dof >> a) & 1u;
        G[a] = is_free[a] ? (((Kaa[a] + Waa[a]) - V * c.S[a]) + twoK_ndof) / W : 0.0;
        }
    if (c.couple != AZP_BAROSTAT_COUPLE_NONE)
        {
        const bool in[3] = {c.couple != AZP_BAROSTAT_COUPLE_YZ, c.couple != AZP_BAROSTAT_COUPLE_XZ, c.couple != AZP_BAROSTAT_COUPLE_XY};
        double sum = 0.0, n = 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a)
            if (in[a])
                {
                sum = sum + G[a];
                if (is_free[a])
                    n = n + 1.0;
                }
        const double mean = sum / n; // (n == 0: no axis takes it)
#pragma unroll
        for (int a = 0; a < 3; ++a)
            if (in[a] && is_free[a])
                G[a] = mean;
        }
    const double hdt = 0.5 * c.dt;
    double nu[3] = {state[AZP_BAROSTAT_NU], state[AZP_BAROSTAT_NU + 1], state[AZP_BAROSTAT_NU + 2]};
    const int halves = ((c.phase & AZP_BAROSTAT_CLOSE) ? 1 : 0) + ((c.phase & AZP_BAROSTAT_OPEN) ? 1 : 0);
    for (int h = 0; h < halves; ++h)
        {
#pragma unroll
        for (int a = 0; a < 3; ++a)
            nu[a] = is_free[a] ? nu[a] + hdt * G[a] : 0.0;
        }
    bool finite = isfinite(nu[0]) && isfinite(nu[1]) && isfinite(nu[2]);
    if (c.phase & AZP_BAROSTAT_OPEN)
        {
        const double trace = (nu[0] + nu[1]) + nu[2];
        const double share = trace / c.ndof;
#pragma unroll
        for (int a = 0; a < 3; ++a)
            {
            const double alpha = exp(-((nu[a] + share) * hdt));
            const double lambda = exp(nu[a] * c.dt);
            const double x = nu[a] * hdt;
            const double b = (c.dt * exp(x)) * baro_sinhc(x);
            finite = finite && isfinite(alpha) && isfinite(lambda) && isfinite(b);
            state[AZP_BAROSTAT_ALPHA + a] = alpha;
            state[AZP_BAROSTAT_LAMBDA + a] = lambda;
            state[AZP_BAROSTAT_B + a] = b;
            }
        double alpha_T = 1.0;
        if (c.has_thermostat)
            {
            const double sum[1] = {K};
            Thermostat::advance(ts_state, tc, 0u, sum);
            alpha_T = ts_state[AZP_THERMOSTAT_ALPHA];
            }
        state[AZP_BAROSTAT_ALPHA_T] = alpha_T;
        }
#pragma unroll
    for (int a = 0; a < 3; ++a)
        {
        state[AZP_BAROSTAT_NU + a] = nu[a];
        state[AZP_BAROSTAT_P + a] = (Kaa[a] + Waa[a]) / V;
        }
    state[AZP_BAROSTAT_ENERGY] = (0.5 * W) * ((nu[0] * nu[0] + nu[1] * nu[1]) + nu[2] * nu[2]);
    state[AZP_BAROSTAT_V] = V;
    state[AZP_BAROSTAT_K] = K;
    state[AZP_BAROSTAT_W] = W;
    state[AZP_BAROSTAT_NONFINITE] = finite ? 0.0 : 1.0;
    }

struct BaroKArgs
    {
    double* pos;
    double* vel;
    const double* net_force;
    int32_t* image;
    const double* state;
    BoxDev box;
    double dt;
    uint32_t N;
    };

__global__ void __launch_bounds__(256) barostat_step_one_kernel(const BaroKArgs a)
    {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.N)
        return;
    // (the same ten values in every lane, loaded ahead of any store)
    const double* s = a.state;
    const double alpha_T = s[AZP_BAROSTAT_ALPHA_T];
    const double cx = alpha_T * s[AZP_BAROSTAT_ALPHA], cy = alpha_T * s[AZP_BAROSTAT_ALPHA + 1], cz = alpha_T * s[AZP_BAROSTAT_ALPHA + 2];
    const double lx = s[AZP_BAROSTAT_LAMBDA], ly = s[AZP_BAROSTAT_LAMBDA + 1], lz = s[AZP_BAROSTAT_LAMBDA + 2];
    const double bx = s[AZP_BAROSTAT_B], by = s[AZP_BAROSTAT_B + 1], bz = s[AZP_BAROSTAT_B + 2];
    double4 v = load_scalar4(a.vel, idx);
    const double4 f = load_scalar4(a.net_force, idx);
    const double4 p = load_scalar4(a.pos, idx);
    const double minv = 1.0 / v.w;
    v.x = cx * v.x; v.y = cy * v.y; v.z = cz * v.z;
    kick(v, f, 0.5 * a.dt, minv);
    store_scalar4(a.vel, idx, v.x, v.y, v.z, v.w);
    double x = lx * p.x + bx * v.x, y = ly * p.y + by * v.y, z = lz * p.z + bz * v.z;
    wrap_with_image(a.box, x, y, z, a.image, idx);
    store_scalar4(a.pos, idx, x, y, z, p.w);
    }

__global__ void __launch_bounds__(256) barostat_step_two_kernel(const BaroKArgs a)
    {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.N)
        return;
    const double* s = a.state;
    const double ax = s[AZP_BAROSTAT_ALPHA], ay = s[AZP_BAROSTAT_ALPHA + 1], az = s[AZP_BAROSTAT_ALPHA + 2];
    double4 v = load_scalar4(a.vel, idx);
    const double4 f = load_scalar4(a.net_force, idx);
    kick(v, f, 0.5 * a.dt, 1.0 / v.w);
    store_scalar4(a.vel, idx, ax * v.x, ay * v.y, az * v.z, v.w);
    }
#pragma clang fp contract(on)

// what every entry refuses
static bool baro_valid(const azp_barostat_args* a)
    {
    if (!a || a->N == 0 || !a->d_state || !(a->dt > 0.0) || a->box_dof > 7u)
        return false;
    for (int k = 0; k < 3; ++k)
        {
        if (a->box.tilt[k] != 0.0 || !(a->box.L[k] > 0.0))
            return false;
        if (((a->box_dof >> k) & 1u) && !a->box.periodic[k])
            return false;
        }
    return true;
    }

static int baro_step(bool one, const azp_barostat_args* a, void* stream)
    {
    if (!baro_valid(a) || !a->d_vel || !a->d_net_force || (one && !a->d_pos))
        return AZP_ERROR_INVALID_ARGUMENT;
    BaroKArgs k;
    k.pos = a->d_pos;
    k.vel = a->d_vel;
    k.net_force = a->d_net_force;
    k.image = a->d_image;
    k.state = a->d_state;
    k.box = make_box_dev(a->box);
    k.dt = a->dt;
    k.N = a->N;
    const dim3 grid((a->N + 255u) / 256u), block(256);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (one)
        hipLaunchKernelGGL(barostat_step_one_kernel, grid, block, 0, s, k);
    else
        hipLaunchKernelGGL(barostat_step_two_kernel, grid, block, 0, s, k);
    return (int)hipGetLastError();
    }
} // namespace azp

extern "C" int azp_barostat_step_one(const azp_barostat_args* args, void* stream) { return azp::baro_step(true, args, stream); }
extern "C" int azp_barostat_step_two(const azp_barostat_args* args, void* stream) { return azp::baro_step(false, args, stream); }

extern "C" int azp_barostat_advance(const azp_barostat_args* args, void* stream)
    {
    using namespace azp;
    if (!baro_valid(args) || !args->d_sums || !(args->tauS > 0.0) || !(args->ndof >= 3.0) || args->couple > AZP_BAROSTAT_COUPLE_XYZ
        || args->phase == 0u || args->phase > (AZP_BAROSTAT_CLOSE | AZP_BAROSTAT_OPEN))
        return AZP_ERROR_INVALID_ARGUMENT;
    BaroConsts c;
    for (int k = 0; k < 3; ++k)
        {
        if (!std::isfinite(args->S[k]))
            return AZP_ERROR_INVALID_ARGUMENT;
        c.L[k] = args->box.L[k];
        c.S[k] = args->S[k];
        }
    c.dt = args->dt;
    c.tauS = args->tauS;
    c.ndof = args->ndof;
    c.couple = args->couple;
    c.box_dof = args->box_dof;
    c.phase = args->phase;
    c.has_thermostat = args->d_thermostat_state != nullptr;
    TSConsts tc = {};
    if (c.has_thermostat)
        {
        azp_thermostat_args t = {};
        t.dt = args->dt;
        t.kT = args->thermostat_kT;
        t.tau = args->thermostat_tau;
        t.ndof = args->ndof;
        t.timestep = args->timestep;
        t.seed = args->thermostat_seed;
        t.kind = args->thermostat_kind;
        if (!Thermostat::valid(CV_ADVANCE, t))
            return AZP_ERROR_INVALID_ARGUMENT;
        Thermostat::constants(t, tc);
        }
    hipLaunchKernelGGL(barostat_advance_kernel, dim3(1), dim3(WAVE), 0, static_cast<hipStream_t>(stream), args->d_state,
                       args->d_sums, args->d_thermostat_state, c, tc);
    return (int)hipGetLastError();
    }
