// langevin_device.hpp -- what the Langevin and Brownian integrators share (gfx950): the per-particle random stream, the
// type selection and the translational half steps. flow_methods.hip (flow.Langevin / flow.Brownian, a flow field u(r))
// and langevin.hip (methods.Langevin / methods.Brownian, u = 0, with rotation) call these same functions, so the
// translation of a methods.* run is the flow.* run at zero flow bit for bit.
//
// Random stream: HOOMD-5's RandomGenerator(Seed(id, timestep, seed), Counter(tag)) as the DPD thermostat restates
// it (evaluators.hpp: philox_key0, philox_u01): key = {id << 24 | (t >> 32 & 0xff) << 16 | seed16, t & 0xffffffff},
// counter {k, tag, 0, 0} for draw k. HOOMD-blue's own source is not available to this project, so this bit layout is
// NOT checked against HOOMD; the Philox core is checked by the golden known answers (philox4x32_10_kat).
#pragma once

#include "azp_device.hpp"
#include "evaluators.hpp"

namespace azp
{
constexpr uint32_t RNG_BROWNIAN_FLOW = 201; // src/RNGIdentifiers.h
constexpr uint32_t RNG_LANGEVIN_FLOW = 202;

// draw k of one particle's stream, uniform(-c, c) (UniformDistribution: a + (b - a) u01)
__device__ __forceinline__ double uniform_draw(uint32_t k0, uint32_t k1, uint32_t k, uint32_t tag, double c)
    {
    return -c + 2.0 * c * philox_u01(k0, k1, k, tag, 0, 0);
    }

// the draws first, first + 1, first + 2 of one particle, uniform(-c.k, c.k)
__device__ __forceinline__ double3 uniform3(uint32_t id, uint32_t seed, uint32_t tag, uint64_t t, const double3& c,
                                            uint32_t first = 0)
    {
    const uint32_t k0 = philox_key0(id, t, seed), k1 = (uint32_t)t;
    return make_double3(uniform_draw(k0, k1, first, tag, c.x), uniform_draw(k0, k1, first + 1, tag, c.y),
                        uniform_draw(k0, k1, first + 2, tag, c.z));
    }

// the type in pos.w if a method with this mask integrates it, else -1
__device__ __forceinline__ int selected_type(double w, uint32_t ntypes, const uint8_t* type_mask)
    {
    const int type = type_from_w(w);
    if ((uint32_t)type >= ntypes)
        return -1;
    if (type_mask && !type_mask[type])
        return -1;
    return type;
    }

// what every step of the family reads by value
struct LangevinScalars
    {
    double dt;
    double kT;
    uint64_t timestep;
    uint32_t seed;
    uint32_t noiseless;
    };

// Langevin step two in the flow velocity u (src/TwoStepLangevinFlow.h:193-245): returns the new acceleration, updates v
__device__ __forceinline__ double3 langevin_step_two(const LangevinScalars& s, double gamma, const double3& u, uint32_t tag,
                                                     const double4& f, double4& v)
    {
    double coeff = sqrt(6.0 * gamma * s.kT / s.dt);                    // :213
    if (s.noiseless)                                                   // :214-215
        coeff = 0.0;
    const double3 R = uniform3(RNG_LANGEVIN_FLOW, s.seed, tag, s.timestep, make_double3(coeff, coeff, coeff)); // :216-221
    const double bx = R.x - gamma * (v.x - u.x);                       // :228
    const double by = R.y - gamma * (v.y - u.y);
    const double bz = R.z - gamma * (v.z - u.z);
    const double minv = 1.0 / v.w;                                     // :234
    const double ax = (f.x + bx) * minv, ay = (f.y + by) * minv, az = (f.z + bz) * minv; // :233-237
    const double hdt = 0.5 * s.dt;                                     // :240
    v.x += hdt * ax; v.y += hdt * ay; v.z += hdt * az;
    return make_double3(ax, ay, az);
    }

// Langevin step one (src/TwoStepLangevinFlow.h:143-150): x += (v + a dt/2) dt, wrap, v += a dt/2; stores the position
__device__ __forceinline__ void langevin_step_one(const BoxDev& box, double dt, double* pos, int32_t* image, uint32_t idx,
                                                  const double4& p, double4& v, const double3& acc)
    {
    const double hdt = 0.5 * dt;
    double x = p.x + (v.x + hdt * acc.x) * dt;                         // :145
    double y = p.y + (v.y + hdt * acc.y) * dt;
    double z = p.z + (v.z + hdt * acc.z) * dt;
    wrap_with_image(box, x, y, z, image, idx);                         // :146
    v.x += hdt * acc.x; v.y += hdt * acc.y; v.z += hdt * acc.z;        // :149
    store_scalar4(pos, idx, x, y, z, p.w);
    }

// Brownian step (src/TwoStepBrownianFlow.h:134-178): x += (u(x) + (F_net + R) / gamma) dt, wrap; stores the position
__device__ __forceinline__ void brownian_step(const LangevinScalars& s, const BoxDev& box, double gamma, const double3& u,
                                              uint32_t tag, const double4& f, double* pos, int32_t* image, uint32_t idx,
                                              const double4& p)
    {
    double coeff = sqrt(6.0 * gamma * s.kT / s.dt);                    // :156
    if (s.noiseless)                                                   // :157-158
        coeff = 0.0;
    const double3 R = uniform3(RNG_BROWNIAN_FLOW, s.seed, tag, s.timestep, make_double3(coeff, coeff, coeff)); // :161-166
    double x = p.x + (u.x + (f.x + R.x) / gamma) * s.dt;               // :173
    double y = p.y + (u.y + (f.y + R.y) / gamma) * s.dt;
    double z = p.z + (u.z + (f.z + R.z) / gamma) * s.dt;
    wrap_with_image(box, x, y, z, image, idx);                         // :174
    store_scalar4(pos, idx, x, y, z, p.w);
    }
} // namespace azp
