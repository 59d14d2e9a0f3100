// rotation.hpp -- the quaternion arithmetic of the rotational integrators (gfx950): the NO_SQUISH scheme of the NVE
// step (external_forces.hip: nve_rot_kernel) and of methods.Langevin (langevin.hip), and the exponential map of
// methods.Brownian. q: orientation, scalar first; p: angular-momentum quaternion; body angular momentum
// S = vec(1/2 conj(q) p). Both translation units call these same functions: the arithmetic of a half kick and of the
// free rotations is one statement sequence, so a Langevin run with gamma_r = 0 and kT = 0 is the NVE run bit for bit.
#pragma once

#include "azp_device.hpp"

namespace azp
{
struct Quat
    {
    double s, x, y, z;
    };

__device__ __forceinline__ Quat load_quat(const double* base, uint32_t i)
    {
    const double4 v = load_scalar4(base, i);
    return Quat {v.x, v.y, v.z, v.w};
    }

__device__ __forceinline__ void store_quat(double* base, uint32_t i, const Quat& q)
    {
    store_scalar4(base, i, q.s, q.x, q.y, q.z);
    }

// rotate(conj(q), t): a space-frame vector into the body frame
__device__ __forceinline__ double3 to_body(const Quat& q, double t_x, double t_y, double t_z)
    {
    const double ux = -q.x, uy = -q.y, uz = -q.z;
    const double c = q.s * q.s - (ux * ux + uy * uy + uz * uz);
    const double d = 2.0 * (ux * t_x + uy * t_y + uz * t_z);
    const double tx = c * t_x + 2.0 * q.s * (uy * t_z - uz * t_y) + d * ux;
    const double ty = c * t_y + 2.0 * q.s * (uz * t_x - ux * t_z) + d * uy;
    const double tz = c * t_z + 2.0 * q.s * (ux * t_y - uy * t_x) + d * uz;
    return make_double3(tx, ty, tz);
    }

// the components of t along axes without a moment of inertia, which are not integrated, set to zero
__device__ __forceinline__ double3 zero_free_axes(double3 t, const double3& I)
    {
    if (I.x == 0.0) t.x = 0.0;
    if (I.y == 0.0) t.y = 0.0;
    if (I.z == 0.0) t.z = 0.0;
    return t;
    }

// the half kick of this project's convention: p += dt q (0, t), t in the body frame
__device__ __forceinline__ void kick(Quat& p, const Quat& q, const double3& t, double dt)
    {
    p.s += dt * -(q.x * t.x + q.y * t.y + q.z * t.z);
    p.x += dt * (q.s * t.x + (q.y * t.z - q.z * t.y));
    p.y += dt * (q.s * t.y + (q.z * t.x - q.x * t.z));
    p.z += dt * (q.s * t.z + (q.x * t.y - q.y * t.x));
    }

// S = vec(1/2 conj(q) p): the body-frame angular momentum
__device__ __forceinline__ double3 body_angmom(const Quat& q, const Quat& p)
    {
    const double sx = 0.5 * (q.s * p.x - p.s * q.x - (q.y * p.z - q.z * p.y));
    const double sy = 0.5 * (q.s * p.y - p.s * q.y - (q.z * p.x - q.x * p.z));
    const double sz = 0.5 * (q.s * p.z - p.s * q.z - (q.x * p.y - q.y * p.x));
    return make_double3(sx, sy, sz);
    }

__device__ __forceinline__ void free_rotation(int axis, Quat& p, Quat& q, double I, double dt)
    {
    Quat pk, qk;
    if (axis == 3)
        {
        pk = Quat {-p.z, p.y, -p.x, p.s};
        qk = Quat {-q.z, q.y, -q.x, q.s};
        }
    else if (axis == 2)
        {
        pk = Quat {-p.y, -p.z, p.s, p.x};
        qk = Quat {-q.y, -q.z, q.s, q.x};
        }
    else
        {
        pk = Quat {-p.x, p.s, p.z, -p.y};
        qk = Quat {-q.x, q.s, q.z, -q.y};
        }
    const double phi = 0.25 / I * (p.s * qk.s + p.x * qk.x + p.y * qk.y + p.z * qk.z);
    const double c = cos(dt * phi), sn = sin(dt * phi);
    p = Quat {c * p.s + sn * pk.s, c * p.x + sn * pk.x, c * p.y + sn * pk.y, c * p.z + sn * pk.z};
    q = Quat {c * q.s + sn * qk.s, c * q.x + sn * qk.x, c * q.y + sn * qk.y, c * q.z + sn * qk.z};
    }

// the free rotations 3, 2, 1, 2, 3 of one time step about the axes that have a moment of inertia, then q renormalised
__device__ __forceinline__ void free_rotations(Quat& p, Quat& q, const double3& I, double dt)
    {
    if (I.z != 0.0) free_rotation(3, p, q, I.z, 0.5 * dt);
    if (I.y != 0.0) free_rotation(2, p, q, I.y, 0.5 * dt);
    if (I.x != 0.0) free_rotation(1, p, q, I.x, dt);
    if (I.y != 0.0) free_rotation(2, p, q, I.y, 0.5 * dt);
    if (I.z != 0.0) free_rotation(3, p, q, I.z, 0.5 * dt);
    const double n = 1.0 / sqrt(q.s * q.s + q.x * q.x + q.y * q.y + q.z * q.z);
    q = Quat {q.s * n, q.x * n, q.y * n, q.z * n};
    }
} // namespace azp
