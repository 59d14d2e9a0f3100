// angle_forces.hip -- three-body bending forces over a per-particle angle table. The reference holds no angle code:
// the semantics are HOOMD's documented md.angle.Harmonic and md.angle.CosineSquared conventions, defined in
// include/azp.h ("angle forces") and DESIGN 4.16.
//
// The outer kernel is bonded_forces_kernel (bonded_kernel.hpp); this file holds the evaluators and the angle geometry.
// The lane keeps, of each angle, the force on its own position, a third of the energy and a third of the virial. The
// three lanes of one angle evaluate the same expression on the same operands, so their forces add to zero to rounding.
// Every table read is one 16-byte load.
//
// EvalAngleTable is the tabulated form (angle.Table; include/azp.h "tabulated angle and dihedral potentials", DESIGN
// 4.26): the rows of EvalTable (evaluators.hpp) over theta in [0, pi], read with its interpolate().
#include "evaluators.hpp"
#include "bonded_kernel.hpp"

namespace azp
{
// U and g = dU/d(cos theta) from c = cos theta (clamped) and s = max(sin theta, 1e-3)
struct EvalAngleHarmonic
    {
    typedef azp_angle_harmonic_params Params;
    static __device__ __forceinline__ void eval(const Params& p, double c, double s, double& U, double& g)
        {
        const double dth = acos(c) - p.t0;
        const double kd = p.k * dth;
        U = 0.5 * kd * dth;
        g = -kd * fast_rcp(s);
        }
    };

struct EvalAngleCosineSquared
    {
    typedef azp_angle_cossq_params Params;
    static __device__ __forceinline__ void eval(const Params& p, double c, double s, double& U, double& g)
        {
        const double dc = c - p.cos_t0;
        g = p.k * dc;
        U = 0.5 * g * dc;
        }
    };

// Tabulated U and torque tau = -dU/dtheta on n intervals of [0, pi]: g = dU/dc = tau / s, because dtheta/dc = -1 / s.
// theta == pi gives an index of n (or just below): interpolate() clamps it to row n - 1 with f = 1, the last knot.
struct EvalAngleTable
    {
    typedef azp_table_params Params;
    static __device__ __forceinline__ void eval(const Params& p, double c, double s, double& U, double& g)
        {
        U = 0.0;
        g = 0.0;
        if (p.n == 0 || p.d_rows == nullptr)
            return;
        double tau;
        EvalTable::interpolate(p.d_rows, p.n - 1, acos(c) * ((double)p.n / M_PI), U, tau);
        g = tau * fast_rcp(s);
        }
    };

struct AngleGeometry
    {
    typedef azp_angle_args Args;
    typedef double3 Own;
    typedef azp_angle_entry Entry;
    static constexpr uint32_t PARTNERS = 2;
    // An interior bead of a linear chain has 3 entries: BATCH = 3 holds it in one batch. The harmonic kernel takes 110
    // VGPRs at 2, 3 and 4 alike (acos sets its peak), the cosine-squared one 75 / 89 / 103.
    // The table instance keeps 3 as well (profiles/bonded_table.md).
    static constexpr uint32_t BATCH = 3;
    static constexpr bool FLAGS = false; // no evaluator can reject its parameters

    static bool tables(const Args& args, BondedKArgs& k)
        {
        k.table = args.d_gpu_anglelist;
        k.counts = args.d_gpu_n_angles;
        k.n_types = args.n_angle_types;
        return k.table && k.counts;
        }
    static bool block_size_ok(uint32_t bs) { return bs % 64 == 0 && bs <= 256; }

    static __device__ __forceinline__ Own own(const double* pos, uint32_t idx) { return load_scalar3_of4(pos, idx); }
    static __device__ __forceinline__ Entry unused(uint32_t idx)
        {
        Entry e;
        e.idx[0] = idx; e.idx[1] = idx; e.type = 0; e.pos = 0;
        return e;
        }
    static __device__ __forceinline__ Entry load(const BondedKArgs& a, uint64_t at)
        {
        const uint4 w = static_cast<const uint4*>(a.table)[at];
        Entry e;
        e.idx[0] = w.x; e.idx[1] = w.y; e.type = w.z; e.pos = w.w;
        return e;
        }
    static __device__ __forceinline__ uint32_t partner(const Entry& e, uint32_t k) { return e.idx[k]; }

    template<class E>
    static __device__ __forceinline__ void one(const BondedKArgs& a, const typename E::Params* s_params, const Own& p,
                                               const Entry& ent, const double3 (&partners)[PARTNERS], BondedSums& sums, unsigned int*)
        {
        const double3 &q0 = partners[0], &q1 = partners[1];
        double &fx = sums.fx, &fy = sums.fy, &fz = sums.fz, &pe = sums.pe;
        double* v = sums.v;
        // members in angle order: this lane's own position goes into slot ent.pos, the partners fill the rest
        const bool is_a = ent.pos == 0, is_c = ent.pos == 2;
        const double3 ra = select3(is_a, p, q0);
        const double3 rb = select3(is_a, q0, select3(is_c, q1, p));
        const double3 rc = select3(is_c, p, q1);
        double abx = ra.x - rb.x, aby = ra.y - rb.y, abz = ra.z - rb.z;
        double cbx = rc.x - rb.x, cby = rc.y - rb.y, cbz = rc.z - rb.z;
        min_image(a.box, abx, aby, abz);
        min_image(a.box, cbx, cby, cbz);
        const double rsqab = abx * abx + aby * aby + abz * abz;
        const double rsqcb = cbx * cbx + cby * cby + cbz * cbz;
        const double inv = fast_rsqrt(rsqab * rsqcb); // 1 / (|dab| |dcb|)
        double c = (abx * cbx + aby * cby + abz * cbz) * inv;
        c = fmin(fmax(c, -1.0), 1.0);
        // (1 - c)(1 + c): one of the factors is exact wherever 1 - c * c would cancel
        const double s = fmax(fast_sqrt((1.0 - c) * (1.0 + c)), 1e-3);
        double U, g;
        E::eval(s_params[ent.type], c, s, U, g);
        const double ca = c * fast_rcp(rsqab), cc = c * fast_rcp(rsqcb);
        const double fax = -g * (cbx * inv - ca * abx), fay = -g * (cby * inv - ca * aby), faz = -g * (cbz * inv - ca * abz);
        const double fcx = -g * (abx * inv - cc * cbx), fcy = -g * (aby * inv - cc * cby), fcz = -g * (abz * inv - cc * cbz);
        // F_b = -F_a - F_c
        fx += is_a ? fax : (is_c ? fcx : -(fax + fcx));
        fy += is_a ? fay : (is_c ? fcy : -(fay + fcy));
        fz += is_a ? faz : (is_c ? fcz : -(faz + fcz));
        const double third = 1.0 / 3.0;
        pe += third * U;
        if (a.compute_virial)
            {
            v[0] += third * (abx * fax + cbx * fcx); v[1] += third * (abx * fay + cbx * fcy);
            v[2] += third * (abx * faz + cbx * fcz); v[3] += third * (aby * fay + cby * fcy);
            v[4] += third * (aby * faz + cby * fcz); v[5] += third * (abz * faz + cbz * fcz);
            }
        }
    };
} // namespace azp

extern "C" int azp_angle_forces_harmonic(const azp_angle_args* args, const azp_angle_harmonic_params* d_params, void* stream)
    {
    return azp::launch_bonded<azp::AngleGeometry, azp::EvalAngleHarmonic>(args, d_params, nullptr, stream);
    }

extern "C" int azp_angle_forces_cosine_squared(const azp_angle_args* args, const azp_angle_cossq_params* d_params,
                                               void* stream)
    {
    return azp::launch_bonded<azp::AngleGeometry, azp::EvalAngleCosineSquared>(args, d_params, nullptr, stream);
    }

// Tabulated angle potential (include/azp.h): no flag word, [0, pi] is the whole domain.
extern "C" int azp_angle_forces_table(const azp_angle_args* args, const azp_table_params* d_params, void* stream)
    {
    return azp::launch_bonded<azp::AngleGeometry, azp::EvalAngleTable>(args, d_params, nullptr, stream);
    }
