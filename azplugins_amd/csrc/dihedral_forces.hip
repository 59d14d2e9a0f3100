// dihedral_forces.hip -- four-body torsion forces over a per-particle dihedral table. The reference holds no dihedral
// code: the semantics (HOOMD's md.dihedral.Periodic and md.dihedral.OPLS class names and parameter keys, the IUPAC
// angle) are defined in include/azp.h ("dihedral forces") and DESIGN 4.17.
//
// The outer kernel is bonded_forces_kernel (bonded_kernel.hpp); this file holds the evaluators and the dihedral
// geometry. The lane keeps, of each dihedral, the force on its own position, a quarter of the energy and a quarter of
// the virial. The four lanes of one dihedral evaluate the same expression on the same operands. Every table read is
// one 16-byte load.
//
// cos phi and sin phi come straight from the geometry (no atan2, no sincos): with n1 = b1 x b2, n2 = b2 x b3 and
// q = 1 / (|n1||n2|), cos phi = (n1 . n2) q and sin phi = |b2| (b1 . n2) q. The multiples of phi follow from the
// angle-addition recurrence, cos phi0 and sin phi0 are folded on the host.
//
// EvalDihedralTable is the tabulated form (dihedral.Table; include/azp.h "tabulated angle and dihedral potentials",
// DESIGN 4.26): it is the one evaluator that needs phi itself and takes it with atan2.
#include "evaluators.hpp"
#include "bonded_kernel.hpp"

#ifndef AZP_DIHEDRAL_BATCH
#define AZP_DIHEDRAL_BATCH 3
#endif

namespace azp
{
// U and dU = dU/dphi from c = cos phi and s = sin phi
struct EvalDihedralPeriodic
    {
    typedef azp_dihedral_periodic_params Params;
    static __device__ __forceinline__ void eval(const Params& p, double c, double s, double& U, double& dU)
        {
        // (cos m phi, sin m phi) for m = 1 .. n by angle addition; n is a small per-type integer
        double cm = c, sm = s;
        for (uint32_t m = 1; m < p.n; ++m)
            {
            const double cn = cm * c - sm * s;
            sm = sm * c + cm * s;
            cm = cn;
            }
        const double hkd = 0.5 * p.k * (double)p.d;
        U = hkd * (cm * p.cos_phi0 + sm * p.sin_phi0) + 0.5 * p.k;   // 1/2 k (1 + d cos(n phi - phi0))
        dU = -hkd * (double)p.n * (sm * p.cos_phi0 - cm * p.sin_phi0); // -1/2 k d n sin(n phi - phi0)
        }
    };

struct EvalDihedralOPLS
    {
    typedef azp_dihedral_opls_params Params;
    static __device__ __forceinline__ void eval(const Params& p, double c, double s, double& U, double& dU)
        {
        const double c2 = c * c - s * s, s2 = 2.0 * s * c;
        const double c3 = c2 * c - s2 * s, s3 = s2 * c + c2 * s;
        const double c4 = c2 * c2 - s2 * s2, s4 = 2.0 * s2 * c2;
        U = 0.5 * (p.k1 * (1.0 + c) + p.k2 * (1.0 - c2) + p.k3 * (1.0 + c3) + p.k4 * (1.0 - c4));
        dU = 0.5 * (-p.k1 * s + 2.0 * p.k2 * s2 - 3.0 * p.k3 * s3 + 4.0 * p.k4 * s4);
        }
    };

// Tabulated U and torque tau = -dU/dphi on n intervals of [-pi, pi], stored over x = phi + pi in [0, 2 pi].
// sin phi = +0 at planar trans gives phi = +pi, x = 2 pi and the last knot (the clamp of interpolate()); sin phi = -0
// gives phi = -pi, x = 0 and the first knot. The two may differ: periodicity is the user's to keep.
struct EvalDihedralTable
    {
    typedef azp_table_params Params;
    static __device__ __forceinline__ void eval(const Params& p, double c, double s, double& U, double& dU)
        {
        U = 0.0;
        dU = 0.0;
        if (p.n == 0 || p.d_rows == nullptr)
            return;
        double tau;
        EvalTable::interpolate(p.d_rows, p.n - 1, (atan2(s, c) + M_PI) * ((double)p.n / (2.0 * M_PI)), U, tau);
        dU = -tau;
        }
    };

struct DihedralGeometry
    {
    typedef azp_dihedral_args Args;
    typedef double3 Own;
    typedef azp_dihedral_entry Entry;
    static constexpr uint32_t PARTNERS = 3;
    // BATCH = 3 is the largest that keeps 4 waves per SIMD (124 VGPRs; 143 and 3 waves at 4). An interior bead of a
    // linear chain has 4 entries and takes one turn of the tail loop; measured on C3, that still beats BATCH = 4 with
    // its lost wave. The table instance takes 142 VGPRs and 3 waves at 2, 3 and 4 alike (atan2 sets its
    // peak) and its times at the three lie within 2 %: it keeps 3 too (profiles/bonded_table.md).
    static constexpr uint32_t BATCH = AZP_DIHEDRAL_BATCH;
    static constexpr bool FLAGS = false; // no evaluator can reject its parameters

    static bool tables(const Args& args, BondedKArgs& k)
        {
        k.table = args.d_gpu_dihedrallist;
        k.counts = args.d_gpu_n_dihedrals;
        k.n_types = args.n_dihedral_types;
        return k.table && k.counts;
        }
    static bool block_size_ok(uint32_t bs) { return bs == 64 || bs == 128 || bs == 256; }

    static __device__ __forceinline__ Own own(const double* pos, uint32_t idx) { return load_scalar3_of4(pos, idx); }
    static __device__ __forceinline__ Entry unused(uint32_t idx)
        {
        Entry e;
        e.idx[0] = idx; e.idx[1] = idx; e.idx[2] = idx; e.type_pos = 0;
        return e;
        }
    static __device__ __forceinline__ Entry load(const BondedKArgs& a, uint64_t at)
        {
        const uint4 w = static_cast<const uint4*>(a.table)[at];
        Entry e;
        e.idx[0] = w.x; e.idx[1] = w.y; e.idx[2] = w.z; e.type_pos = w.w;
        return e;
        }
    static __device__ __forceinline__ uint32_t partner(const Entry& e, uint32_t k) { return e.idx[k]; }

    template<class E>
    static __device__ __forceinline__ void one(const BondedKArgs& a, const typename E::Params* s_params, const Own& p,
                                               const Entry& ent, const double3 (&partners)[PARTNERS], BondedSums& sums, unsigned int*)
        {
        const double3 &q0 = partners[0], &q1 = partners[1], &q2 = partners[2];
        double &fx = sums.fx, &fy = sums.fy, &fz = sums.fz, &pe = sums.pe;
        double* v = sums.v;
        // members in dihedral order: this lane's own position goes into slot m, the partners fill the rest
        const uint32_t m = ent.type_pos >> 30;
        const double3 ra = select3(m == 0, p, q0);
        const double3 rb = select3(m == 0, q0, select3(m == 1, p, q1));
        const double3 rc = select3(m <= 1, q1, select3(m == 2, p, q2));
        const double3 rd = select3(m == 3, p, q2);
        double b1x = rb.x - ra.x, b1y = rb.y - ra.y, b1z = rb.z - ra.z;
        double b2x = rc.x - rb.x, b2y = rc.y - rb.y, b2z = rc.z - rb.z;
        double b3x = rd.x - rc.x, b3y = rd.y - rc.y, b3z = rd.z - rc.z;
        min_image(a.box, b1x, b1y, b1z);
        min_image(a.box, b2x, b2y, b2z);
        min_image(a.box, b3x, b3y, b3z);
        const double n1x = b1y * b2z - b1z * b2y, n1y = b1z * b2x - b1x * b2z, n1z = b1x * b2y - b1y * b2x;
        const double n2x = b2y * b3z - b2z * b3y, n2y = b2z * b3x - b2x * b3z, n2z = b2x * b3y - b2y * b3x;
        const double n1sq = n1x * n1x + n1y * n1y + n1z * n1z;
        const double n2sq = n2x * n2x + n2y * n2y + n2z * n2z;
        const double b2sq = b2x * b2x + b2y * b2y + b2z * b2z;
        const double b2len = fast_sqrt(b2sq);
        const double q = fast_rsqrt(n1sq * n2sq); // 1 / (|n1| |n2|)
        const double c = (n1x * n2x + n1y * n2y + n1z * n2z) * q;
        const double s = b2len * (b1x * n2x + b1y * n2y + b1z * n2z) * q;
        double U, dU;
        E::eval(s_params[ent.type_pos & 0x3fffffffu], c, s, U, dU);
        // F_m = -dU g_m (Blondel-Karplus): g_a = -|b2| / |n1|^2 n1, g_d = |b2| / |n2|^2 n2,
        // g_b = -(1 + s12) g_a + s32 g_d, g_c = -(1 + s32) g_d + s12 g_a
        const double wa = dU * b2len * fast_rcp(n1sq);  // F_a = wa n1
        const double wd = -dU * b2len * fast_rcp(n2sq); // F_d = wd n2
        const double ib2 = fast_rcp(b2sq);
        const double s12 = (b1x * b2x + b1y * b2y + b1z * b2z) * ib2;
        const double s32 = (b3x * b2x + b3y * b2y + b3z * b2z) * ib2;
        const double fax = wa * n1x, fay = wa * n1y, faz = wa * n1z;
        const double fdx = wd * n2x, fdy = wd * n2y, fdz = wd * n2z;
        const double fcx = s12 * fax - (1.0 + s32) * fdx, fcy = s12 * fay - (1.0 + s32) * fdy, fcz = s12 * faz - (1.0 + s32) * fdz;
        const double fbx = s32 * fdx - (1.0 + s12) * fax, fby = s32 * fdy - (1.0 + s12) * fay, fbz = s32 * fdz - (1.0 + s12) * faz;
        fx += m == 0 ? fax : (m == 1 ? fbx : (m == 2 ? fcx : fdx));
        fy += m == 0 ? fay : (m == 1 ? fby : (m == 2 ? fcy : fdy));
        fz += m == 0 ? faz : (m == 1 ? fbz : (m == 2 ? fcz : fdz));
        pe += 0.25 * U;
        if (a.compute_virial)
            {
            // separations from b: a at -b1, c at b2, d at b2 + b3 (composed, not re-imaged)
            const double dx = b2x + b3x, dy = b2y + b3y, dz = b2z + b3z;
            v[0] += 0.25 * (b2x * fcx + dx * fdx - b1x * fax); v[1] += 0.25 * (b2x * fcy + dx * fdy - b1x * fay);
            v[2] += 0.25 * (b2x * fcz + dx * fdz - b1x * faz); v[3] += 0.25 * (b2y * fcy + dy * fdy - b1y * fay);
            v[4] += 0.25 * (b2y * fcz + dy * fdz - b1y * faz); v[5] += 0.25 * (b2z * fcz + dz * fdz - b1z * faz);
            }
        }
    };
} // namespace azp

extern "C" int azp_dihedral_forces_periodic(const azp_dihedral_args* args, const azp_dihedral_periodic_params* d_params,
                                            void* stream)
    {
    return azp::launch_bonded<azp::DihedralGeometry, azp::EvalDihedralPeriodic>(args, d_params, nullptr, stream);
    }

extern "C" int azp_dihedral_forces_opls(const azp_dihedral_args* args, const azp_dihedral_opls_params* d_params, void* stream)
    {
    return azp::launch_bonded<azp::DihedralGeometry, azp::EvalDihedralOPLS>(args, d_params, nullptr, stream);
    }

// Tabulated dihedral potential (include/azp.h): no flag word, [-pi, pi] is the whole domain.
extern "C" int azp_dihedral_forces_table(const azp_dihedral_args* args, const azp_table_params* d_params, void* stream)
    {
    return azp::launch_bonded<azp::DihedralGeometry, azp::EvalDihedralTable>(args, d_params, nullptr, stream);
    }
