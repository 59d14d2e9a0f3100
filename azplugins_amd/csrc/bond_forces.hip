// bond_forces.hip -- two-body bonded forces over HOOMD's per-particle GPU bond
// table. Replaces gpu_compute_bond_forces<E, 2>, requested by the reference at
// src/PotentialBondGPUKernel.cu.inc:25-29 for E = BondEvaluatorDoubleWell and
// BondEvaluatorQuartic.
//
// The outer kernel is bonded_forces_kernel (bonded_kernel.hpp); this file holds the bond geometry. A handful of
// bonds per particle, ~84 B/particle of traffic: a pure streaming kernel. An evaluator that returns false (invalid
// parameters) raises the device flag word, as HOOMD's kernel does. The evaluators are in evaluators.hpp.
#include "evaluators.hpp"
#include "bonded_kernel.hpp"

namespace azp
{
struct BondGeometry
    {
    typedef azp_bond_args Args;
    typedef double4 Own;
    struct Entry
        {
        azp_bond_entry ent;
        uint32_t my_pos; // HOOMD's separate bond_pos column
        };
    static constexpr uint32_t PARTNERS = 1;
    // a linear chain has <= 2 bonds per bead
    static constexpr uint32_t BATCH = 4;
    static constexpr bool FLAGS = true;

    static bool tables(const Args& args, BondedKArgs& k)
        {
        k.table = args.d_gpu_bondlist;
        k.table2 = args.d_gpu_bond_pos;
        k.counts = args.d_gpu_n_bonds;
        k.n_types = args.n_bond_types;
        return k.table && k.table2 && k.counts;
        }
    static bool block_size_ok(uint32_t bs) { return bs % 64 == 0 && bs <= 256; }

    static __device__ __forceinline__ Own own(const double* pos, uint32_t idx) { return load_scalar4(pos, idx); }
    static __device__ __forceinline__ Entry unused(uint32_t idx)
        {
        Entry e;
        e.ent.idx = idx; e.ent.type = 0; e.my_pos = 0;
        return e;
        }
    static __device__ __forceinline__ Entry load(const BondedKArgs& a, uint64_t at)
        {
        Entry e;
        e.ent = static_cast<const azp_bond_entry*>(a.table)[at];
        e.my_pos = a.table2[at];
        return e;
        }
    static __device__ __forceinline__ uint32_t partner(const Entry& e, uint32_t) { return e.ent.idx; }

    template<class E>
    static __device__ __forceinline__ void one(const BondedKArgs& a, const typename E::Params* s_params, const Own& p,
                                               const Entry& entry, const double3 (&partners)[PARTNERS], BondedSums& sums,
                                               unsigned int* d_flags)
        {
        const azp_bond_entry& ent = entry.ent;
        const uint32_t my_pos = entry.my_pos;
        const double3& q = partners[0];
        double &fx = sums.fx, &fy = sums.fy, &fz = sums.fz, &pe = sums.pe;
        double* v = sums.v;
        // dx = x_a - x_b with a the first member of the bond
        double dx, dy, dz;
        if (my_pos == 0) { dx = p.x - q.x; dy = p.y - q.y; dz = p.z - q.z; }
        else { dx = q.x - p.x; dy = q.y - p.y; dz = q.z - p.z; }
        min_image(a.box, dx, dy, dz);
        const double rsq = dx * dx + dy * dy + dz * dz;
        double force_divr, bond_eng;
        const bool evaluated = E::eval(s_params[ent.type], rsq, force_divr, bond_eng);
        if (evaluated)
            {
            const double sgn = (my_pos == 0) ? 1.0 : -1.0;
            fx += sgn * dx * force_divr;
            fy += sgn * dy * force_divr;
            fz += sgn * dz * force_divr;
            pe += 0.5 * bond_eng;
            if (a.compute_virial)
                {
                const double fd2 = 0.5 * force_divr;
                v[0] += fd2 * dx * dx; v[1] += fd2 * dx * dy; v[2] += fd2 * dx * dz;
                v[3] += fd2 * dy * dy; v[4] += fd2 * dy * dz; v[5] += fd2 * dz * dz;
                }
            }
        else
            *d_flags = 1u;
        }
    };
} // namespace azp

extern "C" int azp_bond_forces_double_well(const azp_bond_args* args, const azp_dw_params* d_params,
                                           unsigned int* d_flags, void* stream)
    {
    return azp::launch_bonded<azp::BondGeometry, azp::EvalDoubleWell>(args, d_params, d_flags, stream);
    }

extern "C" int azp_bond_forces_quartic(const azp_bond_args* args, const azp_quartic_params* d_params,
                                       unsigned int* d_flags, void* stream)
    {
    return azp::launch_bonded<azp::BondGeometry, azp::EvalQuartic>(args, d_params, d_flags, stream);
    }

// Tabulated bond (include/azp.h, azp_table_params): no counterpart in the reference. The flag word here means a bond
// outside its table's [r_min, r_max), found before the table is read.
extern "C" int azp_bond_forces_table(const azp_bond_args* args, const azp_table_params* d_params,
                                     unsigned int* d_flags, void* stream)
    {
    return azp::launch_bonded<azp::BondGeometry, azp::EvalTable>(args, d_params, d_flags, stream);
    }
