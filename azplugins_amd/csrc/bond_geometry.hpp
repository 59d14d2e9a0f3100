// bond_geometry.hpp -- the two-body geometry policy of bonded_forces_kernel (bonded_kernel.hpp), shared by the bonds
// (bond_forces.hip) and the special pairs (special_pair_forces.hip): both walk a per-particle table of
// (partner, type) entries with the particle's position in the group in a plane of its own (HOOMD's bond table).
// What differs is the public argument struct the table pointers come from (bond_tables, one overload per struct)
// and whether an evaluator can reject its parameters (FLAGS_: the device flag word is then required and raised).
#pragma once
#include "bonded_kernel.hpp"

namespace azp
{
static inline bool bond_tables(const azp_bond_args& args, BondedKArgs& k)
    {
    k.table = args.d_gpu_bondlist;
    k.table2 = args.d_gpu_bond_pos;
    k.counts = args.d_gpu_n_bonds;
    k.n_types = args.n_bond_types;
    return k.table && k.table2 && k.counts;
    }

static inline bool bond_tables(const azp_special_pair_args& args, BondedKArgs& k)
    {
    k.table = args.d_gpu_pairlist;
    k.table2 = args.d_gpu_pair_pos;
    k.counts = args.d_gpu_n_pairs;
    k.n_types = args.n_pair_types;
    return k.table && k.table2 && k.counts;
    }

template<class ArgsT, bool FLAGS_>
struct TwoBodyGeometry
    {
    typedef ArgsT Args;
    typedef double4 Own;
    struct Entry
        {
        azp_bond_entry ent;
        uint32_t my_pos; // HOOMD's separate bond_pos column
        };
    static constexpr uint32_t PARTNERS = 1;
    // a linear chain has <= 2 bonds per bead
    static constexpr uint32_t BATCH = 4;
    static constexpr bool FLAGS = FLAGS_;

    static bool tables(const Args& args, BondedKArgs& k) { return bond_tables(args, k); }
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
        else if (FLAGS)
            *d_flags = 1u;
        }
    };

typedef TwoBodyGeometry<azp_bond_args, true> BondGeometry;
typedef TwoBodyGeometry<azp_special_pair_args, false> SpecialPairGeometry;
} // namespace azp
