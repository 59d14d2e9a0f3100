// bond_forces.hip -- two-body bonded forces over HOOMD's per-particle GPU bond
// table. Replaces gpu_compute_bond_forces<E, 2>, requested by the reference at
// src/PotentialBondGPUKernel.cu.inc:25-29 for E = BondEvaluatorDoubleWell and
// BondEvaluatorQuartic.
//
// The outer kernel is bonded_forces_kernel (bonded_kernel.hpp), the bond geometry is BondGeometry (bond_geometry.hpp,
// shared with the special pairs); this file holds the entry points. A handful of
// bonds per particle, ~84 B/particle of traffic: a pure streaming kernel. An evaluator that returns false (invalid
// parameters) raises the device flag word, as HOOMD's kernel does. The evaluators are in evaluators.hpp.
#include "evaluators.hpp"
#include "bond_geometry.hpp"

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
