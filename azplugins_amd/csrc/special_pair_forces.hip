// special_pair_forces.hip -- two-body forces over the per-particle table of special pairs (State.groups["pair"]):
// the interactions that stand in for the non-bonded pairs a topology excludes, e.g. the scaled 1-4 Lennard-Jones
// pairs of an OPLS chain. No counterpart in the reference; semantics in include/azp.h ("special pair forces").
//
// The outer kernel is bonded_forces_kernel (bonded_kernel.hpp) on the two-body geometry the bonds use
// (bond_geometry.hpp): one lane per particle, no atomics, the table read coalesced and the partner positions
// gathered; energy and virial shared in halves. The evaluator cannot reject its parameters: no flag word.
#include "evaluators.hpp"
#include "bond_geometry.hpp"

extern "C" int azp_special_pair_forces_lj(const azp_special_pair_args* args, const azp_special_pair_lj_params* d_params,
                                          void* stream)
    {
    return azp::launch_bonded<azp::SpecialPairGeometry, azp::EvalSpecialPairLJ>(args, d_params, nullptr, stream);
    }
