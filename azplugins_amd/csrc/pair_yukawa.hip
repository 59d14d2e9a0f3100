// pair_yukawa.hip -- C-ABI entry points azp_pair_forces_expanded_yukawa and
// azp_pair_forces_planned_expanded_yukawa (see include/azp.h; kernels in
// pair_kernel.hpp / pair_tiled.hpp, entry in pair_auto.hpp, arithmetic in evaluators.hpp).
#include "pair_auto.hpp"

extern "C" int azp_pair_forces_expanded_yukawa(const azp_pair_args* args, const azp_yukawa_params* d_params, void* stream)
    {
    return azp::launch_policy_entry<azp::XIso<azp::EvalYukawa>>(args, d_params, stream);
    }

extern "C" int azp_pair_forces_planned_expanded_yukawa(azp_pair_plan* plan, const azp_pair_args* args,
                                                const azp_yukawa_params* d_params, void* stream)
    {
    return azp::launch_policy_planned<azp::XIso<azp::EvalYukawa>>(plan, args, d_params, stream);
    }
