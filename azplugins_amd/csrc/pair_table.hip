// pair_table.hip -- C-ABI entry points azp_pair_forces_table and azp_pair_forces_planned_table: the tabulated pair
// potential (see include/azp.h, azp_table_params; kernels in pair_kernel.hpp / pair_tiled.hpp, entry in pair_auto.hpp,
// arithmetic in evaluators.hpp). A table is tabulated as the user wants it: no energy shift, no xplor smoothing.
#include "pair_auto.hpp"

extern "C" int azp_pair_forces_table(const azp_pair_args* args, const azp_table_params* d_params, void* stream)
    {
    if (args && args->shift_mode != AZP_SHIFT_NONE)
        return AZP_ERROR_INVALID_ARGUMENT;
    return azp::launch_policy_entry<azp::XIso<azp::EvalTable>>(args, d_params, stream);
    }

extern "C" int azp_pair_forces_planned_table(azp_pair_plan* plan, const azp_pair_args* args,
                                             const azp_table_params* d_params, void* stream)
    {
    if (args && args->shift_mode != AZP_SHIFT_NONE)
        return AZP_ERROR_INVALID_ARGUMENT;
    return azp::launch_policy_planned<azp::XIso<azp::EvalTable>>(plan, args, d_params, stream);
    }
