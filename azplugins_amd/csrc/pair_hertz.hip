// pair_hertz.hip -- C-ABI entry points azp_pair_forces_hertz and
// azp_pair_forces_planned_hertz (see include/azp.h; kernels in
// pair_kernel.hpp / pair_tiled.hpp, entry in pair_auto.hpp, arithmetic in evaluators.hpp).
#include "pair_auto.hpp"

extern "C" int azp_pair_forces_hertz(const azp_pair_args* args, const azp_hertz_params* d_params, void* stream)
    {
    return azp::launch_policy_entry<azp::XIso<azp::EvalHertz>>(args, d_params, stream);
    }

extern "C" int azp_pair_forces_planned_hertz(azp_pair_plan* plan, const azp_pair_args* args,
                                                const azp_hertz_params* d_params, void* stream)
    {
    return azp::launch_policy_planned<azp::XIso<azp::EvalHertz>>(plan, args, d_params, stream);
    }
