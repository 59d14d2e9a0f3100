// pair_auto.hpp -- the tile plan behind the reference's own kernel-driver signatures.
//
// azplugins binds   hipError_t gpu_compute_pair_forces<E>(const pair_args_t&, const param_type*)
// (src/PotentialPairGPUKernel.cu.inc:25-28) and its siblings gpu_compute_dpd_forces<E>
// (src/PotentialPairDPDThermoGPUKernel.cu.inc:21-24) and gpu_compute_pair_aniso_forces<E>
// (src/AnisoPotentialPairGPUKernel.cu.inc:21-25): one call per step, borrowed device
// pointers, no notion of "the neighbor list was rebuilt". libazp's entry points
// azp_pair_forces_<evaluator>, azp_dpd_forces_general_weight and
// azp_aniso_forces_two_patch_morse take exactly that information, so the LDS-staged tile
// kernels have to find out by themselves whether the plan they compiled still describes the
// list they are handed. Per call (round 3: nothing on the caller's stream waits for the host):
//
//   1. two small kernels on the caller's stream (pair_auto.hip: auto_check_kernel leaves one
//      partial result per workgroup, auto_fold_kernel folds them) leave in device memory
//        * a 64-bit fingerprint of the list -- every n_neigh and head_list word, the cutoff
//          table, the box and N, plus every list entry for lists of up to 2^22 entries and,
//          beyond that, two entries of every 8th row, the rows rotating from call to call so
//          that eight calls cover every row -- compared there with the value learned when the
//          plan was compiled: the "stale" word;
//        * the largest displacement of any particle (and any type change) since the plan was
//          compiled, against a copy of the positions taken at that time, and the number of
//          Verlet-buffer shells that displacement makes the tile kernel walk;
//   2. the tile kernel is launched right behind it, SPECULATIVELY: it reads the shell count
//      from device memory and its workgroups leave at once when the stale word is set;
//   3. the 48-byte result travels to the host on a side stream (event-ordered after the check
//      kernel only), and the host waits for THAT -- about the duration of the check kernel,
//      while the tile kernel is already running;
//   4. stale (or no plan yet): the plan is recompiled from the list, the positions are copied,
//      the fingerprints are learned, and the tile kernel is launched again -- stream order
//      makes its results the ones the caller sees.
//
// The plans live in a small process-wide cache keyed by the list's device pointers, N, the
// number of types, the cutoff table and the kind of kernel (one lane per particle for the DPD /
// TwoPatchMorse kernels). The cache lock is held from the lookup to the last launch of a call.
// Callers that know when the list changes (the Python layer, HOOMD's
// NeighborList::getNumUpdates()) either use the explicit azp_pair_plan_* API or pass
// azp_pair_args.list_generation. With it non-zero the list words are not fingerprinted (N, the
// box and the cutoffs still are): the plan is recompiled when the number changes, so the caller
// must change it on every rewrite of the list, re-sorts of the particles included.
//
// Restrictions, stated: the call blocks the host for the duration of the check kernel (it
// cannot be captured into a HIP graph); all calls that share a list must use one stream. Residual
// risk of the sampled fingerprint (lists above 2^22 entries without list_generation): a rebuild
// that leaves every row length and every row start unchanged is noticed only when the rotating
// sample reaches a changed row (within eight calls). A million-particle rebuild changes on the
// order of a million row lengths. AZP_AUTO_PLAN=0 (environment) or AZP_PAIR_FLAG_NO_AUTO_PLAN
// (per call) selects the generic kernel instead.
#pragma once

#include <functional>

#include "pair_tiled.hpp"
#include "xtiled.hpp"

namespace azp
{
// What the kernel launcher gets from the cache: the plan, the arguments to launch with, and -- for the
// speculative launch -- the device words the kernel reads (null for the launch after a recompile).
struct AutoLaunch
    {
    const PairPlan* plan;
    const azp_pair_args* args;  // displacement fields filled in
    const TileDyn* dyn;         // speculative launch: shell count / stale word in device memory
    };
typedef std::function<int(const AutoLaunch&)> AutoLauncher;

// pair_auto.hip. lanes_one: the kernel needs a plan with one lane per particle (xtiled kernels).
// launch_tiled is called once (plan current) or twice (speculative launch found stale); launch_generic
// when the list cannot be tiled. Returns an azp status.
int auto_plan_run(const azp_pair_args& args, bool lanes_one, hipStream_t stream, const AutoLauncher& launch_tiled,
                  const std::function<int()>& launch_generic);
bool auto_plan_enabled();
void auto_plan_count_generic_fallback(); // azp_auto_plan_stats.generic_fallbacks of a planned entry

inline bool auto_plan_wanted(const azp_pair_args& a)
    {
    // an explicit launch shape (threads per particle) asks for the generic kernel
    return a.threads_per_particle == 0 && !(a.flags & AZP_PAIR_FLAG_NO_AUTO_PLAN) && auto_plan_enabled();
    }

// What the entry points need to know of a policy besides its generic kernel. XDPD / XTPM: the arguments wrap an
// azp_pair_args (args.pair); the tile kernel is xtiled_kernel, which takes plans with one lane per particle.
template<class X> struct PolicyEntry
    {
    template<class Args> static const azp_pair_args& pair(const Args& a) { return a.pair; }
    static constexpr bool kLanesOne = true;
    static bool usable(const PairPlan& plan, const azp_pair_args& a) { return xtiled_usable(plan, a); }
    static int tiled(const PairPlan& plan, const azp_pair_args& a, const typename X::KExtra& x, const typename X::Params* d_params, hipStream_t s,
                     const TileDyn* dyn)
        {
        return launch_xtiled<X>(plan, a, x, d_params, s, dyn);
        }
    static int generic(const azp_pair_args& a, const typename X::KExtra& x, const typename X::Params* d_params, hipStream_t s)
        {
        return launch_generic<X>(a, x, d_params, s);
        }
    };

// The isotropic potentials (XIso): azp_pair_args itself; pair_forces_tiled_kernel at the plan's lanes per particle, split
// launches included (pair_tiled.hpp); the xplor instance of the generic kernel picked per call
template<class E, bool XPLOR> struct PolicyEntry<XIso<E, XPLOR>>
    {
    static const azp_pair_args& pair(const azp_pair_args& a) { return a; }
    static constexpr bool kLanesOne = false;
    static bool usable(const PairPlan& plan, const azp_pair_args&) { return plan.valid; }
    static int tiled(const PairPlan& plan, const azp_pair_args& a, const typename XIso<E, XPLOR>::KExtra&, const typename E::Params* d_params, hipStream_t s,
                     const TileDyn* dyn)
        {
        return launch_tiled_tpp<E>(plan, a, d_params, s, dyn);
        }
    static int generic(const azp_pair_args& a, const typename XIso<E, XPLOR>::KExtra&, const typename E::Params* d_params, hipStream_t s)
        {
        if (a.shift_mode == AZP_SHIFT_XPLOR)
            return launch_generic<XIso<E, true>>(a, {}, d_params, s);
        return launch_generic<XIso<E, false>>(a, {}, d_params, s);
        }
    };

// Entry points of the pair potentials: azp_pair_forces_planned_<evaluator>, azp_dpd_forces_planned_general_weight,
// azp_aniso_forces_planned_two_patch_morse. X::validate returns an azp status (< 0), 1 when there is nothing to do,
// or 0; X::extra builds the kernels' KExtra from the arguments.
template<class X, class Args>
int launch_policy_planned(azp_pair_plan* plan_, const Args* args, const typename X::Params* d_params, void* stream)
    {
    typedef PolicyEntry<X> P;
    if (!plan_)
        return AZP_ERROR_INVALID_ARGUMENT;
    const int bad = X::validate(args, d_params);
    if (bad < 0) return bad;
    if (bad > 0) return AZP_SUCCESS;
    const PairPlan& plan = *reinterpret_cast<const PairPlan*>(plan_);
    const azp_pair_args& pa = P::pair(*args);
    if (plan.builds == 0 || plan.N != pa.N || plan.nlist_ptr != pa.d_nlist || plan.head_ptr != pa.d_head_list)
        return AZP_ERROR_INVALID_ARGUMENT; // a plan compiled from a different list is a caller bug
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!P::usable(plan, pa)) // (a plan compiled from the cell list has no HOOMD-format list to fall back to)
        return plan.from_cells ? AZP_ERROR_INVALID_ARGUMENT : P::generic(pa, X::extra(*args), d_params, s);
    const int rc = P::tiled(plan, pa, X::extra(*args), d_params, s, nullptr);
    // the tile instance cannot hold the per-type-pair table beside its staged slots: the generic kernel's table is
    // smaller (a plan from the cells has no list for it: the caller compiles one from the list)
    if (rc != AZP_ERROR_TOO_MANY_TYPES || plan.from_cells)
        return rc;
    auto_plan_count_generic_fallback();
    return P::generic(pa, X::extra(*args), d_params, s);
    }

// ... and azp_pair_forces_<evaluator>, azp_dpd_forces_general_weight, azp_aniso_forces_two_patch_morse: the tile-staged
// kernel from libazp's own plan cache unless the caller asks for the generic kernel. r_list_max is not part of
// pair_args_t: when the caller leaves it 0 the tile kernels decide per tile from the staged positions whether the staged
// images are minimum images.
template<class X, class Args> int launch_policy_entry(const Args* args, const typename X::Params* d_params, void* stream)
    {
    typedef PolicyEntry<X> P;
    const int bad = X::validate(args, d_params);
    if (bad < 0) return bad;
    if (bad > 0) return AZP_SUCCESS;
    const azp_pair_args& pa = P::pair(*args);
    const typename X::KExtra x = X::extra(*args);
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto generic = [&]() { return P::generic(pa, x, d_params, s); };
    if (!auto_plan_wanted(pa))
        return generic();
    return auto_plan_run(
        pa, P::kLanesOne, s,
        [&](const AutoLaunch& l) { return P::usable(*l.plan, *l.args) ? P::tiled(*l.plan, *l.args, x, d_params, s, l.dyn) : generic(); },
        generic);
    }
} // namespace azp
