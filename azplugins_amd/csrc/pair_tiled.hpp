// pair_tiled.hpp -- tile-staged pair-force kernel (uses a PairPlan).
//
// One workgroup (4 waves) per tile of 256/TPP consecutive particles:
//   0. loads first (steps 0, the second staging form of 1 and the phases of 2: the instances
//      with one lane per particle, one type and no xplor of a split-energy evaluator --
//      PerturbedLJ with the lanes per particle the plan compilers default to; every other
//      instance tests its arguments,
//      derives the coefficients, stages asking per axis and reads the row words behind the
//      barrier, see the kernel). The uniform words of a tile (stage range, reference
//      particle, cutoff, row head and length, the words of a speculative launch) are scalar
//      loads; the stage indices are requested as soon as their range is known, the other
//      words and the coefficient arithmetic run beside that round trip, and a stale launch
//      leaves before anything is stored: arguments -> stage range -> stage indices ->
//      positions.
//   1. stage: the tile's sorted unique neighbor set is loaded once (index list
//      coalesced, positions semi-coalesced because the list is sorted) into LDS
//      as SoA x | y | z (| type), shifted to the periodic image nearest the
//      tile's reference particle. Slot 0 is a dummy parked at 1e30 for padding.
//      Two forms, uniform over the launch: orthorhombic boxes periodic along all
//      axes with the r_list_max hint and fewer than 2^27 particles shift every axis
//      without asking and address positions with 32-bit offsets; any other launch
//      asks per axis (TiledKArgs::fast_stage).
//   2. loop: each lane reads one 16-byte chunk = 8 u16 byte offsets per
//      iteration (a wave reads 1 KiB contiguous), then for each of the 8
//      neighbors three LDS gathers and the evaluator, software-pipelined in
//      batches of 4 pairs. No global gathers, no minimum image (unless the tile
//      is wide compared with the box), no row-length test (rows are padded with
//      the dummy). Rows are ordered core | sure | near | buffer shell classes
//      (pair_plan.hpp: 16 shells, the outer ones filed together): a batch with no
//      pair in range is skipped after the separations, and a batch with no pair in
//      the evaluator's core uses the cheaper tail form (PerturbedLJ); both are
//      tested on the actual separations. Under a displacement bound small enough
//      that no entry outside row class core can have entered the evaluator's core
//      (plan_core_reach_sq), the iterations behind the plan's core-class count run
//      the tail form without the core test (tiled_loop_phases).
//      Rows end at a batch, not at a chunk: a slice whose walked
//      entries end in the first half of a chunk gets one final half iteration
//      after the loop. The row ends after the buffer shells that the displacement
//      since the plan was built can have brought into range (n_shells): from
//      the caller's bound, from the words of the list's distance check, or per
//      tile from per-particle displacements.
//   3. DPP butterfly over the TPP lanes, lane 0 stores force (and virial).
// Same evaluators, same outputs as pair_kernel.hpp; results agree with it to
// rounding (the periodic shift is applied to r_j instead of to r_i - r_j).
// Counts and measurements of this form: profiles/tile_setup.md; of the phased loop's bookkeeping: profiles/pair_loop.md.
#pragma once

#include <type_traits>

#include "pair_kernel.hpp"
#include "pair_plan.hpp"

#ifndef AZP_TILED_WAVES_PER_SIMD
#define AZP_TILED_WAVES_PER_SIMD 4 // register budget: <= 128 VGPRs => 4 workgroups (of 4 waves) per CU
#endif

namespace azp
{
#ifdef AZP_TIMELINE
// debug build only (tools/timeline.py): per (tile, wave) realtime stamps (100 MHz):
// kernel entry, tile staged, loop done, and the hardware id of the wave
extern __device__ unsigned long long g_timeline[8 * 4 * 16384];
#endif

// Words a speculatively launched tile kernel reads from device memory (pair_auto.hpp): written by the
// list-check kernel that runs right before it on the same stream.
struct TileDyn
    {
    uint32_t n_shells;   // buffer shells to walk for the displacement measured by the check
    uint32_t stale;      // != 0: the plan does not describe the list any more -- leave at once (the call is repeated)
    };

struct TiledKArgs
    {
    PairKArgs p;
    const uint32_t* tile_nstage;
    const uint64_t* tile_head;
    const uint32_t* stage_idx;
    const uint32_t* slice_Kend;  // PLAN_SHELLS + 1 per slice: batches of 4 entries per lane (half chunks, plan_row_batches)
                                 // covering the in-range entries [0] / the entries up to the end of buffer shell s [1 + s];
                                 // [PLAN_SHELLS]: whole rows
    uint32_t n_shells;           // buffer shells this launch has to walk: 0 = none (positions as at plan build) ...
                                 // PLAN_SHELLS = whole rows
    const uint64_t* slice_head;
    const uint4* cnl;
    const uint8_t* perm;         // balanced plans (one lane per particle): lane -> member of the tile; NULL = identity
    const TileDyn* dyn;           // NULL: n_shells above is final
    // the same idea with the raw words of the neighbor list's distance check (azp_pair_args.d_stale_flag,
    // d_displacement_sq_bits): leave when *dflag != 0, displacement = sqrt(double(*dbits)) + bound_extra
    const uint32_t* dflag;
    const unsigned long long* dbits;
    // Local displacement bound (azp_pair_args.d_displacement): per-particle upper bounds on the distance moved since the
    // plan was built. A tile then walks the shells ITS members and staged neighbors can have crossed -- an entry of shell s
    // was at least r_cut + s w away, and the two particles of a pair have closed in by at most the sum of their own
    // displacements <= 2 x the largest one in the tile -- instead of the shells the fastest particle of the whole system
    // dictates. bound_extra is added to every entry (a plan compiled later than the positions the displacements refer to).
    const float* disp;            // n_max entries; NULL: n_shells above
    double shell_w;               // shell width of the plan
    double shell_winv;            // 1 / shell_w (0: no shells)
    double bound_extra;
    // Core phase / tail phase of a row (split-energy instances, tiled_loop_phases): chunks per lane that cover every entry of
    // row class core, per slice, and the square of the distance below which an entry OUTSIDE that class cannot have
    // come under the caller's displacement bound (plan_core_reach_sq; 0: no statement, one loop as before)
    const uint32_t* slice_Kphase;
    double core_reach_sq;
    // != 0: orthorhombic box periodic along all three axes, r_list_max given, fewer than 2^27 particles: the staging
    // shifts every axis without asking, and addresses positions with a scalar base and a 32-bit byte offset
    uint32_t fast_stage;
    };

// wave-wide maximum of a non-negative float (all lanes get it)
__device__ __forceinline__ float wave_max_nonneg(float v)
    {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
    }

// Shells a tile has to walk for the displacement bound b of its own particles (device form of plan_shells_for)
__device__ __forceinline__ uint32_t tile_shells_for(double b, double shell_winv)
    {
    if (!(b >= 0.0))
        return PLAN_SHELLS; // NaN
    if (b == 0.0)
        return 0u;
    if (!(shell_winv > 0.0))
        return PLAN_SHELLS;
    const double n = ceil(2.0 * b * (1.0 + 1e-9) * shell_winv); // (1e-9 covers the rounded reciprocal)
    return n >= (double)PLAN_SHELLS ? PLAN_SHELLS : (uint32_t)n;
    }

// A wave-uniform word that no kernel of this launch writes (plan tables, the words of an earlier kernel, positions),
// read through the constant address space: a scalar load, so neither a VGPR is held while it is in flight nor a
// v_readfirstlane needed afterwards
template<class T> __device__ __forceinline__ T load_uniform(const T* p)
    {
    return *(const __attribute__((address_space(4))) T*)p;
    }

// Scalar4 row idx of a position array with fewer than 2^27 rows: scalar base + 32-bit byte offset (one VGPR, no 64-bit
// address arithmetic per load)
__device__ __forceinline__ double4 load_scalar4_o32(const double* base, uint32_t idx)
    {
    const char* p = reinterpret_cast<const char*>(base) + (idx << 5);
    const double2 a = *reinterpret_cast<const double2*>(p);
    const double2 b = *reinterpret_cast<const double2*>(p + 16);
    return make_double4(a.x, a.y, b.x, b.y);
    }
__device__ __forceinline__ double3 load_scalar3_of4_o32(const double* base, uint32_t idx)
    {
    const char* p = reinterpret_cast<const char*>(base) + (idx << 5);
    const double2 a = *reinterpret_cast<const double2*>(p);
    const double z = *reinterpret_cast<const double*>(p + 16);
    return make_double3(a.x, a.y, z);
    }

// Stride (in slots) between the x, y and z arrays in LDS. With a stride of CAP the compiler
// fuses the x and y gathers of a pair into one ds_read2st64_b64, which runs at half the LDS
// rate of ds_read_b64 (MI355X_MICROARCH.md, LDS table); an odd stride (CAP + 1) keeps them two
// ds_read_b64: whole rows 0.143 -> 0.135 ms, MD cycle mean 0.127 -> 0.124 ms (the kernel is
// as much LDS- as VALU-bound).
#define AZP_TILE_STRIDE(CAP) ((CAP) + 1)

constexpr int TILE_BATCH = 4; // pairs per register batch: half a chunk (a whole chunk spills: 1,099 VGPRs)

// A batch of gathered neighbor data (half a chunk).
struct TileBatch
    {
    double x[TILE_BATCH], y[TILE_BATCH], z[TILE_BATCH];
    uint32_t off[TILE_BATCH];
    };

// the local-displacement fields of the kernel arguments (pair_tiled.hpp and xtiled.hpp launchers)
inline void fill_local_bound(TiledKArgs& k, const PairPlan& plan, const azp_pair_args& args)
    {
    // per-particle displacements count only together with a (global) bound: has_displacement_bound says the caller
    // tracks displacements since the plan build at all; displacement_bound_extra covers a plan built later than the
    // reference positions of d_displacement
    const bool local = args.d_displacement && args.has_displacement_bound && args.displacement_bound >= 0.0;
    k.disp = local ? args.d_displacement : nullptr;
    k.dflag = (args.d_stale_flag && args.d_displacement_sq_bits) ? args.d_stale_flag : nullptr;
    k.dbits = k.dflag ? args.d_displacement_sq_bits : nullptr;
    if (k.dflag)
        k.disp = nullptr; // (the per-particle displacements of a check whose result is not known yet are not either)
    k.shell_w = plan.shell_width;
    k.shell_winv = plan.shell_width > 0.0 ? 1.0 / plan.shell_width : 0.0;
    k.bound_extra = args.displacement_bound_extra > 0.0 ? args.displacement_bound_extra : 0.0;
    }

// phase 1: issue the LDS gathers of a batch (half H of the chunk)
template<int CAP, int H> __device__ __forceinline__ void tile_gather(TileBatch& b, const uint4& u, const char* bx)
    {
    constexpr int NB = TILE_BATCH;
    const uint32_t w0 = H ? u.z : u.x, w1 = H ? u.w : u.y;
    b.off[0] = w0 & 0xffffu;
    b.off[1] = w0 >> 16;
    b.off[2] = w1 & 0xffffu;
    b.off[3] = w1 >> 16;
#pragma unroll
    for (int e = 0; e < NB; ++e)
        {
        b.x[e] = *reinterpret_cast<const double*>(bx + b.off[e]);
        b.y[e] = *reinterpret_cast<const double*>(bx + b.off[e] + AZP_TILE_STRIDE(CAP) * 8);
        b.z[e] = *reinterpret_cast<const double*>(bx + b.off[e] + AZP_TILE_STRIDE(CAP) * 16);
        }
    }

// phase 2: arithmetic on a gathered half chunk. The separations of the 4 pairs
// are formed first; if no lane of the wave has any of them inside the (largest)
// cutoff, the evaluator work is skipped -- exact, and the common case at the far
// end of the near-first ordered rows. TAIL (split-energy instances only): the batch
// lies in the tail phase of its row, where no pair can be inside the evaluator's core
// (tiled_loop_phases): the tail form without the core test.
template<class E, int CAP, bool VIRIAL, bool SINGLE, bool XPLOR, bool WRAP, bool TAIL = false>
__device__ __forceinline__ void tile_compute(const TileBatch& b, const TiledKArgs& a, const char* bt,
                                             const typename E::Coeff* __restrict__ s_coeff,
                                             const double* __restrict__ s_ronsq, const typename E::Coeff& c0, double ronsq0,
                                             double rcutsq_max, const double3& pi, int typei, double& fx, double& fy,
                                             double& fz, double& pe, double (&v)[6], uint32_t& n_core, uint32_t& n_in, double (&es)[2])
    {
    typedef typename E::Coeff Coeff;
    constexpr int NB = TILE_BATCH;
    constexpr bool SPLIT = SINGLE && !XPLOR && E::kSplitEnergy; // energy offsets counted, see EvalPLJ::eval_split
    double dx[NB], dy[NB], dz[NB], rsq[NB];
    bool any_in = false;
#pragma unroll
    for (int e = 0; e < NB; ++e)
        {
        dx[e] = pi.x - b.x[e]; dy[e] = pi.y - b.y[e]; dz[e] = pi.z - b.z[e];
        if (WRAP)
            min_image(a.p.box, dx[e], dy[e], dz[e]);
        rsq[e] = __builtin_fma(dz[e], dz[e], __builtin_fma(dy[e], dy[e], dx[e] * dx[e]));
        if (WRAP)
            rsq[e] = (b.off[e] == 0) ? 1.0e60 : rsq[e]; // the minimum image would fold the padding slot back into the box
                                                        // (1e60: out of range, and a product of four stays finite for rcp4)
        any_in = any_in || (rsq[e] < rcutsq_max);
        }
    // (SPLIT: the hint lays the code out for the walked part of a row, where some lane nearly always has a pair in range --
    // rows end at the shell the displacement bound allows. Without it the register allocator parks the core path's energy
    // accumulator in scratch inside the hot loop: +2 % on the north star, profiles/tile_kernel_options_removed.md)
    const bool none_in = !__any(any_in);
    if (SPLIT ? __builtin_expect(none_in, 0) : none_in)
        return;
    double fd[NB]; // force / r of the batch (SPLIT: filled by one of two forms of the evaluator)
    if constexpr (SPLIT)
        {
        // one v_rcp_f64 for the four pairs of the batch (EvalPLJ::rcp4)
        double x[NB];
        E::rcp4(rsq, x);
        // rows list the pairs inside the evaluator's core first (plan hint), so beyond
        // the first chunks no lane of the wave has one and the cheaper tail-only form
        // applies to the whole batch (exact: tested on the actual separations). Both
        // branches only produce fd[]; the accumulation below is shared, so the force
        // accumulators are not live-out of either branch (no register copies at the join).
        bool any_core = false;
        if constexpr (!TAIL)
            {
#pragma unroll
            for (int e = 0; e < NB; ++e)
                any_core = any_core || E::in_core(c0, rsq[e]);
            }
        if (TAIL || !__any(any_core))
            {
            // (TAIL: the count stays a branch around four adds. As a plain condition the compiler folds it into selects
            // that every batch pays, the launches without an energy shift included)
            const bool count_in = c0.tail_add != 0.0;
#pragma unroll
            for (int e = 0; e < NB; ++e)
                E::eval_split_tail(c0, rsq[e], x[e], fd[e], es[0], es[1], n_in, TAIL ? false : count_in);
            if (TAIL && __builtin_expect(count_in, 0))
                {
#pragma unroll
                for (int e = 0; e < NB; ++e)
                    n_in += (rsq[e] < c0.rcutsq) ? 1u : 0u;
                }
            }
        else
            {
#pragma unroll
            for (int e = 0; e < NB; ++e)
                E::eval_split(c0, rsq[e], x[e], fd[e], pe, n_core, n_in);
            }
        }
#pragma unroll
    for (int e = 0; e < NB; ++e)
        {
        double force_divr, pair_eng = 0.0;
        if constexpr (SPLIT)
            force_divr = fd[e];
        else if (SINGLE)
            {
            const bool evaluated = E::eval(c0, rsq[e], force_divr, pair_eng);
            if (XPLOR && evaluated)
                apply_xplor(rsq[e], ronsq0, c0.rcutsq, force_divr, pair_eng);
            }
        else
            {
            const int typej = *reinterpret_cast<const int*>(bt + (b.off[e] >> 1));
            const uint32_t tp = (uint32_t)typei * a.p.ntypes + (uint32_t)typej;
            const Coeff cc = s_coeff[tp];
            const bool evaluated = E::eval(cc, rsq[e], force_divr, pair_eng);
            if (XPLOR && evaluated)
                apply_xplor(rsq[e], s_ronsq[tp], cc.rcutsq, force_divr, pair_eng);
            }
        fx = __builtin_fma(dx[e], force_divr, fx);
        fy = __builtin_fma(dy[e], force_divr, fy);
        fz = __builtin_fma(dz[e], force_divr, fz);
        if constexpr (!SPLIT)
            pe += pair_eng;
        if (VIRIAL)
            {
            const double fxx = force_divr * dx[e], fyy = force_divr * dy[e];
            v[0] = __builtin_fma(fxx, dx[e], v[0]);
            v[1] = __builtin_fma(fxx, dy[e], v[1]);
            v[2] = __builtin_fma(fxx, dz[e], v[2]);
            v[3] = __builtin_fma(fyy, dy[e], v[3]);
            v[4] = __builtin_fma(fyy, dz[e], v[4]);
            v[5] = __builtin_fma(force_divr * dz[e], dz[e], v[5]);
            }
        }
    }

// Inner loop over this lane's chunks, software-pipelined at half-chunk
// granularity: while the arithmetic of one half (4 pairs) runs, the 12 LDS gathers
// of the next half and the index load of the next chunk are in flight. The row is
// Kb batches (half chunks) long: Kb / 2 whole iterations, and for an odd Kb the first
// half of one more chunk, peeled off behind the loop (its gathers are the ones the
// last iteration -- or the prologue -- issued anyway; nothing is loaded for it). WRAP = true
// re-applies the minimum image to every pair (tiles that are wide compared with the
// box, triclinic boxes, or no r_list_max hint); WRAP = false trusts the staged
// image (the common case).
template<class E, int TPP, int CAP, bool VIRIAL, bool SINGLE, bool XPLOR, bool WRAP>
__device__ __forceinline__ void tiled_loop(const TiledKArgs& a, const char* bx, const char* bt,
                                           const typename E::Coeff* __restrict__ s_coeff,
                                           const double* __restrict__ s_ronsq, const typename E::Coeff& c0, double ronsq0,
                                           double rcutsq_max, const char* __restrict__ slice_base, uint32_t lane_off, uint32_t Kb,
                                           double3 pi, int typei, double& fx, double& fy, double& fz, double& pe, double (&v)[6], uint32_t& n_core,
                                           uint32_t& n_in, double (&es)[2])
    {
    const uint4 zero4 = make_uint4(0, 0, 0, 0);
    // chunk kk of this lane: uniform base + kk KiB (scalar) + 16 lane (one VGPR)
    auto chunk_at = [&](uint32_t kk) -> uint4
        { return *reinterpret_cast<const uint4*>(slice_base + (uint64_t)kk * 1024u + lane_off); };
    // (prefetching the chunk indices two iterations ahead instead of one costs 9 more
    // spilled registers and measures 3 % slower)
    const uint32_t K = Kb >> 1;         // whole iterations
    const uint32_t Kc = (Kb + 1u) >> 1; // chunks this lane reads (the last one only its first half when Kb is odd)
    uint4 u = (Kc > 0) ? chunk_at(0) : zero4;
    uint4 un = (Kc > 1) ? chunk_at(1) : u;
    TileBatch A, B;
    tile_gather<CAP, 0>(A, u, bx);
    for (uint32_t kk = 0; kk < K; ++kk)
        {
        // indices two chunks ahead (consumed 1.5 iterations from now: one iteration
        // does not always cover an HBM round trip); past the end the last chunk is
        // reloaded (an unconditional 16-byte load: a predicated one is split into
        // four 4-byte loads)
        const uint4 un2 = chunk_at((kk + 2 < Kc) ? kk + 2 : Kc - 1);
        tile_gather<CAP, 1>(B, u, bx);
        __builtin_amdgcn_sched_barrier(0);
        tile_compute<E, CAP, VIRIAL, SINGLE, XPLOR, WRAP>(A, a, bt, s_coeff, s_ronsq, c0, ronsq0, rcutsq_max, pi, typei, fx, fy, fz, pe, v, n_core, n_in, es);
        __builtin_amdgcn_sched_barrier(0);
        tile_gather<CAP, 0>(A, un, bx); // when kk + 1 == Kc: gathered, never used
        __builtin_amdgcn_sched_barrier(0);
        tile_compute<E, CAP, VIRIAL, SINGLE, XPLOR, WRAP>(B, a, bt, s_coeff, s_ronsq, c0, ronsq0, rcutsq_max, pi, typei, fx, fy, fz, pe, v, n_core, n_in, es);
        __builtin_amdgcn_sched_barrier(0);
        u = un;
        un = un2;
        }
    if (Kb & 1u) // A holds the first half of chunk K
        tile_compute<E, CAP, VIRIAL, SINGLE, XPLOR, WRAP>(A, a, bt, s_coeff, s_ronsq, c0, ronsq0, rcutsq_max, pi, typei, fx, fy, fz, pe, v, n_core, n_in, es);
    }

// The loop of the split-energy instances where the staged image is trusted (no per-pair minimum image), in two
// phases: rows list class core first, and Kcore whole iterations cover every entry of that class in the slice. When
// the launch states that no other entry can have come inside the evaluator's core (plan_core_reach_sq), the iterations
// from Kcore on run the tail form alone, without the core test: the form that test would have picked for them, so
// the bits are the same. Kcore >= Kb / 2: every batch tested, as in tiled_loop (any other launch). The pipeline is
// tiled_loop's; one iteration body serves both phases. What differs from tiled_loop is bookkeeping only (no arithmetic
// operation, no order of a sum): the chunk load's address, the names of the index words and where c6_lam lives.
template<class E, int TPP, int CAP, bool VIRIAL>
__device__ __forceinline__ void tiled_loop_phases(const TiledKArgs& a, const char* bx, const typename E::Coeff& c0, double rcutsq_max,
                                                  const char* __restrict__ slice_base, uint32_t lane_off, uint32_t Kb, uint32_t Kcore,
                                                  double3 pi, int typei, double& fx, double& fy, double& fz, double& pe, double (&v)[6],
                                                  uint32_t& n_core, uint32_t& n_in, double (&es)[2])
    {
    const uint4 zero4 = make_uint4(0, 0, 0, 0);
    // chunk kk of this lane: the chunk's base (slice base + kk KiB) stays in SGPRs and the lane part (16 lane, below
    // 1 KiB) in one VGPR -- global_load_dwordx4 v, v_off, s[base:base+1], no vector address arithmetic in the loop. The
    // empty asm names the base as a scalar and the lane part as a 32-bit vector at the load: without it the compiler
    // keeps slice base + lane as a 64-bit vector outside the loop and adds the chunk offset to it with one VALU
    // instruction per chunk. (The lane part is carried through the asm from load to load, so no copy is made of it;
    // the pointer is named global again, the asm hides where it came from.)
    uint32_t lane_part = lane_off;
    auto chunk_at = [&](uint32_t kk) -> uint4
        {
        uint64_t chunk_base = reinterpret_cast<uint64_t>(slice_base) + (uint64_t)kk * 1024u;
        asm("" : "+s"(chunk_base), "+v"(lane_part));
        typedef uint32_t words4 __attribute__((ext_vector_type(4)));
        typedef const __attribute__((address_space(1))) char* gptr;
        const words4 w = *reinterpret_cast<const __attribute__((address_space(1))) words4*>(reinterpret_cast<gptr>(chunk_base) + lane_part);
        return make_uint4(w.x, w.y, w.z, w.w);
        };
    const uint32_t K = Kb >> 1;         // whole iterations
    const uint32_t Kc = (Kb + 1u) >> 1; // chunks this lane reads (the last one only its first half when Kb is odd)
    // the index words of the chunk in work, of the next one and of the one after it: three names that rotate through
    // the unrolled loops below (no register copies)
    uint4 u = (Kc > 0) ? chunk_at(0) : zero4;
    uint4 un = (Kc > 1) ? chunk_at(1) : u;
    uint4 un2;
    TileBatch A, B;
    tile_gather<CAP, 0>(A, u, bx);
    // the tail phase's copy of the coefficients keeps c6_lam in a VGPR pair (the one the chunk address used to hold):
    // v_fma_f64 cannot take c12_lam and c6_lam both from SGPRs, and the compiler otherwise copies one of them into
    // VGPRs once per batch
    typename E::Coeff ct = c0;
    if constexpr (!VIRIAL) // (with the virial's six accumulators the pair costs up to three spill slots)
        E::tail_resident(ct);
    // one iteration: chunk kk in w0 (its first half gathered in A), chunk kk + 1 in w1; the words two chunks ahead are
    // loaded into w2
    auto iteration = [&](auto tail_tag, const uint32_t kk, const uint4& w0, const uint4& w1, uint4& w2)
        {
        constexpr bool TAIL = decltype(tail_tag)::value;
        w2 = chunk_at((kk + 2 < Kc) ? kk + 2 : Kc - 1);
        tile_gather<CAP, 1>(B, w0, bx);
        __builtin_amdgcn_sched_barrier(0);
        tile_compute<E, CAP, VIRIAL, true, false, false, TAIL>(A, a, nullptr, nullptr, nullptr, TAIL ? ct : c0, 0.0, rcutsq_max, pi, typei, fx, fy, fz, pe, v, n_core, n_in, es);
        __builtin_amdgcn_sched_barrier(0);
        tile_gather<CAP, 0>(A, w1, bx); // when kk + 1 == Kc: gathered, never used
        __builtin_amdgcn_sched_barrier(0);
        tile_compute<E, CAP, VIRIAL, true, false, false, TAIL>(B, a, nullptr, nullptr, nullptr, TAIL ? ct : c0, 0.0, rcutsq_max, pi, typei, fx, fy, fz, pe, v, n_core, n_in, es);
        __builtin_amdgcn_sched_barrier(0);
        };
    // iterations [kk, kend) of one phase. Tail phase: three at a time with the names rotating, the left-over one or two
    // through a single-iteration body that moves them. The core phase is two iterations long in the mean (the plan's
    // core count), so a three-iteration body would hardly ever be entered; it keeps the single-iteration body alone
    // (unrolled as well, the hot instance grows by another 8 KB of code).
    auto phase = [&](auto tail_tag, uint32_t kk, const uint32_t kend)
        {
        if constexpr (decltype(tail_tag)::value)
            {
            for (; kk + 3 <= kend; kk += 3)
                {
                iteration(tail_tag, kk, u, un, un2);
                iteration(tail_tag, kk + 1, un, un2, u);
                iteration(tail_tag, kk + 2, un2, u, un);
                }
            }
        for (; kk < kend; ++kk)
            {
            iteration(tail_tag, kk, u, un, un2);
            u = un;
            un = un2;
            }
        };
    const uint32_t K1 = (Kcore < K) ? Kcore : K; // iterations of the core phase
    phase(std::false_type(), 0, K1);
    phase(std::true_type(), K1, K);
    // A holds the first half of chunk K (the tested form serves either phase)
    if (Kb & 1u)
        tile_compute<E, CAP, VIRIAL, true, false, false>(A, a, nullptr, nullptr, nullptr, c0, 0.0, rcutsq_max, pi, typei, fx, fy, fz, pe, v, n_core, n_in, es);
    }
// Two bodies, chosen at compile time. The split-energy instances with one lane per particle (one type, no xplor:
// PerturbedLJ with the lanes per particle both plan compilers default to, what the benchmark and an MD run launch) get
// the loads-first set-up, the
// two staging forms and the core / tail phases (header comment, steps 0 - 2). Every other instance keeps the earlier
// order -- per-wave argument tests, coefficients, staging that asks per axis, row words behind the barrier, one loop:
// the new set-up costs Hertz, xplor and several-type instances, and two virial instances with four lanes per particle,
// a spill slot of 8 - 12 B per lane (profiles/tile_setup.md).
template<class E, int TPP, int CAP, bool VIRIAL, bool SINGLE, bool XPLOR>
__global__ void __launch_bounds__(256, E::kTileWaves) pair_forces_tiled_kernel(const TiledKArgs a, const typename E::Params* __restrict__ params)
    {
    if constexpr (TPP == 1 && SINGLE && !XPLOR && E::kSplitEnergy)
        {
        // (one lane per particle, one type, no xplor: no type table, no per-type coefficients, no lane groups)
        typedef typename E::Coeff Coeff;
        constexpr int TB = 256;
        extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
        double* s_x = reinterpret_cast<double*>(s_raw);
        double* s_y = s_x + AZP_TILE_STRIDE(CAP);
        double* s_z = s_y + AZP_TILE_STRIDE(CAP);

        const uint32_t tid = threadIdx.x;
        // A new tile's waves share their SIMDs with three older waves that are deep in
        // the pair loop; raise the priority while staging so the short prologue is not
        // starved (tools/timeline.py: the staging took 17 of a tile's 41 us).
        __builtin_amdgcn_s_setprio(3);
#ifdef AZP_TIMELINE
        const unsigned long long tl_t0 = __builtin_amdgcn_s_memrealtime();
        const unsigned long long tl_c0 = __builtin_amdgcn_s_memtime(); // shader clock
        unsigned long long tl_tb = 0, tl_tc = 0, tl_td = 0, tl_ta = 0;
#endif
        // a.p.first / a.p.end are tile-aligned outwards by the launcher
        const uint32_t tile = a.p.first / TB + xcd_remap(blockIdx.x, a.p.nblocks_padded);
        const uint32_t first = tile * TB;
        if (first >= a.p.end)
            return;
        const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), lane = tid & 63; // wave id: scalar
        const uint32_t slice = tile * 4 + wave;

        // ---- loads first: the uniform words of the tile are scalar loads (load_uniform) -- its stage range, the
        // reference particle, the slice's row, and the words a speculative launch has to look at (a pointer that is not
        // set reads a word of the plan that is there anyway: no branch; the word is then ignored). Only the stage range is
        // waited for ahead of the stage-index loads; the other words travel beside them. From kernel entry to the
        // first position load: arguments -> stage range -> stage indices -> positions.
        const uint32_t n_stage = load_uniform(a.tile_nstage + tile);
        const uint64_t stage_head = load_uniform(a.tile_head + tile);
        asm volatile("" ::"s"(n_stage), "s"(stage_head)); // (both words of the stage range in one group, one wait)
        const uint32_t* __restrict__ stage = a.stage_idx + stage_head;
        const uint32_t* spare = a.tile_nstage + tile;
        const uint32_t w_stale = load_uniform(a.dyn ? &a.dyn->stale : spare);
        const uint32_t w_shells = load_uniform(a.dyn ? &a.dyn->n_shells : spare);
        const uint32_t w_flag = load_uniform(a.dflag ? a.dflag : spare);
        const unsigned long long w_bits = load_uniform(a.dbits ? a.dbits : reinterpret_cast<const unsigned long long*>(a.tile_head + tile));
        const double3 c = make_double3(load_uniform(a.p.pos + 4ull * first), load_uniform(a.p.pos + 4ull * first + 1),
                                       load_uniform(a.p.pos + 4ull * first + 2));
        const uint64_t slice_head = load_uniform(a.slice_head + slice);
        // this lane's own particle (balanced plans: lane -> member of the tile)
        const uint8_t member = *(a.perm ? a.perm + ((uint64_t)tile * 256u + tid) : reinterpret_cast<const uint8_t*>(spare));
        // All loads of the staging are issued before the first result is used: the index
        // loads of every round first, then every position load (two dependent HBM round
        // trips per tile instead of two per 256 staged particles -- the staging took 17 of
        // a tile's 41 us when it was written as a plain loop, tools/timeline.py).
        constexpr int ROUNDS = (CAP + 255) / 256; // n_stage < CAP
        uint32_t sj[ROUNDS];
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r)
            {
            const uint32_t sidx = (uint32_t)r * 256u + tid;
            sj[r] = (sidx < n_stage) ? stage[sidx] : first; // out-of-range lanes load the reference particle (unused)
            }
        // a barrier for the instruction scheduler: what follows (the shell arithmetic of a launch with dbits first of all)
        // stays behind the stage-index loads
        __builtin_amdgcn_sched_barrier(0);
        const uint32_t idx = first + (a.perm ? (uint32_t)member : wave * 64u + lane);
        const bool active = idx < a.p.end;
        // speculative launch on a plan that turned out stale, or whose list has to be rebuilt first (the distance check said
        // so): the whole grid leaves (uniform), before anything is stored
        // (no short-circuit: both words are read in the same group)
        if (((a.dyn != nullptr) & (w_stale != 0u)) | ((a.dflag != nullptr) & (w_flag != 0u)))
            return;
#ifdef AZP_TIMELINE
        __builtin_amdgcn_s_waitcnt(0); // all counters
        tl_tb = __builtin_amdgcn_s_memrealtime();
#endif
        // the slice's row: iterations of the core phase, and the length for the shells the launch has to walk. Scalar
        // trip count, in batches of 4 pairs (the loop counter and the chunk address stay in SGPRs); with a displacement
        // bound the row ends early: entries that were at least 2 x bound outside the cutoff when the plan was built cannot be
        // in range. The shells come from the arguments, or from the words of the list's check (the length is then one more
        // scalar round trip, beside the stage indices'); per-particle displacements replace the length behind the barrier.
        uint32_t n_shells = a.dyn ? min(w_shells, PLAN_SHELLS) : a.n_shells;
        if (a.dbits)
            n_shells = tile_shells_for(to_uniform(sqrt(__longlong_as_double((long long)w_bits)) + a.bound_extra), a.shell_winv);
        uint32_t Kb = load_uniform(a.slice_Kend + ((PLAN_SHELLS + 1) * slice + min(n_shells, PLAN_SHELLS)));
        uint32_t Kcore = load_uniform(a.core_reach_sq > 0.0 ? a.slice_Kphase + slice : spare);

        // ---- coefficients (while the stage indices are on their way; the cutoff is a scalar load like the words above, so
        // no wait for a vector load stands between the stage-index loads and the position loads). One type, no xplor: the
        // launcher picks these instances for shift modes none and shift only (prepare_coeff's xplor clause cannot apply).
        const Coeff c0 = to_uniform(E::prepare(params[0], load_uniform(a.p.rcutsq), a.p.shift_mode == AZP_SHIFT_SHIFT)); // SGPRs
        const double rcutsq_max = c0.rcutsq; // the evaluator's own (effective) cutoff: one compare serves both tests
        // tail phase from iteration Kcore on: only when no entry outside row class core can be inside the evaluator's core
        if (!(a.core_reach_sq > 0.0 && c0.wca_rsq <= a.core_reach_sq))
            Kcore = 0xffffffffu;
        // The compiler sinks scalar loads to their first use, which for the reference particle and the row words lies behind
        // the wait for the stage indices: one more round trip ahead of the position loads. Asking for the values here keeps
        // those loads, and their wait, beside the stage indices' round trip.
        asm volatile("" ::"s"(c.x), "s"(c.y), "s"(c.z), "s"(slice_head), "s"(Kb), "s"(Kcore), "s"(a.fast_stage), "s"(a.p.pos));
        __builtin_amdgcn_sched_barrier(0);
#ifdef AZP_TIMELINE
        tl_ta = __builtin_amdgcn_s_memrealtime();
#endif
        if (tid == 0)
            {
            s_x[0] = PLAN_FAR; s_y[0] = PLAN_FAR; s_z[0] = PLAN_FAR;
            }

        // ---- stage: positions shifted to the periodic image nearest the tile's reference particle c, and this lane's
        // own particle in the same image frame. Two forms, chosen by TiledKArgs::fast_stage (uniform over the launch):
        // every axis shifted without asking and positions addressed with 32-bit offsets, or asking per axis.
        // Without the r_list_max hint (callers that only have HOOMD's pair_args_t) the tile is
        // "compact" when every staged image and every member lies within L / 4 of the reference
        // particle on each periodic axis: then any two of them are closer than L / 2 per axis, so
        // the staged image of a neighbor IS its minimum image for every member.
        double3 pi = make_double3(0.0, 0.0, 0.0);
        bool lane_wide = false;
        float dmax = 0.f; // largest displacement among what this lane stages, and its own
        const uint32_t me = active ? idx : first;
        if (a.disp)
            {
            // (lanes beyond the staged set read the reference particle's entry: a member of the tile anyway)
            dmax = a.disp[me];
#pragma unroll
            for (int r = 0; r < ROUNDS; ++r)
                dmax = fmaxf(dmax, a.disp[sj[r]]);
            }
        double sxv[ROUNDS], syv[ROUNDS], szv[ROUNDS];
        if (a.fast_stage)
            {
            const double3 own = load_scalar3_of4_o32(a.p.pos, me);
#pragma unroll
            for (int r = 0; r < ROUNDS; ++r)
                {
                const double3 pj = load_scalar3_of4_o32(a.p.pos, sj[r]);
                sxv[r] = pj.x; syv[r] = pj.y; szv[r] = pj.z;
                }
#ifdef AZP_TIMELINE
            __builtin_amdgcn_s_waitcnt(0);
            tl_tc = __builtin_amdgcn_s_memrealtime();
#endif
#pragma unroll
            for (int r = 0; r < ROUNDS; ++r)
                {
                const uint32_t sidx = (uint32_t)r * 256u + tid;
                if (sidx < n_stage)
                    {
                    s_x[sidx + 1] = __builtin_fma(-a.p.box.Lx, rint((sxv[r] - c.x) * a.p.box.Lxinv), sxv[r]);
                    s_y[sidx + 1] = __builtin_fma(-a.p.box.Ly, rint((syv[r] - c.y) * a.p.box.Lyinv), syv[r]);
                    s_z[sidx + 1] = __builtin_fma(-a.p.box.Lz, rint((szv[r] - c.z) * a.p.box.Lzinv), szv[r]);
                    }
                }
            if (active)
                {
                const double x = __builtin_fma(-a.p.box.Lx, rint((own.x - c.x) * a.p.box.Lxinv), own.x);
                const double y = __builtin_fma(-a.p.box.Ly, rint((own.y - c.y) * a.p.box.Lyinv), own.y);
                const double z = __builtin_fma(-a.p.box.Lz, rint((own.z - c.z) * a.p.box.Lzinv), own.z);
                // every member closer to c than L / 2 minus the largest possible pair separation: see below
                lane_wide = (fabs(x - c.x) + a.p.r_list_max >= 0.5 * a.p.box.Lx) || (fabs(y - c.y) + a.p.r_list_max >= 0.5 * a.p.box.Ly)
                            || (fabs(z - c.z) + a.p.r_list_max >= 0.5 * a.p.box.Lz);
                pi = make_double3(x, y, z);
                }
            }
        else
            {
            const double3 own = load_scalar3_of4(a.p.pos, me);
            const bool no_hint = !(a.p.r_list_max > 0.0);
            bool far_from_c = false;
#pragma unroll
            for (int r = 0; r < ROUNDS; ++r)
                {
                const double3 pj = load_scalar3_of4(a.p.pos, sj[r]);
                sxv[r] = pj.x; syv[r] = pj.y; szv[r] = pj.z;
                }
#ifdef AZP_TIMELINE
            __builtin_amdgcn_s_waitcnt(0);
            tl_tc = __builtin_amdgcn_s_memrealtime();
#endif
#pragma unroll
            for (int r = 0; r < ROUNDS; ++r)
                {
                const uint32_t sidx = (uint32_t)r * 256u + tid;
                if (sidx < n_stage)
                    {
                    double x = sxv[r], y = syv[r], z = szv[r];
                    if (!a.p.box.triclinic)
                        {
                        if (a.p.box.px) x = __builtin_fma(-a.p.box.Lx, rint((x - c.x) * a.p.box.Lxinv), x);
                        if (a.p.box.py) y = __builtin_fma(-a.p.box.Ly, rint((y - c.y) * a.p.box.Lyinv), y);
                        if (a.p.box.pz) z = __builtin_fma(-a.p.box.Lz, rint((z - c.z) * a.p.box.Lzinv), z);
                        if (no_hint)
                            far_from_c = far_from_c || (a.p.box.px && fabs(x - c.x) >= 0.25 * a.p.box.Lx)
                                         || (a.p.box.py && fabs(y - c.y) >= 0.25 * a.p.box.Ly)
                                         || (a.p.box.pz && fabs(z - c.z) >= 0.25 * a.p.box.Lz);
                        }
                    s_x[sidx + 1] = x; s_y[sidx + 1] = y; s_z[sidx + 1] = z;
                    }
                }
            // Fast path condition, per tile: every member is closer to c than L/2 minus
            // the largest possible pair separation, so the staged image of each listed
            // neighbor IS its minimum image. Otherwise every pair is re-imaged.
            lane_wide = far_from_c || a.p.box.triclinic;
            if (active)
                {
                double x = own.x, y = own.y, z = own.z;
                if (!a.p.box.triclinic)
                    {
                    if (a.p.box.px) x = __builtin_fma(-a.p.box.Lx, rint((x - c.x) * a.p.box.Lxinv), x);
                    if (a.p.box.py) y = __builtin_fma(-a.p.box.Ly, rint((y - c.y) * a.p.box.Lyinv), y);
                    if (a.p.box.pz) z = __builtin_fma(-a.p.box.Lz, rint((z - c.z) * a.p.box.Lzinv), z);
                    // (without the hint r_reach = L / 4: the member itself has to be within L / 4 of c)
                    const double rx = no_hint ? 0.25 * a.p.box.Lx : a.p.r_list_max, ry = no_hint ? 0.25 * a.p.box.Ly : a.p.r_list_max,
                                 rz = no_hint ? 0.25 * a.p.box.Lz : a.p.r_list_max;
                    lane_wide = lane_wide || (a.p.box.px && fabs(x - c.x) + rx >= 0.5 * a.p.box.Lx)
                                || (a.p.box.py && fabs(y - c.y) + ry >= 0.5 * a.p.box.Ly)
                                || (a.p.box.pz && fabs(z - c.z) + rz >= 0.5 * a.p.box.Lz);
                    }
                pi = make_double3(x, y, z);
                }
            }
#ifdef AZP_TIMELINE
        __builtin_amdgcn_s_waitcnt(0);
        tl_td = __builtin_amdgcn_s_memrealtime();
#endif
        __shared__ float s_dmax[4];
        if (a.disp)
            {
            dmax = wave_max_nonneg(dmax);
            if (lane == 0)
                s_dmax[wave] = dmax;
            }
        const bool wide = __syncthreads_or(lane_wide); // also publishes the staged tile
        __builtin_amdgcn_s_setprio(0);
#ifdef AZP_TIMELINE
        const unsigned long long tl_t1 = __builtin_amdgcn_s_memrealtime();
#endif
        if (a.disp)
            {
            // per-particle displacements: the shells THIS tile has to walk, and the row end for them
            const float d4 = fmaxf(fmaxf(s_dmax[0], s_dmax[1]), fmaxf(s_dmax[2], s_dmax[3]));
            const uint32_t tile_shells = tile_shells_for(to_uniform((double)d4 + a.bound_extra), a.shell_winv); // NaN / inf: whole rows
            Kb = to_uniform(a.slice_Kend[(PLAN_SHELLS + 1) * slice + min(tile_shells, PLAN_SHELLS)]);
            }
        // wave-uniform slice base (SGPRs) + lane: the loads use scalar-base addressing
        const char* __restrict__ slice_base = reinterpret_cast<const char*>(a.cnl + slice_head * 64ull);
        const uint32_t lane_off = lane * 16u;

        double fx = 0.0, fy = 0.0, fz = 0.0, pe = 0.0;
        double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        uint32_t n_core = 0, n_in = 0;
        double es[2] = {0.0, 0.0}; // tail-path energy sums (EvalPLJ::eval_split_tail)
        const char* bx = reinterpret_cast<const char*>(s_x);
        if (wide)
            tiled_loop<E, 1, CAP, VIRIAL, true, false, true>(a, bx, nullptr, nullptr, nullptr, c0, 0.0, rcutsq_max, slice_base, lane_off, Kb, pi, 0,
                                                             fx, fy, fz, pe, v, n_core, n_in, es);
        else
            tiled_loop_phases<E, 1, CAP, VIRIAL>(a, bx, c0, rcutsq_max, slice_base, lane_off, Kb, Kcore, pi, 0, fx, fy, fz, pe, v, n_core,
                                                 n_in, es);
        pe = E::finish_split(c0, pe, es[0], es[1], n_core, n_in);

#ifdef AZP_TIMELINE
        if (lane == 0 && tile < 16384)
            {
            unsigned long long* t = g_timeline + (tile * 4 + wave) * 8;
            t[4] = tl_ta; t[5] = tl_tb; t[6] = tl_tc; t[7] = tl_td;
            if (wave == 3)
                t[4] = __builtin_amdgcn_s_memtime() - tl_c0; // wave 3 reports shader-clock ticks over its lifetime
            t[0] = tl_t0; t[1] = tl_t1; t[2] = __builtin_amdgcn_s_memrealtime();
            t[3] = ((unsigned long long)__builtin_amdgcn_s_getreg((20 /*XCC_ID*/) | (0 << 6) | (31 << 11)) << 32)
                   | (unsigned)__builtin_amdgcn_s_getreg((4 /*HW_ID*/) | (0 << 6) | (31 << 11));
            }
#endif
        // (one lane per particle: nothing to sum over lanes)
        if (active)
            {
            store_scalar4(a.p.force, idx, fx, fy, fz, 0.5 * pe);
            if (VIRIAL)
                {
#pragma unroll
                for (int cidx = 0; cidx < 6; ++cidx)
                    a.p.virial[(uint64_t)cidx * a.p.virial_pitch + idx] = 0.5 * v[cidx];
                }
            }
        }
    else
        {
        typedef typename E::Coeff Coeff;
        constexpr int TB = 256 / TPP;
        constexpr int PW = 64 / TPP;
        extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
        double* s_x = reinterpret_cast<double*>(s_raw);
        double* s_y = s_x + AZP_TILE_STRIDE(CAP);
        double* s_z = s_y + AZP_TILE_STRIDE(CAP);
        int* s_t = reinterpret_cast<int*>(s_z + AZP_TILE_STRIDE(CAP)); // CAP ints, only when !SINGLE
        Coeff* s_coeff = reinterpret_cast<Coeff*>(s_raw + (size_t)AZP_TILE_STRIDE(CAP) * 24 + (SINGLE ? 0 : (size_t)CAP * 4 + 8));
        double* s_ronsq = reinterpret_cast<double*>(s_coeff + (SINGLE ? 0 : a.p.ntypes * a.p.ntypes));

        const uint32_t tid = threadIdx.x;
        // A new tile's waves share their SIMDs with three older waves that are deep in
        // the pair loop; raise the priority while staging so the short prologue is not
        // starved (tools/timeline.py: the staging took 17 of a tile's 41 us).
        __builtin_amdgcn_s_setprio(3);
#ifdef AZP_TIMELINE
        const unsigned long long tl_t0 = __builtin_amdgcn_s_memrealtime();
        const unsigned long long tl_c0 = __builtin_amdgcn_s_memtime(); // shader clock
        unsigned long long tl_tb = 0, tl_tc = 0, tl_td = 0, tl_ta = 0;
#endif
        // a.p.first / a.p.end are tile-aligned outwards by the launcher
        const uint32_t tile = a.p.first / TB + xcd_remap(blockIdx.x, a.p.nblocks_padded);
        const uint32_t first = tile * TB;
        if (first >= a.p.end)
            return;
        if (a.dyn && a.dyn->stale) // speculative launch on a plan that turned out stale (uniform: whole grid leaves)
            return;
        if (a.dflag && *a.dflag)   // ... or whose list has to be rebuilt first (the distance check said so)
            return;

        Coeff c0;
        double ronsq0 = 0.0;
        double rcutsq_max = 0.0; // largest cutoff^2 over the type pairs: bound for the skip test
        if (SINGLE)
            {
            c0 = to_uniform(prepare_coeff<E>(a.p, params, 0)); // same for every lane: keep it in SGPRs
            if (XPLOR)
                ronsq0 = a.p.ronsq[0];
            rcutsq_max = c0.rcutsq; // the evaluator's own (effective) cutoff: one compare serves both tests
            }
        else
            {
            const uint32_t ntp = a.p.ntypes * a.p.ntypes;
            for (uint32_t t = tid; t < ntp; t += 256)
                {
                s_coeff[t] = prepare_coeff<E>(a.p, params, t);
                s_ronsq[t] = XPLOR ? a.p.ronsq[t] : 0.0;
                }
            for (uint32_t t = 0; t < ntp; ++t)
                rcutsq_max = fmax(rcutsq_max, a.p.rcutsq[t]);
            }

#ifdef AZP_TIMELINE
        tl_ta = __builtin_amdgcn_s_memrealtime();
#endif
        // ---- stage: positions shifted to the periodic image nearest the tile's
        // reference particle c ----
        const uint32_t n_stage = a.tile_nstage[tile];
        const uint32_t* __restrict__ stage = a.stage_idx + a.tile_head[tile];
        const double3 c = load_scalar3_of4(a.p.pos, first);
        if (tid == 0)
            {
            s_x[0] = PLAN_FAR; s_y[0] = PLAN_FAR; s_z[0] = PLAN_FAR;
            if (!SINGLE) s_t[0] = 0;
            }
        // this lane's own particle: its load is issued first and consumed after the staging
        const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), lane = tid & 63; // wave id: scalar
        const uint32_t pl = lane / TPP;
        const uint32_t idx = first + ((TPP == 1 && a.perm) ? (uint32_t)a.perm[(uint64_t)tile * 256u + tid] : wave * PW + pl);
        const bool active = idx < a.p.end;
        const double4 own = load_scalar4(a.p.pos, active ? idx : first);
        // All loads of the staging are issued before the first result is used: the index
        // loads of every round first, then every position load (two dependent HBM round
        // trips per tile instead of two per 256 staged particles -- the staging took 17 of
        // a tile's 41 us when it was written as a plain loop, tools/timeline.py).
        // Without the r_list_max hint (callers that only have HOOMD's pair_args_t) the tile is
        // "compact" when every staged image and every member lies within L / 4 of the reference
        // particle on each periodic axis: then any two of them are closer than L / 2 per axis, so
        // the staged image of a neighbor IS its minimum image for every member.
        const bool no_hint = !(a.p.r_list_max > 0.0);
        bool far_from_c = false;
        float dmax = a.disp ? a.disp[active ? idx : first] : 0.f; // largest displacement among what this lane stages, and its own
        {
        constexpr int ROUNDS = (CAP + 255) / 256; // n_stage < CAP
        uint32_t sj[ROUNDS];
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r)
            {
            const uint32_t sidx = (uint32_t)r * 256u + tid;
            sj[r] = (sidx < n_stage) ? stage[sidx] : first; // out-of-range lanes load the reference particle (unused)
            }
#ifdef AZP_TIMELINE
        __builtin_amdgcn_s_waitcnt(0); // all counters
        tl_tb = __builtin_amdgcn_s_memrealtime();
#endif
        double sxv[ROUNDS], syv[ROUNDS], szv[ROUNDS];
        int stv[ROUNDS];
        if (a.disp)
            {
            // (lanes beyond the staged set read the reference particle's entry: a member of the tile anyway)
#pragma unroll
            for (int r = 0; r < ROUNDS; ++r)
                dmax = fmaxf(dmax, a.disp[sj[r]]);
            }
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r)
            {
            if (SINGLE)
                {
                const double3 pj = load_scalar3_of4(a.p.pos, sj[r]);
                sxv[r] = pj.x; syv[r] = pj.y; szv[r] = pj.z;
                }
            else
                {
                const double4 pj = load_scalar4(a.p.pos, sj[r]);
                sxv[r] = pj.x; syv[r] = pj.y; szv[r] = pj.z;
                stv[r] = type_from_w(pj.w);
                }
            }
#ifdef AZP_TIMELINE
        __builtin_amdgcn_s_waitcnt(0);
        tl_tc = __builtin_amdgcn_s_memrealtime();
#endif
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r)
            {
            const uint32_t sidx = (uint32_t)r * 256u + tid;
            if (sidx < n_stage)
                {
                double x = sxv[r], y = syv[r], z = szv[r];
                if (!a.p.box.triclinic)
                    {
                    if (a.p.box.px) x = __builtin_fma(-a.p.box.Lx, rint((x - c.x) * a.p.box.Lxinv), x);
                    if (a.p.box.py) y = __builtin_fma(-a.p.box.Ly, rint((y - c.y) * a.p.box.Lyinv), y);
                    if (a.p.box.pz) z = __builtin_fma(-a.p.box.Lz, rint((z - c.z) * a.p.box.Lzinv), z);
                    if (no_hint)
                        far_from_c = far_from_c || (a.p.box.px && fabs(x - c.x) >= 0.25 * a.p.box.Lx)
                                     || (a.p.box.py && fabs(y - c.y) >= 0.25 * a.p.box.Ly)
                                     || (a.p.box.pz && fabs(z - c.z) >= 0.25 * a.p.box.Lz);
                    }
                s_x[sidx + 1] = x; s_y[sidx + 1] = y; s_z[sidx + 1] = z;
                if (!SINGLE)
                    s_t[sidx + 1] = stv[r];
                }
            }
        }

        // ---- this lane's particle, in the same image frame ----
        double3 pi = make_double3(0.0, 0.0, 0.0);
        int typei = 0;
        // Fast path condition, per tile: every member is closer to c than L/2 minus
        // the largest possible pair separation, so the staged image of each listed
        // neighbor IS its minimum image. Otherwise every pair is re-imaged.
        bool lane_wide = far_from_c || a.p.box.triclinic;
        if (active)
            {
            const double4 p = own;
            double x = p.x, y = p.y, z = p.z;
            if (!a.p.box.triclinic)
                {
                if (a.p.box.px) x = __builtin_fma(-a.p.box.Lx, rint((x - c.x) * a.p.box.Lxinv), x);
                if (a.p.box.py) y = __builtin_fma(-a.p.box.Ly, rint((y - c.y) * a.p.box.Lyinv), y);
                if (a.p.box.pz) z = __builtin_fma(-a.p.box.Lz, rint((z - c.z) * a.p.box.Lzinv), z);
                // (without the hint r_reach = L / 4: the member itself has to be within L / 4 of c)
                const double rx = no_hint ? 0.25 * a.p.box.Lx : a.p.r_list_max, ry = no_hint ? 0.25 * a.p.box.Ly : a.p.r_list_max,
                             rz = no_hint ? 0.25 * a.p.box.Lz : a.p.r_list_max;
                lane_wide = lane_wide || (a.p.box.px && fabs(x - c.x) + rx >= 0.5 * a.p.box.Lx)
                            || (a.p.box.py && fabs(y - c.y) + ry >= 0.5 * a.p.box.Ly)
                            || (a.p.box.pz && fabs(z - c.z) + rz >= 0.5 * a.p.box.Lz);
                }
            pi = make_double3(x, y, z);
            typei = type_from_w(p.w);
            }
#ifdef AZP_TIMELINE
        __builtin_amdgcn_s_waitcnt(0);
        tl_td = __builtin_amdgcn_s_memrealtime();
#endif
        __shared__ float s_dmax[4];
        if (a.disp)
            {
            dmax = wave_max_nonneg(dmax);
            if (lane == 0)
                s_dmax[wave] = dmax;
            }
        const bool wide = __syncthreads_or(lane_wide); // also publishes the staged tile
        __builtin_amdgcn_s_setprio(0);
#ifdef AZP_TIMELINE
        const unsigned long long tl_t1 = __builtin_amdgcn_s_memrealtime();
#endif
        // the shells this tile has to walk
        uint32_t n_shells = a.dyn ? min(a.dyn->n_shells, PLAN_SHELLS) : a.n_shells;
        if (a.dbits)
            n_shells = tile_shells_for(to_uniform(sqrt(__longlong_as_double((long long)*a.dbits)) + a.bound_extra), a.shell_winv);
        if (a.disp)
            {
            const float d4 = fmaxf(fmaxf(s_dmax[0], s_dmax[1]), fmaxf(s_dmax[2], s_dmax[3]));
            n_shells = tile_shells_for(to_uniform((double)d4 + a.bound_extra), a.shell_winv); // NaN / inf displacements: whole rows
            }

        const uint32_t slice = tile * 4 + wave;
        // scalar trip count, in batches of 4 pairs (the loop counter and the chunk address stay in SGPRs).
        // With a displacement bound from the caller the row ends early: entries that were at
        // least 2 x bound outside the cutoff when the plan was built cannot be in range.
        const uint32_t Kb = to_uniform(a.slice_Kend[(PLAN_SHELLS + 1) * slice + min(n_shells, PLAN_SHELLS)]);
        // wave-uniform slice base (SGPRs) + lane: the loads use scalar-base addressing
        const uint64_t slice_head = to_uniform(a.slice_head[slice]);
        const char* __restrict__ slice_base = reinterpret_cast<const char*>(a.cnl + slice_head * 64ull);
        const uint32_t lane_off = lane * 16u;

        double fx = 0.0, fy = 0.0, fz = 0.0, pe = 0.0;
        double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        uint32_t n_core = 0, n_in = 0;
        double es[2] = {0.0, 0.0}; // tail-path energy sums (EvalPLJ::eval_split_tail)
        const char* bx = reinterpret_cast<const char*>(s_x);
        const char* bt = reinterpret_cast<const char*>(s_t);
        if (wide)
            tiled_loop<E, TPP, CAP, VIRIAL, SINGLE, XPLOR, true>(a, bx, bt, s_coeff, s_ronsq, c0, ronsq0, rcutsq_max, slice_base, lane_off, Kb, pi,
                                                                typei, fx, fy, fz, pe, v, n_core, n_in, es);
        else
            tiled_loop<E, TPP, CAP, VIRIAL, SINGLE, XPLOR, false>(a, bx, bt, s_coeff, s_ronsq, c0, ronsq0, rcutsq_max, slice_base, lane_off, Kb, pi,
                                                                 typei, fx, fy, fz, pe, v, n_core, n_in, es);
        if constexpr (SINGLE && !XPLOR && E::kSplitEnergy)
            pe = E::finish_split(c0, pe, es[0], es[1], n_core, n_in);

#ifdef AZP_TIMELINE
        if (lane == 0 && tile < 16384)
            {
            unsigned long long* t = g_timeline + (tile * 4 + wave) * 8;
            t[4] = tl_ta; t[5] = tl_tb; t[6] = tl_tc; t[7] = tl_td;
            if (wave == 3)
                t[4] = __builtin_amdgcn_s_memtime() - tl_c0; // wave 3 reports shader-clock ticks over its lifetime
            t[0] = tl_t0; t[1] = tl_t1; t[2] = __builtin_amdgcn_s_memrealtime();
            t[3] = ((unsigned long long)__builtin_amdgcn_s_getreg((20 /*XCC_ID*/) | (0 << 6) | (31 << 11)) << 32)
                   | (unsigned)__builtin_amdgcn_s_getreg((4 /*HW_ID*/) | (0 << 6) | (31 << 11));
            }
#endif
        fx = group_sum<TPP>(fx);
        fy = group_sum<TPP>(fy);
        fz = group_sum<TPP>(fz);
        pe = group_sum<TPP>(pe);
        if (VIRIAL)
            {
#pragma unroll
            for (int cidx = 0; cidx < 6; ++cidx)
                v[cidx] = group_sum<TPP>(v[cidx]);
            }
        if (active && (lane % TPP) == 0)
            {
            store_scalar4(a.p.force, idx, fx, fy, fz, 0.5 * pe);
            if (VIRIAL)
                {
#pragma unroll
                for (int cidx = 0; cidx < 6; ++cidx)
                    a.p.virial[(uint64_t)cidx * a.p.virial_pitch + idx] = 0.5 * v[cidx];
                }
            }
        }
    }

// Square of the separation below which no entry OUTSIDE row class core can be found under the caller's displacement
// bound b (0: no statement). Both plan compilers file an entry in class core when its single-precision separation is
// below the inner radius r_in (azp_pair_args.d_rinnersq), and both state the margin that test needs as m = 1e-4: every
// other entry was at least plan.core_r = r_in - m away when the plan was built (pair_plan.hip, pair_plan_cells.hip). Two
// particles close in by at most 2 b, so such an entry is now at least core_r - 2 b (1 + 1e-9) away. The kernel takes the
// tail phase when the square of its core radius is <= this value, that is when
//   sqrt(wca_rsq) + 2 b (1 + 1e-9) + m <= r_in   (the 1e-12 covers the roundings of this square and of a separation).
// Launches that learn the displacement on the device (dyn, dflag / dbits, disp) make no statement.
inline double plan_core_reach_sq(const PairPlan& plan, const azp_pair_args& args, const TiledKArgs& k)
    {
    if (!(plan.core_r > 0.f) || !plan.d_slice_Kphase || k.dyn || k.dflag || k.disp)
        return 0.0;
    if (!args.has_displacement_bound || !(args.displacement_bound >= 0.0))
        return 0.0;
    const double reach = (double)plan.core_r - 2.0 * (args.displacement_bound + k.bound_extra) * (1.0 + 1e-9);
    return reach > 0.0 ? reach * reach * (1.0 - 1e-12) : 0.0;
    }

// Arguments of a tile kernel (this one and xtiled.hpp's) for the tiles of tb particles a launch covers: sub-range
// launches are rounded outwards to whole tiles (a tile computed by two launches of one step gets the later launch's
// values: stream order).
inline TiledKArgs make_tiled_kargs(const PairPlan& plan, const azp_pair_args& args, const TileDyn* dyn, uint32_t tb)
    {
    TiledKArgs k = {};
    k.p = make_pair_kargs(args);
    k.tile_nstage = plan.d_tile_nstage;
    k.tile_head = plan.d_tile_head;
    k.stage_idx = plan.d_stage_idx;
    k.perm = plan.balanced ? plan.d_perm : nullptr;
    k.slice_Kend = plan.d_slice_Kend;
    k.n_shells = plan_shells_for(plan, args);
    fill_local_bound(k, plan, args);
    k.dyn = dyn;
    k.slice_head = plan.d_slice_head;
    k.cnl = plan.d_cnl;
    k.slice_Kphase = plan.d_slice_Kphase;
    k.core_reach_sq = plan_core_reach_sq(plan, args, k);
    k.fast_stage = (!k.p.box.triclinic && k.p.box.px && k.p.box.py && k.p.box.pz && k.p.r_list_max > 0.0 && args.n_max < (1u << 27)) ? 1u : 0u;
    const uint32_t t0 = k.p.first / tb, t1 = (k.p.end + tb - 1) / tb;
    k.p.first = t0 * tb;
    k.p.end = (t1 * tb < args.N) ? t1 * tb : args.N;
    k.p.nblocks_padded = (t1 - t0 + 7u) & ~7u;
    return k;
    }

// LDS variant of a launch: from the tiles of tb particles it covers (all of them unless a range is given)
inline uint32_t plan_launch_cap(const PairPlan& plan, const azp_pair_args& args, uint32_t tb)
    {
    if (args.range_count == 0 || plan.h_tile_nstage.empty())
        return plan.cap;
    const uint32_t end = (args.range_first + args.range_count < args.N) ? args.range_first + args.range_count : args.N;
    const uint32_t t0 = args.range_first / tb, t1 = (end + tb - 1) / tb;
    uint32_t most = 0;
    for (uint32_t t = t0; t < t1 && t < plan.n_tiles; ++t)
        most = plan.h_tile_nstage[t] > most ? plan.h_tile_nstage[t] : most;
    return plan_cap_for(most);
    }

template<class E, int TPP, int CAP, bool VIRIAL, bool SINGLE>
int launch_tiled_instance(const PairPlan& plan, const azp_pair_args& args, const typename E::Params* d_params,
                          hipStream_t stream, const TileDyn* dyn)
    {
    const TiledKArgs k = make_tiled_kargs(plan, args, dyn, plan.tile);
    size_t lds = (size_t)AZP_TILE_STRIDE(CAP) * 24 + (SINGLE ? 0 : (size_t)CAP * 4 + 8);
    if (!SINGLE)
        lds += (sizeof(typename E::Coeff) + sizeof(double)) * (size_t)args.ntypes * args.ntypes;
    if (args.shift_mode == AZP_SHIFT_XPLOR)
        return launch_dyn_lds(pair_forces_tiled_kernel<E, TPP, CAP, VIRIAL, SINGLE, true>, k.p.nblocks_padded, 256, TPP, lds, stream, k, d_params);
    return launch_dyn_lds(pair_forces_tiled_kernel<E, TPP, CAP, VIRIAL, SINGLE, false>, k.p.nblocks_padded, 256, TPP, lds, stream, k, d_params);
    }

template<class E, int TPP, bool VIRIAL, bool SINGLE>
int launch_tiled_cap(const PairPlan& plan, const azp_pair_args& args, const typename E::Params* d_params, hipStream_t s, const TileDyn* dyn)
    {
    const uint32_t cap = plan_launch_cap(plan, args, plan.tile);
    switch (cap)
        {
    case 1024: return launch_tiled_instance<E, TPP, 1024, VIRIAL, SINGLE>(plan, args, d_params, s, dyn);
    case 1536: return launch_tiled_instance<E, TPP, 1536, VIRIAL, SINGLE>(plan, args, d_params, s, dyn);
    case 1664: return launch_tiled_instance<E, TPP, 1664, VIRIAL, SINGLE>(plan, args, d_params, s, dyn);
    case 2048: return launch_tiled_instance<E, TPP, 2048, VIRIAL, SINGLE>(plan, args, d_params, s, dyn);
    case 2560: return launch_tiled_instance<E, TPP, 2560, VIRIAL, SINGLE>(plan, args, d_params, s, dyn);
    default: return AZP_ERROR_INVALID_ARGUMENT;
        }
    }

// the tile kernel at the plan's lanes per particle (a plan valid for these arguments: pair_auto.hpp)
template<class E>
int launch_tiled_tpp(const PairPlan& plan, const azp_pair_args& args, const typename E::Params* d_params, hipStream_t s, const TileDyn* dyn)
    {
    const bool single = (args.ntypes == 1);
    auto go = [&](auto t)
        {
        constexpr int TPP = decltype(t)::value;
        if (args.compute_virial)
            return single ? launch_tiled_cap<E, TPP, true, true>(plan, args, d_params, s, dyn)
                          : launch_tiled_cap<E, TPP, true, false>(plan, args, d_params, s, dyn);
        return single ? launch_tiled_cap<E, TPP, false, true>(plan, args, d_params, s, dyn)
                      : launch_tiled_cap<E, TPP, false, false>(plan, args, d_params, s, dyn);
        };
    switch (plan.tpp)
        {
    case 1: return go(std::integral_constant<int, 1>());
    case 2: return go(std::integral_constant<int, 2>());
    case 4: return go(std::integral_constant<int, 4>());
    default: return AZP_ERROR_INVALID_ARGUMENT;
        }
    }

} // namespace azp
