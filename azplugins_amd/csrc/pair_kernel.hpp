// pair_kernel.hpp -- the generic neighbor-list kernel of every pair potential
// (replaces HOOMD's gpu_compute_pair_forces<E>, gpu_compute_dpd_forces<E> and
// gpu_compute_pair_aniso_forces<E>, requested by the reference at
// src/PotentialPairGPUKernel.cu.inc:25-28, src/PotentialPairDPDThermoGPUKernel.cu.inc:21-24
// and src/AnisoPotentialPairGPUKernel.cu.inc:21-25). It runs on the HOOMD-format list
// for explicit threads_per_particle, without an auto plan and for lists that cannot be
// tiled; the tile-staged kernels are in pair_tiled.hpp and xtiled.hpp.
//
// pair_forces_kernel<X, TPP, VIRIAL, SINGLE> knows no potential. A policy class X holds
// the physics: coefficients (prepare), what a pair reads beyond the neighbor's position
// (load_extra: kExtra doubles, a tag with kTag) and of the particle itself (load_own), the
// in-range test, the pair arithmetic, the reduction over lanes and the store. XIso (below)
// adapts the isotropic evaluators of evaluators.hpp; XDPD (dpd_forces.hip) and XTPM
// (aniso_forces.hip) also drive xtiled_kernel.
//
// Mapping (gfx950, wave64):
//   * TPP consecutive lanes cooperate on one particle; a wave covers 64/TPP
//     consecutive particles, so the neighbor-index rows a wave streams are
//     adjacent in memory and every fetched 128-B line is fully consumed.
//   * lanes stride the row: lane s handles entries s, s+TPP, ... ; the next
//     index is prefetched one iteration ahead.
//   * neighbor positions are gathered as 16-B loads and rely on L1 / the
//     XCD's L2 (block -> particle range mapping is XCD-aware); the payload of
//     a neighbor is loaded for in-range pairs only.
//   * per-type-pair coefficients: registers when ntypes == 1, LDS otherwise.
//   * interior waves (every particle farther than r_list_max from all periodic
//     faces) skip the minimum-image arithmetic; the choice is wave-uniform.
//   * FP64 accumulate, DPP butterfly reduction over the TPP lanes, lane 0
//     writes force (fx, fy, fz, e) with two 16-B stores.
#pragma once

#include <type_traits>

#include "evaluators.hpp"
#include "pair_kernel_host.hpp"

namespace azp
{
struct PairKArgs
    {
    double* force;
    double* virial;
    uint64_t virial_pitch;
    const double* pos;
    const uint32_t* n_neigh;
    const uint32_t* nlist;
    const uint64_t* head_list;
    const double* rcutsq;
    const double* ronsq;
    BoxDev box;
    double r_list_max;
    uint32_t N;
    uint32_t ntypes;
    uint32_t shift_mode;
    uint32_t nblocks_padded; // grid size, multiple of 8
    uint32_t first;          // particles [first, end) are computed by this launch
    uint32_t end;
    };

template<class E> __device__ __forceinline__ typename E::Coeff
prepare_coeff(const PairKArgs& a, const typename E::Params* params, uint32_t tp)
    {
    const double rcutsq = a.rcutsq[tp];
    bool energy_shift = (a.shift_mode == AZP_SHIFT_SHIFT);
    if (a.shift_mode == AZP_SHIFT_XPLOR && a.ronsq[tp] > rcutsq)
        energy_shift = true;
    return E::prepare(params[tp], rcutsq, energy_shift);
    }

inline int validate_pair_args(const azp_pair_args* args, const void* d_params)
    {
    if (!args || !d_params) return AZP_ERROR_INVALID_ARGUMENT;
    if (args->N == 0) return 1; // nothing to do (caller returns success)
    if (!args->d_force || !args->d_pos || !args->d_n_neigh || !args->d_nlist || !args->d_head_list || !args->d_rcutsq)
        return AZP_ERROR_INVALID_ARGUMENT;
    if (args->ntypes == 0 || args->shift_mode > AZP_SHIFT_XPLOR) return AZP_ERROR_INVALID_ARGUMENT;
    if (args->shift_mode == AZP_SHIFT_XPLOR && !args->d_ronsq) return AZP_ERROR_INVALID_ARGUMENT;
    if (args->compute_virial && (!args->d_virial || args->virial_pitch < args->N)) return AZP_ERROR_INVALID_ARGUMENT;
    if (args->n_max < args->N) return AZP_ERROR_INVALID_ARGUMENT;
    if (args->block_size && (args->block_size % 64 || args->block_size > 256)) return AZP_ERROR_INVALID_ARGUMENT;
    if (args->range_count && (uint64_t)args->range_first + args->range_count > args->N) return AZP_ERROR_INVALID_ARGUMENT;
    return 0;
    }

// force (fx, fy, fz) and pair energy summed over a particle's neighbors (XIso, XDPD)
struct ForceEnergy
    {
    struct Acc
        {
        double fx, fy, fz, pe;
        };
    static __device__ __forceinline__ void zero(Acc& a) { a.fx = a.fy = a.fz = a.pe = 0.0; }
    template<int TPP> static __device__ __forceinline__ void reduce(Acc& a)
        {
        a.fx = group_sum<TPP>(a.fx);
        a.fy = group_sum<TPP>(a.fy);
        a.fz = group_sum<TPP>(a.fz);
        a.pe = group_sum<TPP>(a.pe);
        }
    template<class KExtra> static __device__ __forceinline__ void store(const Acc& a, const PairKArgs& p, const KExtra&, uint32_t idx)
        {
        store_scalar4(p.force, idx, a.fx, a.fy, a.fz, 0.5 * a.pe);
        }
    };

// An isotropic evaluator E (evaluators.hpp) as a policy: no payload, and every listed pair is evaluated -- E::eval is
// branch-free and gives zero force and energy beyond the cutoff. XPLOR smoothing is a separate instance, chosen per
// call from shift_mode (pair_auto.hpp).
template<class E, bool XPLOR = false> struct XIso : ForceEnergy
    {
    typedef typename E::Params Params;
    struct Coeff
        {
        typename E::Coeff c;
        double ronsq; // (xplor only)
        };
    struct KExtra {};
    struct Own {};
    static constexpr int kExtra = 0;
    static constexpr bool kTag = false;
    static __device__ __forceinline__ Coeff prepare(const Params* params, const PairKArgs& a, uint32_t t, const KExtra&)
        {
        Coeff c;
        c.c = prepare_coeff<E>(a, params, t);
        c.ronsq = XPLOR ? a.ronsq[t] : 0.0;
        return c;
        }
    static __device__ __forceinline__ void load_own(const KExtra&, uint32_t, Own&) {}
    static __device__ __forceinline__ void load_extra(const KExtra&, uint32_t, const double*, uint32_t&) {}
    static __device__ __forceinline__ bool in_range(const Coeff&, double) { return true; }
    template<bool VIRIAL>
    static __device__ __forceinline__ void pair(const Coeff& c, const KExtra&, const Own&, double dx, double dy, double dz, double rsq,
                                                const double*, uint32_t, Acc& a, double (&v)[6])
        {
        double force_divr, pair_eng;
        const bool evaluated = E::eval(c.c, rsq, force_divr, pair_eng);
        if (XPLOR && evaluated)
            apply_xplor(rsq, c.ronsq, c.c.rcutsq, force_divr, pair_eng);
        a.fx = __builtin_fma(dx, force_divr, a.fx);
        a.fy = __builtin_fma(dy, force_divr, a.fy);
        a.fz = __builtin_fma(dz, force_divr, a.fz);
        a.pe += pair_eng;
        if (VIRIAL)
            {
            const double fxx = force_divr * dx, fyy = force_divr * dy;
            v[0] = __builtin_fma(fxx, dx, v[0]);
            v[1] = __builtin_fma(fxx, dy, v[1]);
            v[2] = __builtin_fma(fxx, dz, v[2]);
            v[3] = __builtin_fma(fyy, dy, v[3]);
            v[4] = __builtin_fma(fyy, dz, v[4]);
            v[5] = __builtin_fma(force_divr * dz, dz, v[5]);
            }
        }
    static int validate(const azp_pair_args* args, const Params* d_params) { return validate_pair_args(args, d_params); }
    static KExtra extra(const azp_pair_args&) { return KExtra(); }
    };

// TPP lanes per particle, each striding the row (entries sub, sub + TPP, ...) with the next index
// prefetched; coefficients in registers (one type) or LDS; the minimum image skipped by waves whose
// particles are all interior
template<class X, int TPP, bool VIRIAL, bool SINGLE>
__global__ void __launch_bounds__(256) pair_forces_kernel(const PairKArgs a, const typename X::KExtra x, const typename X::Params* __restrict__ params)
    {
    typedef typename X::Coeff Coeff;
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    Coeff* s_coeff = reinterpret_cast<Coeff*>(s_raw);
    Coeff c0;
    if (SINGLE)
        c0 = X::prepare(params, a, 0, x);
    else
        {
        const uint32_t ntp = a.ntypes * a.ntypes;
        for (uint32_t t = threadIdx.x; t < ntp; t += blockDim.x)
            s_coeff[t] = X::prepare(params, a, t, x);
        __syncthreads();
        }

    const uint32_t block = xcd_remap(blockIdx.x, a.nblocks_padded);
    const uint32_t idx = a.first + block * (blockDim.x / TPP) + threadIdx.x / TPP;
    const uint32_t sub = threadIdx.x % TPP;
    const bool active = idx < a.end;

    uint32_t n = 0;
    uint64_t head = 0;
    double3 pi = make_double3(0.0, 0.0, 0.0);
    int typei = 0;
    typename X::Own own = {};
    if (active)
        {
        n = a.n_neigh[idx];
        head = a.head_list[idx];
        const double4 p = load_scalar4(a.pos, idx);
        pi = make_double3(p.x, p.y, p.z);
        typei = type_from_w(p.w);
        X::load_own(x, idx, own);
        }
    typename X::Acc acc;
    X::zero(acc);
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};

    bool wrap = true;
    if (a.r_list_max > 0.0 && !a.box.triclinic)
        {
        const bool interior = !active || is_interior(a.box, pi.x, pi.y, pi.z, a.r_list_max);
        wrap = !__all(interior);
        }
    auto walk = [&](auto wrap_tag)
        {
        constexpr bool WRAP = decltype(wrap_tag)::value;
        const uint32_t* __restrict__ row = a.nlist + head;
        uint32_t k = sub;
        uint32_t j = (k < n) ? row[k] : 0u;
        while (k < n)
            {
            const uint32_t kn = k + TPP;
            const uint32_t jn = (kn < n) ? row[kn] : 0u;
            double dx, dy, dz;
            int typej = 0;
            if (SINGLE)
                {
                const double3 pj = load_scalar3_of4(a.pos, j); // (one type: w is not read)
                dx = pi.x - pj.x; dy = pi.y - pj.y; dz = pi.z - pj.z;
                }
            else
                {
                const double4 pj = load_scalar4(a.pos, j);
                dx = pi.x - pj.x; dy = pi.y - pj.y; dz = pi.z - pj.z;
                typej = type_from_w(pj.w);
                }
            if (WRAP)
                min_image(a.box, dx, dy, dz);
            const double rsq = __builtin_fma(dz, dz, __builtin_fma(dy, dy, dx * dx));
            const Coeff c = SINGLE ? c0 : s_coeff[(uint32_t)typei * a.ntypes + (uint32_t)typej];
            if (X::in_range(c, rsq))
                {
                double ext[X::kExtra > 0 ? X::kExtra : 1]; // (XIso: none)
                uint32_t tagj = 0;
                X::load_extra(x, j, ext, tagj);
                X::template pair<VIRIAL>(c, x, own, dx, dy, dz, rsq, ext, tagj, acc, v);
                }
            k = kn;
            j = jn;
            }
        };
    if (wrap)
        walk(std::true_type());
    else
        walk(std::false_type());

    X::template reduce<TPP>(acc);
    if (VIRIAL)
        {
#pragma unroll
        for (int cidx = 0; cidx < 6; ++cidx)
            v[cidx] = group_sum<TPP>(v[cidx]);
        }
    if (active && sub == 0)
        {
        X::store(acc, a, x, idx);
        if (VIRIAL)
            {
#pragma unroll
            for (int cidx = 0; cidx < 6; ++cidx)
                a.virial[(uint64_t)cidx * a.virial_pitch + idx] = 0.5 * v[cidx];
            }
        }
    }

// ---------------------------------------------------------------------------
// host-side driver
// ---------------------------------------------------------------------------

inline uint32_t choose_tpp(const azp_pair_args& args)
    {
    uint32_t tpp = args.threads_per_particle;
    if (tpp == 0)
        {
        // mean row length decides: rows shorter than ~2*TPP waste lanes in the tail
        double mean = (args.size_nlist && args.N) ? (double)args.size_nlist / (double)args.N : 64.0;
        if (mean >= 96.0) tpp = 8;
        else if (mean >= 40.0) tpp = 4;
        else if (mean >= 16.0) tpp = 2;
        else tpp = 1;
        }
    return tpp;
    }

// Launches kern with lds bytes of dynamic LDS and records the launch shape in last_launch(): more than
// 160 KiB is refused, more than 64 KiB is opted in to first.
template<class... KArgs, class... Args>
int launch_dyn_lds(void (*kern)(KArgs...), uint32_t grid, uint32_t block_size, uint32_t tpp, size_t lds, hipStream_t stream,
                   const Args&... args)
    {
    if (lds > 160 * 1024)
        return AZP_ERROR_TOO_MANY_TYPES;
    if (lds > 64 * 1024)
        {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess)
            return (int)e;
        }
    LaunchInfo& li = last_launch();
    li.block_size = block_size; li.tpp = tpp; li.grid = grid; li.lds_bytes = (uint32_t)lds;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block_size), lds, stream, args...);
    return (int)hipGetLastError();
    }

// f(std::integral_constant<int, TPP>()) for the lanes-per-particle counts of the generic kernels
template<class F> int dispatch_tpp(uint32_t tpp, F&& f)
    {
    switch (tpp)
        {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    case 4: return f(std::integral_constant<int, 4>());
    case 8: return f(std::integral_constant<int, 8>());
    case 16: return f(std::integral_constant<int, 16>());
    case 32: return f(std::integral_constant<int, 32>());
    default: return AZP_ERROR_INVALID_ARGUMENT;
        }
    }

// grid of a generic launch: block_size / TPP particles per workgroup, padded to a multiple of 8 (xcd_remap)
inline uint32_t generic_grid(const PairKArgs& k, uint32_t block_size, uint32_t tpp)
    {
    const uint32_t groups_per_block = block_size / tpp;
    const uint32_t nblocks = (k.end - k.first + groups_per_block - 1) / groups_per_block;
    return (nblocks + 7u) & ~7u;
    }

inline PairKArgs make_pair_kargs(const azp_pair_args& args)
    {
    PairKArgs k;
    k.force = args.d_force;
    k.virial = args.d_virial;
    k.virial_pitch = args.virial_pitch;
    k.pos = args.d_pos;
    k.n_neigh = args.d_n_neigh;
    k.nlist = args.d_nlist;
    k.head_list = args.d_head_list;
    k.rcutsq = args.d_rcutsq;
    k.ronsq = args.d_ronsq;
    k.box = make_box_dev(args.box);
    k.r_list_max = args.r_list_max;
    k.N = args.N;
    k.ntypes = args.ntypes;
    k.shift_mode = args.shift_mode;
    k.nblocks_padded = 0;
    k.first = args.range_count ? args.range_first : 0u;
    k.end = args.range_count ? args.range_first + args.range_count : args.N;
    return k;
    }

template<class X, int TPP, bool VIRIAL, bool SINGLE>
int launch_generic_instance(const azp_pair_args& args, const typename X::KExtra& x, const typename X::Params* d_params, uint32_t block_size,
                            hipStream_t stream)
    {
    PairKArgs k = make_pair_kargs(args);
    k.nblocks_padded = generic_grid(k, block_size, TPP);
    const size_t lds = SINGLE ? 0 : sizeof(typename X::Coeff) * (size_t)args.ntypes * args.ntypes;
    return launch_dyn_lds(pair_forces_kernel<X, TPP, VIRIAL, SINGLE>, k.nblocks_padded, block_size, TPP, lds, stream, k, x, d_params);
    }

// the generic kernel (arguments validated by the caller)
template<class X>
int launch_generic(const azp_pair_args& args, const typename X::KExtra& x, const typename X::Params* d_params, hipStream_t s)
    {
    const uint32_t bs = args.block_size ? args.block_size : 256u;
    const bool single = (args.ntypes == 1);
    return dispatch_tpp(choose_tpp(args), [&](auto t)
        {
        constexpr int TPP = decltype(t)::value;
        if (args.compute_virial)
            return single ? launch_generic_instance<X, TPP, true, true>(args, x, d_params, bs, s)
                          : launch_generic_instance<X, TPP, true, false>(args, x, d_params, bs, s);
        return single ? launch_generic_instance<X, TPP, false, true>(args, x, d_params, bs, s)
                      : launch_generic_instance<X, TPP, false, false>(args, x, d_params, bs, s);
        });
    }

} // namespace azp
