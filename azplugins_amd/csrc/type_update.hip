// type_update.hip -- particle types changed during a run (gfx950): the region type updater of the reference
// (src/TypeUpdater.cc:93-127) and its particle evaporator (src/ParticleEvaporator.cc:100-203), both HOOMD-2-era
// code that the reference's CMake no longer builds; restated for the HOOMD v5-style interface.
//
// Both read (z, type) of every row as one 16-byte load per lane and write the type word alone, as a 4-byte vector
// store: x, y, z and the upper half of w keep their bits.
//
// The evaporator picks the min(Nmax, M) of its M candidates that have the smallest 64-bit keys, key = (first word
// of Philox4x32-10 with the flow methods' key layout, id 203, counter {0, tag, 0, 0}) << 32 | tag. This replaces the
// reference's host-side shuffle of candidate indices (src/ParticleEvaporator.cc:229-259); see include/azp.h.
//   candidates : one pass over pos; the candidates of a wave are compacted with a ballot and a prefix popcount, ONE
//                integer atomic per wave reserves their slots in the key buffer
//   select     : most-significant-digit radix select of the K-th smallest key, 8 passes of 8-bit digits; every pass
//                histograms the digit of the keys still in the wanted bucket in LDS and folds it into global memory
//                with integer atomics; the next pass (every workgroup, redundantly) scans that histogram and narrows
//                the bucket. M lives on the device only: the grids are sized for N, and workgroups beyond M leave at once
//   apply      : one pass over pos; candidates whose key is <= the K-th smallest get the evaporated type
// Keys are unique (tags are), so the picked set does not depend on the order of the key buffer.
#include "azp_device.hpp"
#include "evaluators.hpp"

namespace azp
{
constexpr uint32_t RNG_EVAPORATOR = 203; // src/RNGIdentifiers.h
constexpr uint32_t SELECT_CHUNK = 4096;  // keys per workgroup and pass
constexpr uint32_t SORT_LDS_MAX = 4096;  // keys the single-workgroup sort holds in LDS (32 KiB)

enum { MODE_SELECT = 0, MODE_ALL = 1, MODE_NONE = 2 };
enum { THRESHOLD_DEVICE = 0, THRESHOLD_VALUE = 1, THRESHOLD_ALL = 2 };

struct SelState
    {
    uint64_t prefix; // the digits of the wanted key found so far
    uint32_t k;      // 1-based rank of the wanted key among the keys that share `prefix`
    uint32_t mode;
    };

struct EvapHeader
    {
    uint32_t M;     // candidates
    uint32_t n_out; // local_keys: keys collected
    uint32_t _pad[2];
    SelState state[9]; // state[p]: ahead of pass p; state[8].prefix: the K-th smallest key
    uint32_t hist[8][256];
    };
constexpr uint64_t HEADER_BYTES = (sizeof(EvapHeader) + 255) / 256 * 256;

struct EvapKArgs
    {
    double* pos;
    const uint32_t* tag;
    EvapHeader* hdr;
    uint64_t* keys;
    uint32_t* counts;
    double z_lo, z_hi;
    uint64_t threshold;
    uint32_t k0, k1; // Philox key
    uint32_t N;
    uint32_t solvent, evaporated;
    uint32_t nmax;
    };

// src/TypeUpdater.cc:107 / src/ParticleEvaporator.cc:190: a particle ON a face is inside
__device__ __forceinline__ bool in_slab(double z, double lo, double hi) { return !(z > hi || z < lo); }

__device__ __forceinline__ double2 load_zw(const double* pos, uint32_t idx)
    {
    return reinterpret_cast<const double2*>(pos)[2ull * idx + 1];
    }
__device__ __forceinline__ void store_type(double* pos, uint32_t idx, uint32_t type)
    {
    reinterpret_cast<uint32_t*>(pos)[8ull * idx + 6] = type; // low word of w
    }

__device__ __forceinline__ uint64_t evaporator_key(uint32_t k0, uint32_t k1, uint32_t tag)
    {
    uint32_t c0 = 0, c1 = tag, c2 = 0, c3 = 0;
    philox4x32_10(c0, c1, c2, c3, k0, k1);
    return ((uint64_t)c0 << 32) | (uint64_t)tag;
    }

__device__ __forceinline__ uint32_t lanes_below(uint64_t mask)
    {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
    }

// Slot of this lane among the `take` lanes of its wave in a buffer whose fill count is *cursor: one atomic per wave.
// Every lane of the wave calls it; lanes with take = false get no slot.
__device__ __forceinline__ uint32_t wave_reserve(uint32_t* cursor, bool take)
    {
    const uint64_t mask = __ballot(take);
    if (mask == 0)
        return 0;
    const int leader = __ffsll((unsigned long long)mask) - 1;
    uint32_t base = 0;
    if ((int)(threadIdx.x & 63u) == leader)
        base = atomicAdd(cursor, (uint32_t)__popcll(mask));
    base = __shfl(base, leader, WAVE);
    return base + lanes_below(mask);
    }

// src/TypeUpdater.cc:93-127
__global__ void __launch_bounds__(256)
type_update_region_kernel(double* pos, uint32_t N, uint32_t inside, uint32_t outside, double lo, double hi)
    {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N)
        return;
    const double2 zw = load_zw(pos, idx);
    const uint32_t type = (uint32_t)type_from_w(zw.y);
    if (type != inside && type != outside)
        return;
    const uint32_t now = in_slab(zw.x, lo, hi) ? inside : outside;
    if (now != type)
        store_type(pos, idx, now);
    }

// src/ParticleEvaporator.cc:176-203 (the marking pass) with the key of every candidate
__global__ void __launch_bounds__(256) evap_candidates_kernel(const EvapKArgs a)
    {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    bool cand = false;
    uint64_t key = 0;
    if (idx < a.N)
        {
        const double2 zw = load_zw(a.pos, idx);
        cand = (uint32_t)type_from_w(zw.y) == a.solvent && in_slab(zw.x, a.z_lo, a.z_hi);
        if (cand)
            key = evaporator_key(a.k0, a.k1, a.tag[idx]);
        }
    const uint32_t slot = wave_reserve(&a.hdr->M, cand);
    if (cand) // (M <= N: the slot is inside the N-entry key buffer)
        a.keys[slot] = key;
    }

// state[p] (p = 1..8) from state[p - 1] and the histogram of pass p - 1. All 256 threads of the workgroup call it.
__device__ SelState advance(const EvapHeader* h, int p, uint32_t* s_wave, SelState* s_state)
    {
    const SelState prev = h->state[p - 1];
    if (prev.mode != MODE_SELECT) // (uniform over the workgroup)
        return prev;
    const uint32_t tid = threadIdx.x;
    const uint32_t c = h->hist[p - 1][tid];
    uint32_t total;
    const uint32_t excl = block_exclusive_scan<4>(c, s_wave, total), incl = excl + c;
    // the digit whose bucket holds the k-th key: excl < k <= incl (exactly one digit: the counts sum to >= k)
    if (excl < prev.k && prev.k <= incl)
        {
        SelState next;
        next.prefix = prev.prefix | ((uint64_t)tid << (56 - 8 * (p - 1)));
        next.k = prev.k - excl;
        next.mode = MODE_SELECT;
        *s_state = next;
        }
    __syncthreads();
    return *s_state;
    }

// pass p (0..7) of the radix select; workgroup b takes keys [b, b + 1) * SELECT_CHUNK
__global__ void __launch_bounds__(256) evap_select_pass_kernel(EvapHeader* h, const uint64_t* keys, uint32_t nmax, int p)
    {
    __shared__ uint32_t s_hist[256];
    __shared__ uint32_t s_wave[4];
    __shared__ SelState s_state;
    const uint32_t M = h->M;
    const uint32_t first = blockIdx.x * SELECT_CHUNK;
    if (first >= M && blockIdx.x != 0)
        return;
    SelState st;
    if (p == 0)
        {
        // src/ParticleEvaporator.cc:110-116: fewer candidates than Nmax: all of them
        st.prefix = 0;
        st.k = nmax < M ? nmax : M;
        st.mode = st.k == 0 ? MODE_NONE : (st.k >= M ? MODE_ALL : MODE_SELECT);
        }
    else
        st = advance(h, p, s_wave, &s_state);
    if (blockIdx.x == 0 && threadIdx.x == 0)
        h->state[p] = st;
    if (st.mode != MODE_SELECT)
        return;
    s_hist[threadIdx.x] = 0;
    __syncthreads();
    const int shift = 56 - 8 * p;
    const uint64_t known = p == 0 ? 0ull : ~0ull << (64 - 8 * p);
    const uint32_t last = first + SELECT_CHUNK < M ? first + SELECT_CHUNK : M;
    for (uint32_t i = first + threadIdx.x; i < last; i += 256)
        {
        const uint64_t key = keys[i];
        if ((key & known) == st.prefix)
            atomicAdd(&s_hist[(uint32_t)(key >> shift) & 255u], 1u);
        }
    __syncthreads();
    const uint32_t c = s_hist[threadIdx.x];
    if (c)
        atomicAdd(&h->hist[p][threadIdx.x], c);
    }

// src/ParticleEvaporator.cc:205-227 (the type change of the picked particles). SRC: where the threshold comes from.
template<int SRC> __global__ void __launch_bounds__(256) evap_apply_kernel(const EvapKArgs a)
    {
    __shared__ uint32_t s_wave[4];
    __shared__ SelState s_state;
    uint32_t mode = SRC == THRESHOLD_ALL ? MODE_ALL : MODE_SELECT;
    uint64_t threshold = a.threshold;
    if (SRC == THRESHOLD_DEVICE)
        {
        const SelState st = advance(a.hdr, 8, s_wave, &s_state);
        mode = st.mode;
        threshold = st.prefix;
        if (a.counts && blockIdx.x == 0 && threadIdx.x == 0)
            {
            const uint32_t M = a.hdr->M;
            a.counts[0] = M;
            a.counts[1] = a.nmax < M ? a.nmax : M;
            }
        if (mode == MODE_NONE)
            return;
        }
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    bool cand = false, pick = false;
    if (idx < a.N)
        {
        const double2 zw = load_zw(a.pos, idx);
        cand = (uint32_t)type_from_w(zw.y) == a.solvent && in_slab(zw.x, a.z_lo, a.z_hi);
        if (cand)
            pick = mode == MODE_ALL || evaporator_key(a.k0, a.k1, a.tag[idx]) <= threshold;
        if (pick)
            store_type(a.pos, idx, a.evaporated);
        }
    if (SRC != THRESHOLD_DEVICE && a.counts)
        {
        // (one atomic per wave and counter; the caller zeroed the two words)
        const uint64_t mc = __ballot(cand), mp = __ballot(pick);
        if ((threadIdx.x & 63u) == 0)
            {
            if (mc)
                atomicAdd(&a.counts[0], (uint32_t)__popcll(mc));
            if (mp)
                atomicAdd(&a.counts[1], (uint32_t)__popcll(mp));
            }
        }
    }

// local_keys: the keys <= the K-th smallest, in any order, behind the sort buffer's cursor
__global__ void __launch_bounds__(256) evap_collect_kernel(EvapHeader* h, const uint64_t* keys, uint64_t* out, uint32_t capacity)
    {
    __shared__ uint32_t s_wave[4];
    __shared__ SelState s_state;
    const SelState st = advance(h, 8, s_wave, &s_state);
    if (st.mode == MODE_NONE)
        return;
    const uint32_t M = h->M;
    const uint32_t first = blockIdx.x * SELECT_CHUNK;
    const uint32_t last = first + SELECT_CHUNK < M ? first + SELECT_CHUNK : M;
    for (uint32_t i0 = first; i0 < last; i0 += 256) // (whole waves stay in the loop: wave_reserve is a wave operation)
        {
        const uint32_t i = i0 + threadIdx.x;
        uint64_t key = 0;
        bool take = false;
        if (i < last)
            {
            key = keys[i];
            take = st.mode == MODE_ALL || key <= st.prefix;
            }
        const uint32_t slot = wave_reserve(&h->n_out, take);
        if (take && slot < capacity)
            out[slot] = key;
        }
    }

__device__ __forceinline__ void compare_exchange(uint64_t* v, uint32_t t, uint32_t j, uint32_t k)
    {
    const uint32_t i = 2u * t - (t & (j - 1u)), l = i + j;
    const uint64_t x = v[i], y = v[l];
    if ((x > y) == ((i & k) == 0u))
        {
        v[i] = y;
        v[l] = x;
        }
    }

// ascending bitonic sort of P <= SORT_LDS_MAX keys (P a power of two) in one workgroup
__global__ void __launch_bounds__(1024) evap_sort_lds_kernel(uint64_t* keys, uint32_t P)
    {
    __shared__ uint64_t s[SORT_LDS_MAX];
    for (uint32_t i = threadIdx.x; i < P; i += 1024)
        s[i] = keys[i];
    __syncthreads();
    for (uint32_t k = 2; k <= P; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1)
            {
            for (uint32_t t = threadIdx.x; t < P / 2; t += 1024)
                compare_exchange(s, t, j, k);
            __syncthreads();
            }
    for (uint32_t i = threadIdx.x; i < P; i += 1024)
        keys[i] = s[i];
    }

// one step of the same network in global memory (P > SORT_LDS_MAX: a rank that offers thousands of keys per update)
__global__ void __launch_bounds__(256) evap_sort_step_kernel(uint64_t* keys, uint32_t P, uint32_t j, uint32_t k)
    {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < P / 2)
        compare_exchange(keys, t, j, k);
    }

__global__ void __launch_bounds__(256)
evap_emit_kernel(const EvapHeader* h, const uint64_t* sorted, uint32_t capacity, uint64_t* out, uint32_t* n_out, uint32_t* counts)
    {
    const uint32_t n = h->n_out < capacity ? h->n_out : capacity;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        out[i] = sorted[i];
    if (i == 0)
        {
        *n_out = n;
        if (counts)
            {
            counts[0] = h->M;
            counts[1] = 0;
            }
        }
    }

// (returns from the calling entry point with the runtime's error code)
#define AZP_TRY(call)                 \
    do                                \
        {                             \
        const hipError_t e_ = (call); \
        if (e_ != hipSuccess)         \
            return (int)e_;           \
        } while (0)

static uint32_t pow2_at_least(uint32_t n)
    {
    uint32_t p = 1;
    while (p < n && p < 0x80000000u)
        p <<= 1;
    return p;
    }

static uint64_t scratch_size(uint32_t N) { return HEADER_BYTES + 8ull * N + 8ull * pow2_at_least(N > 2 ? N : 2); }

static int check_args(const azp_evaporate_args* args, bool needs_scratch, uint32_t& bs)
    {
    if (!args->d_pos || !args->d_tag)
        return AZP_ERROR_INVALID_ARGUMENT;
    if (!(args->z_lo <= args->z_hi)) // (also rejects NaN)
        return AZP_ERROR_INVALID_ARGUMENT;
    if (needs_scratch && (!args->d_scratch || args->scratch_bytes < scratch_size(args->N)))
        return AZP_ERROR_INVALID_ARGUMENT;
    bs = args->block_size ? args->block_size : 256u;
    if (bs % 64 || bs > 256)
        return AZP_ERROR_INVALID_ARGUMENT;
    return AZP_SUCCESS;
    }

static EvapKArgs kernel_args(const azp_evaporate_args* args)
    {
    EvapKArgs k;
    k.pos = args->d_pos;
    k.tag = args->d_tag;
    k.hdr = static_cast<EvapHeader*>(args->d_scratch);
    k.keys = args->d_scratch ? reinterpret_cast<uint64_t*>(static_cast<char*>(args->d_scratch) + HEADER_BYTES) : nullptr;
    k.counts = args->d_counts;
    k.z_lo = args->z_lo;
    k.z_hi = args->z_hi;
    k.threshold = 0;
    k.k0 = philox_key0(RNG_EVAPORATOR, args->timestep, args->seed);
    k.k1 = (uint32_t)args->timestep;
    k.N = args->N;
    k.solvent = args->solvent_type;
    k.evaporated = args->evaporated_type;
    k.nmax = args->Nmax;
    return k;
    }

// candidates and the eight select passes: leaves the K-th smallest key one `advance` away (state[7], hist[7])
static int launch_select(const EvapKArgs& k, uint32_t bs, hipStream_t s)
    {
    AZP_TRY(hipMemsetAsync(k.hdr, 0, sizeof(EvapHeader), s));
    hipLaunchKernelGGL(evap_candidates_kernel, dim3((k.N + bs - 1) / bs), dim3(bs), 0, s, k);
    const uint32_t grid = (k.N + SELECT_CHUNK - 1) / SELECT_CHUNK;
    for (int p = 0; p < 8; ++p)
        hipLaunchKernelGGL(evap_select_pass_kernel, dim3(grid), dim3(256), 0, s, k.hdr, (const uint64_t*)k.keys, k.nmax, p);
    return (int)hipGetLastError();
    }
} // namespace azp

extern "C" int azp_type_update_region(const azp_type_update_args* args, void* stream)
    {
    using namespace azp;
    if (!args)
        return AZP_ERROR_INVALID_ARGUMENT;
    if (args->N == 0)
        return AZP_SUCCESS;
    if (!args->d_pos || !(args->z_lo <= args->z_hi))
        return AZP_ERROR_INVALID_ARGUMENT;
    const uint32_t bs = args->block_size ? args->block_size : 256u;
    if (bs % 64 || bs > 256)
        return AZP_ERROR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(type_update_region_kernel, dim3((args->N + bs - 1) / bs), dim3(bs), 0, static_cast<hipStream_t>(stream),
                       args->d_pos, args->N, args->inside_type, args->outside_type, args->z_lo, args->z_hi);
    return (int)hipGetLastError();
    }

extern "C" uint64_t azp_evaporate_scratch_size(uint32_t N) { return azp::scratch_size(N); }

extern "C" int azp_evaporate(const azp_evaporate_args* args, void* stream)
    {
    using namespace azp;
    if (!args)
        return AZP_ERROR_INVALID_ARGUMENT;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (args->N == 0)
        {
        if (args->d_counts)
            AZP_TRY(hipMemsetAsync(args->d_counts, 0, 8, s));
        return AZP_SUCCESS;
        }
    const bool unlimited = args->Nmax == 0xffffffffu;
    uint32_t bs;
    const int rc = check_args(args, !unlimited, bs);
    if (rc != AZP_SUCCESS)
        return rc;
    const EvapKArgs k = kernel_args(args);
    const uint32_t grid = (args->N + 255u) / 256u;
    if (unlimited)
        {
        // every candidate: nothing to select
        if (args->d_counts)
            AZP_TRY(hipMemsetAsync(args->d_counts, 0, 8, s));
        hipLaunchKernelGGL(evap_apply_kernel<THRESHOLD_ALL>, dim3(grid), dim3(256), 0, s, k);
        return (int)hipGetLastError();
        }
    const int rs = launch_select(k, bs, s);
    if (rs != AZP_SUCCESS)
        return rs;
    hipLaunchKernelGGL(evap_apply_kernel<THRESHOLD_DEVICE>, dim3(grid), dim3(256), 0, s, k);
    return (int)hipGetLastError();
    }

extern "C" int azp_evaporate_local_keys(const azp_evaporate_args* args, void* stream)
    {
    using namespace azp;
    if (!args || !args->d_n_keys_out)
        return AZP_ERROR_INVALID_ARGUMENT;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (args->N == 0 || args->Nmax == 0)
        {
        AZP_TRY(hipMemsetAsync(args->d_n_keys_out, 0, 4, s));
        if (args->d_counts)
            AZP_TRY(hipMemsetAsync(args->d_counts, 0, 8, s));
        return AZP_SUCCESS;
        }
    uint32_t bs;
    const int rc = check_args(args, true, bs);
    if (rc != AZP_SUCCESS)
        return rc;
    if (!args->d_keys_out)
        return AZP_ERROR_INVALID_ARGUMENT;
    const EvapKArgs k = kernel_args(args);
    const int rs = launch_select(k, bs, s);
    if (rs != AZP_SUCCESS)
        return rs;
    // at most min(Nmax, N) keys, sorted in a power-of-two buffer padded with the largest key
    const uint32_t capacity = args->Nmax < args->N ? args->Nmax : args->N;
    const uint32_t P = pow2_at_least(capacity > 2 ? capacity : 2);
    uint64_t* sortbuf = k.keys + args->N;
    AZP_TRY(hipMemsetAsync(sortbuf, 0xff, 8ull * P, s));
    hipLaunchKernelGGL(evap_collect_kernel, dim3((args->N + SELECT_CHUNK - 1) / SELECT_CHUNK), dim3(256), 0, s, k.hdr,
                       (const uint64_t*)k.keys, sortbuf, capacity);
    if (P <= SORT_LDS_MAX)
        hipLaunchKernelGGL(evap_sort_lds_kernel, dim3(1), dim3(1024), 0, s, sortbuf, P);
    else
        for (uint32_t kk = 2; kk != 0 && kk <= P; kk <<= 1)
            for (uint32_t j = kk >> 1; j > 0; j >>= 1)
                hipLaunchKernelGGL(evap_sort_step_kernel, dim3((P / 2 + 255u) / 256u), dim3(256), 0, s, sortbuf, P, j, kk);
    hipLaunchKernelGGL(evap_emit_kernel, dim3((capacity + 255u) / 256u), dim3(256), 0, s, (const EvapHeader*)k.hdr,
                       (const uint64_t*)sortbuf, capacity, args->d_keys_out, args->d_n_keys_out, args->d_counts);
    return (int)hipGetLastError();
    }

extern "C" int azp_evaporate_apply_below(const azp_evaporate_args* args, uint64_t threshold_key, void* stream)
    {
    using namespace azp;
    if (!args)
        return AZP_ERROR_INVALID_ARGUMENT;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (args->d_counts)
        AZP_TRY(hipMemsetAsync(args->d_counts, 0, 8, s));
    if (args->N == 0)
        return AZP_SUCCESS;
    uint32_t bs;
    const int rc = check_args(args, false, bs);
    if (rc != AZP_SUCCESS)
        return rc;
    EvapKArgs k = kernel_args(args);
    k.threshold = threshold_key;
    hipLaunchKernelGGL(evap_apply_kernel<THRESHOLD_VALUE>, dim3((args->N + bs - 1) / bs), dim3(bs), 0, s, k);
    return (int)hipGetLastError();
    }
