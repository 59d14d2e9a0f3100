// cluster_properties.hip -- centres and gyration tensors per cluster behind compute.ClusterProperties (include/azp.h
// "cluster properties"): a segmented sum over the labels that azp_cluster_compute left per row, kept as
// integers in units of 2^-shift, so that the row of a key does not depend on the order in which anything arrives.
//
// The launches of one call, all on the caller's stream (nothing is read back; no lane waits for another workgroup):
//   count     per workgroup of 1024 rows, the number of representatives that get a table row:
//             rep[i] == i && size[i] >= min_size.
//   offsets   one workgroup: the exclusive scan of those counts (block_exclusive_scan in trips), the total into the head.
//   ids       per workgroup the scan of its own flags on top of its offset: id[i] = the dense index of representative
//             i, row_of[id] = i. (Three launches and no look-back chain: this file family's rule.)
//   zero      the accumulators of the dense indices below the total (the host does not know the total).
//   circular  per row of an eligible cluster: C_k, S_k of sincospi(2 s_k) on the periodic axes.
//   s0        per cluster: the reference point from the integer sums.
//   moments   per row: ds = s - s0 unwrapped, M1 (3), M2 (6), and per axis max(BIAS + ds) and max(BIAS - ds), BIAS = 1
//             (two maxima over positive integers: a zeroed word is "nothing yet", which a minimum could not start from).
//   finalize  per cluster: the table row; the largest cluster as one 64-bit atomicMax of size << 32 | ~key and the
//             number of particles in the table into the head.
//   summary   the table row whose (size, key) is that maximum is copied into the summary; words [0..3].
//
// The hot part is circular and moments: up to 6 + 15 integer atomics per row go to the words of its cluster.
//   size == 1            the row is alone: plain stores.
//   size < CP_DIRECT     one atomic per word and lane (a wave holds fewer than CP_DIRECT lanes of such a cluster). Never
//                        taken at the default CP_DIRECT = 2; it is what the probe's candidates 4 and 8 are built from.
//   otherwise            the leader loop of cl_flatten_kernel: the lanes that share the leader's cluster are counted by a
//                        ballot; CP_DIRECT or more of them add up through the wave butterfly, fewer send their own
//                        atomics. A turn of the loop that does not reduce costs a readlane and a ballot, and at most
//                        64 / CP_DIRECT turns of a wave reduce: the cost of a wave is bounded whatever the input, and no
//                        word receives more than CP_DIRECT - 1 direct atomics of one wave.
//   the carry            a wave takes CP_TRIPS chunks of 64 rows in turn and keeps the sums of the last cluster it
//                        reduced in registers; they are sent when another cluster is reduced or the wave ends.
// One cluster of all N: 21 atomics per wave, N / (64 CP_TRIPS) waves. N singletons: no atomic at all. Both constants are
// measured at N = 2^20 (profiles/cluster_properties.md; a candidate is a library of its own, hence compile-time):
// CP_DIRECT = 2, any two lanes that share a cluster combine (the liquid: 0.79 ms against 0.91 at 4 and 0.99 at 8: 64-bit
// atomics cost more than the butterfly); CP_TRIPS = 8 (one cluster of everything: 2.91 ms at 1, 0.45 at 8, 0.31 at 16, while
// the liquid stays at 0.79 up to 8 and takes 1.00 at 16, where the grid is down to one workgroup per CU).
#include <cmath>

#include "pair_walk.hpp"

#ifndef AZP_CP_DIRECT
#define AZP_CP_DIRECT 2
#endif
#ifndef AZP_CP_TRIPS
#define AZP_CP_TRIPS 8
#endif

namespace azp
{
constexpr uint32_t CP_BLOCK = 256;
constexpr uint32_t CP_SCAN_BLOCK = 1024;
constexpr uint32_t CP_HEAD_BYTES = 256;
constexpr uint32_t CP_DIRECT = AZP_CP_DIRECT;
constexpr uint32_t CP_TRIPS = AZP_CP_TRIPS;  // chunks of CP_BLOCK rows per workgroup of the two segmented-sum kernels
static_assert(CP_DIRECT >= 2 && CP_DIRECT <= 64, "a cluster of one takes the plain stores");
// the words of a cluster's accumulator row
constexpr uint32_t CP_CIRC = 0;      // C_x, S_x, C_y, S_y, C_z, S_z
constexpr uint32_t CP_M1 = 6;        // 3
constexpr uint32_t CP_M2 = 9;        // xx, xy, xz, yy, yz, zz
constexpr uint32_t CP_HI = 15;       // max (BIAS + ds) per axis
constexpr uint32_t CP_LO = 18;       // max (BIAS - ds) per axis
constexpr uint32_t CP_S0 = 21;       // 3 doubles
constexpr uint32_t CP_WORDS = 24;

struct CpHead
    {
    unsigned long long best;       // size << 32 | ~key of the largest cluster in the table
    unsigned long long particles;  // in the table's rows
    uint32_t rows;
    };

struct CpKArgs
    {
    const double* pos;
    const uint32_t* rep;
    const uint32_t* key;
    const uint32_t* size;
    uint32_t N, min_size, max_rows, n_blocks;
    int shift;
    double to_fixed, from_fixed;  // 2^shift, 2^-shift
    FracDev frac;
    double L[3], tilt[3];
    int periodic[3];
    CpHead* head;
    uint32_t* id;        // N: the dense index of a representative
    uint32_t* row_of;    // max_rows: dense index -> row
    uint32_t* block_sum; // n_blocks
    uint32_t* block_off; // n_blocks
    long long* acc;      // max_rows x CP_WORDS
    double* table;
    double* summary;
    };

__device__ __forceinline__ bool cp_flag(const CpKArgs& a, uint32_t i)
    {
    return i < a.N && a.rep[i] == i && a.size[i] >= a.min_size;
    }

__global__ void __launch_bounds__(CP_SCAN_BLOCK) cp_count_kernel(const CpKArgs a)
    {
    const int n = __syncthreads_count(cp_flag(a, blockIdx.x * CP_SCAN_BLOCK + threadIdx.x));
    if (threadIdx.x == 0)
        a.block_sum[blockIdx.x] = (uint32_t)n;
    }

__global__ void __launch_bounds__(CP_SCAN_BLOCK) cp_offsets_kernel(const CpKArgs a)
    {
    __shared__ uint32_t s_wave[CP_SCAN_BLOCK / WAVE];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < a.n_blocks; base += CP_SCAN_BLOCK)
        {
        const uint32_t b = base + threadIdx.x;
        const uint32_t v = b < a.n_blocks ? a.block_sum[b] : 0u;
        uint32_t total;
        const uint32_t excl = block_exclusive_scan<CP_SCAN_BLOCK / WAVE>(v, s_wave, total);
        if (b < a.n_blocks)
            a.block_off[b] = carry + excl;
        carry += total;
        __syncthreads();  // (s_wave is written again in the next trip)
        }
    if (threadIdx.x == 0)  // (carry <= max_rows for the outputs of one azp_cluster_compute call; nothing is indexed past the table)
        a.head->rows = min(carry, a.max_rows);
    }

__global__ void __launch_bounds__(CP_SCAN_BLOCK) cp_ids_kernel(const CpKArgs a)
    {
    __shared__ uint32_t s_wave[CP_SCAN_BLOCK / WAVE];
    const uint32_t i = blockIdx.x * CP_SCAN_BLOCK + threadIdx.x;
    const bool flag = cp_flag(a, i);
    uint32_t total;
    const uint32_t d = a.block_off[blockIdx.x] + block_exclusive_scan<CP_SCAN_BLOCK / WAVE>(flag ? 1u : 0u, s_wave, total);
    if (flag && d < a.max_rows)  // (d < floor(N / min_size): the flagged clusters are disjoint and hold min_size rows or more each)
        {
        a.id[i] = d;
        a.row_of[d] = i;
        }
    }

__global__ void __launch_bounds__(CP_BLOCK) cp_zero_kernel(const CpKArgs a)
    {
    const uint64_t w = (uint64_t)blockIdx.x * CP_BLOCK + threadIdx.x;
    if (w < (uint64_t)a.head->rows * CP_WORDS)
        a.acc[w] = 0;
    }

// ---------------------------------------------------------------------------------------------------------------
// the segmented sums
// ---------------------------------------------------------------------------------------------------------------
template<int CTRL> __device__ __forceinline__ long long cp_dpp(long long v)
    {
    int lo = (int)(uint32_t)(unsigned long long)v, hi = (int)(uint32_t)((unsigned long long)v >> 32);
    lo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xF, 0xF, false);
    hi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xF, 0xF, false);
    return (long long)(((unsigned long long)(uint32_t)hi << 32) | (unsigned long long)(uint32_t)lo);
    }

template<bool MAX> __device__ __forceinline__ long long cp_join(long long x, long long y) { return MAX ? (x > y ? x : y) : x + y; }

// the sum or the maximum over the 64 lanes, in every lane (the butterfly of group_sum, on integers)
template<bool MAX> __device__ __forceinline__ long long cp_wave(long long v)
    {
    v = cp_join<MAX>(v, cp_dpp<0xB1>(v));
    v = cp_join<MAX>(v, cp_dpp<0x4E>(v));
    v = cp_join<MAX>(v, cp_dpp<0x141>(v));
    v = cp_join<MAX>(v, cp_dpp<0x140>(v));
    v = cp_join<MAX>(v, __shfl_xor(v, 16, WAVE));
    v = cp_join<MAX>(v, __shfl_xor(v, 32, WAVE));
    return v;
    }

template<int NADD, int NMAX> __device__ __forceinline__ void cp_atomics(long long* dst, const long long (&v)[NADD + NMAX])
    {
#pragma unroll
    for (int k = 0; k < NADD; ++k)
        if (v[k])
            atomicAdd(reinterpret_cast<unsigned long long*>(dst + k), (unsigned long long)v[k]);
#pragma unroll
    for (int k = NADD; k < NADD + NMAX; ++k)
        __hip_atomic_fetch_max(dst + k, v[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }

// What a wave has added up for one cluster and not sent yet (wave-uniform): the rows of a wave's next trip mostly belong to
// the same cluster, whose sums then stay in registers. One cluster of all 2^20 particles sent 21 atomics per wave and
// trip, 344,064 on 21 words: 2.9 ms of serialised atomics (profiles/cluster_properties.md); carried over CP_TRIPS trips
// it is an eighth of that per word.
template<int NV> struct CpCarry
    {
    bool on;
    uint32_t d;
    long long v[NV];
    };

template<int NADD, int NMAX> __device__ __forceinline__ void cp_flush(long long* words, const CpCarry<NADD + NMAX>& c)
    {
    if (c.on && (threadIdx.x & 63u) == 0)
        cp_atomics<NADD, NMAX>(words + (uint64_t)c.d * CP_WORDS, c.v);
    }

// Every lane of the wave calls it. A lane with `in` adds v[0 .. NADD) to and takes the maximum of v[NADD ..) (all > 0)
// with the words `words + d * CP_WORDS` of its cluster, whose dense index is d and whose size is `size`.
template<int NADD, int NMAX>
__device__ __forceinline__ void cp_send(long long* words, bool in, uint32_t d, uint32_t size, const long long (&v)[NADD + NMAX],
                                        CpCarry<NADD + NMAX>& carry)
    {
    constexpr int NV = NADD + NMAX;
    long long* dst = words + (uint64_t)d * CP_WORDS;
    if (in && size == 1)
        {
#pragma unroll
        for (int k = 0; k < NV; ++k)
            dst[k] = v[k];
        }
    const bool big = in && size >= CP_DIRECT;
    bool direct = in && size > 1 && size < CP_DIRECT;  // (never at CP_DIRECT = 2: the candidates' branch, folded away here)
    unsigned long long todo = __ballot(big);
    while (todo)
        {
        const int leader = __builtin_ctzll(todo);
        const uint32_t d0 = (uint32_t)__builtin_amdgcn_readlane((int)d, leader);
        const bool mine = big && d == d0;
        const unsigned long long same = __ballot(mine);
        if ((uint32_t)__popcll(same) < CP_DIRECT)
            direct = direct || mine;
        else
            {
            long long sum[NV];
#pragma unroll
            for (int k = 0; k < NADD; ++k)
                sum[k] = cp_wave<false>(mine ? v[k] : 0ll);
#pragma unroll
            for (int k = NADD; k < NV; ++k)
                sum[k] = cp_wave<true>(mine ? v[k] : 0ll);
            if (carry.on && carry.d == d0)
                {
#pragma unroll
                for (int k = 0; k < NADD; ++k)
                    carry.v[k] += sum[k];
#pragma unroll
                for (int k = NADD; k < NV; ++k)
                    carry.v[k] = cp_join<true>(carry.v[k], sum[k]);
                }
            else
                {
                cp_flush<NADD, NMAX>(words, carry);
                carry.on = true;
                carry.d = d0;
#pragma unroll
                for (int k = 0; k < NV; ++k)
                    carry.v[k] = sum[k];
                }
            }
        todo &= ~same;
        }
    if (direct)
        cp_atomics<NADD, NMAX>(dst, v);
    }

struct CpRow
    {
    bool in;
    uint32_t d, size;
    double s[3];
    };

__device__ __forceinline__ CpRow cp_row(const CpKArgs& a, uint32_t i)
    {
    CpRow r;
    r.in = false;
    r.d = 0;
    r.size = 0;
    r.s[0] = r.s[1] = r.s[2] = 0.0;
    if (i < a.N)
        {
        const uint32_t rep = a.rep[i];
        r.size = a.size[i];
        if (rep != AZP_CLUSTER_NONE && rep < a.N && r.size >= a.min_size)
            {
            r.d = a.id[rep];
            r.in = r.d < a.max_rows;  // (always, for the outputs of one azp_cluster_compute call: nothing is written past the table)
            const double3 p = load_scalar3_of4(a.pos, i);
            const double3 f = fractional(a.frac, p.x, p.y, p.z);
            r.s[0] = f.x + 0.5;
            r.s[1] = f.y + 0.5;
            r.s[2] = f.z + 0.5;
            }
        }
    return r;
    }

__device__ __forceinline__ long long cp_fix(const CpKArgs& a, double x) { return __double2ll_rn(x * a.to_fixed); }

// the rows of trip `trip` of a workgroup of the two segmented-sum kernels: CP_TRIPS consecutive chunks of CP_BLOCK rows
__device__ __forceinline__ uint32_t cp_trip_row(uint32_t trip) { return (blockIdx.x * CP_TRIPS + trip) * CP_BLOCK + threadIdx.x; }

__global__ void __launch_bounds__(CP_BLOCK) cp_circular_kernel(const CpKArgs a)
    {
    CpCarry<6> carry;
    carry.on = false;
#pragma unroll 1
    for (uint32_t trip = 0; trip < CP_TRIPS && cp_trip_row(trip) - threadIdx.x < a.N; ++trip)
        {
        const CpRow r = cp_row(a, cp_trip_row(trip));
        long long v[6] = {0, 0, 0, 0, 0, 0};
        if (r.in)
            {
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if (a.periodic[k])
                    {
                    double sn, cs;
                    sincospi(2.0 * r.s[k], &sn, &cs);
                    v[2 * k] = cp_fix(a, cs);
                    v[2 * k + 1] = cp_fix(a, sn);
                    }
            }
        cp_send<6, 0>(a.acc + CP_CIRC, r.in, r.d, r.size, v, carry);
        }
    cp_flush<6, 0>(a.acc + CP_CIRC, carry);
    }

__global__ void __launch_bounds__(CP_BLOCK) cp_s0_kernel(const CpKArgs a)
    {
    const uint32_t d = blockIdx.x * CP_BLOCK + threadIdx.x;
    if (d >= a.head->rows)
        return;
    long long* row = a.acc + (uint64_t)d * CP_WORDS;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        {
        double s0 = 0.5;
        if (a.periodic[k])
            {
            const long long c = row[CP_CIRC + 2 * k], s = row[CP_CIRC + 2 * k + 1];
            s0 = 0.0;
            if (c != 0 || s != 0)
                {
                s0 = atan2((double)s, (double)c) * 0.15915494309189535;  // 1 / (2 pi)
                if (s0 < 0.0)
                    s0 += 1.0;
                if (!(s0 < 1.0))
                    s0 = 0.0;
                }
            }
        reinterpret_cast<double*>(row)[CP_S0 + k] = s0;
        }
    }

__global__ void __launch_bounds__(CP_BLOCK) cp_moments_kernel(const CpKArgs a)
    {
    CpCarry<15> carry;
    carry.on = false;
#pragma unroll 1
    for (uint32_t trip = 0; trip < CP_TRIPS && cp_trip_row(trip) - threadIdx.x < a.N; ++trip)
        {
        const CpRow r = cp_row(a, cp_trip_row(trip));
        long long v[15];
#pragma unroll
        for (int k = 0; k < 15; ++k)
            v[k] = 0;
        if (r.in)
            {
            const double* s0 = reinterpret_cast<const double*>(a.acc + (uint64_t)r.d * CP_WORDS) + CP_S0;
            const long long bias = 1ll << a.shift;
            double ds[3];
#pragma unroll
            for (int k = 0; k < 3; ++k)
                {
                ds[k] = r.s[k] - s0[k];
                if (a.periodic[k])
                    ds[k] -= rint(ds[k]);
                const long long f = cp_fix(a, ds[k]);
                v[k] = f;
                v[9 + k] = bias + f;
                v[12 + k] = bias - f;
                }
            v[3] = cp_fix(a, ds[0] * ds[0]);
            v[4] = cp_fix(a, ds[0] * ds[1]);
            v[5] = cp_fix(a, ds[0] * ds[2]);
            v[6] = cp_fix(a, ds[1] * ds[1]);
            v[7] = cp_fix(a, ds[1] * ds[2]);
            v[8] = cp_fix(a, ds[2] * ds[2]);
            }
        cp_send<9, 6>(a.acc + CP_M1, r.in, r.d, r.size, v, carry);
        }
    cp_flush<9, 6>(a.acc + CP_M1, carry);
    }

__global__ void __launch_bounds__(CP_BLOCK) cp_finalize_kernel(const CpKArgs a)
    {
    const uint32_t d = blockIdx.x * CP_BLOCK + threadIdx.x;
    const uint32_t i = d < a.head->rows ? a.row_of[d] : a.N;
    unsigned long long packed = 0, n_rows = 0;
    if (i < a.N)
        {
        const long long* row = a.acc + (uint64_t)d * CP_WORDS;
        const double* s0 = reinterpret_cast<const double*>(row) + CP_S0;
        const uint32_t size = a.size[i], key = a.key[i];
        const double n = (double)size;
        const long long bias2 = 2ll << a.shift, half = 1ll << (a.shift - 1);
        double m[3], c[3], ext[3];
        bool compact = true;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            {
            m[k] = (double)row[CP_M1 + k] * a.from_fixed / n;
            c[k] = s0[k] + m[k];
            if (a.periodic[k])
                {
                c[k] -= floor(c[k]);
                if (!(c[k] < 1.0))  // (a tiny negative c rounds to 1: the box is half-open, as in cp_s0_kernel)
                    c[k] = 0.0;
                }
            c[k] -= 0.5;
            const long long e = row[CP_HI + k] + row[CP_LO + k] - bias2;
            ext[k] = (double)e * a.from_fixed;
            if (a.periodic[k] && e >= half)
                compact = false;
            }
        // the covariance in fractional coordinates, then G = H cov H^T with H upper triangular
        double cov[3][3];
        const int word[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = 0; q < 3; ++q)
                // (one particle has no extent: exactly 0, not the rounding of M2 against m m^T)
                cov[p][q] = size == 1 ? 0.0 : (double)row[CP_M2 + word[p][q]] * a.from_fixed / n - m[p] * m[q];
        const double H[3][3] = {{a.L[0], a.tilt[0] * a.L[1], a.tilt[1] * a.L[2]}, {0.0, a.L[1], a.tilt[2] * a.L[2]}, {0.0, 0.0, a.L[2]}};
        double T[3][3], G[3][3];
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = 0; q < 3; ++q)
                T[p][q] = H[p][0] * cov[0][q] + H[p][1] * cov[1][q] + H[p][2] * cov[2][q];
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p; q < 3; ++q)
                G[p][q] = T[p][0] * H[q][0] + T[p][1] * H[q][1] + T[p][2] * H[q][2];
        double* out = a.table + (uint64_t)d * AZP_CLUSTER_PROPERTIES_ROW;
        out[0] = (double)key;
        out[1] = n;
        out[2] = H[0][0] * c[0] + H[0][1] * c[1] + H[0][2] * c[2];
        out[3] = H[1][1] * c[1] + H[1][2] * c[2];
        out[4] = H[2][2] * c[2];
        out[5] = G[0][0]; out[6] = G[0][1]; out[7] = G[0][2];
        out[8] = G[1][1]; out[9] = G[1][2]; out[10] = G[2][2];
        out[11] = G[0][0] + G[1][1] + G[2][2];
        out[12] = compact ? 1.0 : 0.0;
        out[13] = ext[0]; out[14] = ext[1]; out[15] = ext[2];
        packed = ((unsigned long long)size << 32) | (unsigned long long)(~key);
        n_rows = size;
        }
    // per wave one atomicMax and one atomicAdd
#pragma unroll
    for (int o = 32; o; o >>= 1)
        {
        const unsigned long long other = (unsigned long long)__shfl_xor((long long)packed, o, WAVE);
        packed = packed > other ? packed : other;
        n_rows += (unsigned long long)__shfl_xor((long long)n_rows, o, WAVE);
        }
    if ((threadIdx.x & 63u) == 0 && n_rows)
        {
        atomicMax(&a.head->best, packed);
        atomicAdd(&a.head->particles, n_rows);
        }
    }

// head == NULL: no particles at all
__global__ void __launch_bounds__(CP_BLOCK) cp_summary_kernel(const CpHead* head, const double* table, double* summary, int shift)
    {
    const uint32_t d = blockIdx.x * CP_BLOCK + threadIdx.x;
    const uint32_t rows = head ? head->rows : 0u;
    if (d == 0)
        {
        summary[0] = (double)rows;
        summary[1] = head ? (double)head->particles : 0.0;
        summary[2] = (double)shift;
        summary[3] = 0.0;
        if (rows == 0)
            {
            summary[4] = -1.0;
            for (int k = 5; k < AZP_CLUSTER_PROPERTIES_SUMMARY; ++k)
                summary[k] = 0.0;
            }
        }
    if (d >= rows)
        return;
    const double* row = table + (uint64_t)d * AZP_CLUSTER_PROPERTIES_ROW;
    const unsigned long long best = head->best;
    if (row[1] == (double)(uint32_t)(best >> 32) && row[0] == (double)(uint32_t)~(uint32_t)best)  // (keys are unique: one row)
        for (int k = 0; k < AZP_CLUSTER_PROPERTIES_ROW; ++k)
            summary[4 + k] = row[k];
    }

// ---------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------
struct CpPlan
    {
    int shift;
    uint32_t max_rows, n_blocks;
    uint64_t off_id, off_row_of, off_block_sum, off_block_off, off_acc, bytes;
    };

static int cp_plan(const azp_cluster_properties_args* a, CpPlan& p)
    {
    if (!a || a->min_size == 0 || a->N > AZP_CLUSTER_MAX_N)
        return AZP_ERROR_INVALID_ARGUMENT;
    for (int d = 0; d < 3; ++d)
        if (!(a->box.L[d] > 0.0))
            return AZP_ERROR_INVALID_ARGUMENT;
    int bits = 1;  // ceil(log2(max(N, 2)))
    while ((1ull << bits) < (uint64_t)a->N)
        ++bits;
    p.shift = std::min(52, 61 - bits);
    const uint64_t n = a->N;
    p.max_rows = a->N / a->min_size;
    p.n_blocks = (uint32_t)((n + CP_SCAN_BLOCK - 1) / CP_SCAN_BLOCK);
    p.off_id = CP_HEAD_BYTES;
    p.off_row_of = p.off_id + walk_align(n * 4);
    p.off_block_sum = p.off_row_of + walk_align((uint64_t)p.max_rows * 4);
    p.off_block_off = p.off_block_sum + walk_align((uint64_t)p.n_blocks * 4);
    p.off_acc = p.off_block_off + walk_align((uint64_t)p.n_blocks * 4);
    p.bytes = p.off_acc + walk_align((uint64_t)p.max_rows * CP_WORDS * 8);
    return AZP_SUCCESS;
    }

} // namespace azp

extern "C" int azp_cluster_properties_scratch_size(const azp_cluster_properties_args* args, uint64_t* bytes)
    {
    using namespace azp;
    if (!bytes)
        return AZP_ERROR_INVALID_ARGUMENT;
    CpPlan p;
    const int rc = cp_plan(args, p);
    if (rc != AZP_SUCCESS)
        return rc;
    *bytes = p.bytes;
    return AZP_SUCCESS;
    }

extern "C" int azp_cluster_properties(const azp_cluster_properties_args* args, void* stream)
    {
    using namespace azp;
    CpPlan p;
    const int rc = cp_plan(args, p);
    if (rc != AZP_SUCCESS)
        return rc;
    if (!args->d_summary)
        return AZP_ERROR_INVALID_ARGUMENT;
    if (args->N && (!args->d_pos || !args->d_cluster_rep || !args->d_cluster_key || !args->d_cluster_size || !args->d_scratch
                    || args->scratch_bytes < p.bytes || (p.max_rows && !args->d_table)))
        return AZP_ERROR_INVALID_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t e;
    if (p.max_rows == 0)  // (N == 0 or min_size > N: no cluster can have a row)
        {
        hipLaunchKernelGGL(cp_summary_kernel, dim3(1), dim3(CP_BLOCK), 0, st, (const CpHead*)nullptr, (const double*)nullptr,
                           args->d_summary, p.shift);
        return (int)hipGetLastError();
        }
    char* base = static_cast<char*>(args->d_scratch);
    if ((e = hipMemsetAsync(base, 0, CP_HEAD_BYTES, st)) != hipSuccess)
        return (int)e;
    CpKArgs k = {};
    k.pos = args->d_pos;
    k.rep = args->d_cluster_rep;
    k.key = args->d_cluster_key;
    k.size = args->d_cluster_size;
    k.N = args->N;
    k.min_size = args->min_size;
    k.max_rows = p.max_rows;
    k.n_blocks = p.n_blocks;
    k.shift = p.shift;
    k.to_fixed = std::ldexp(1.0, p.shift);
    k.from_fixed = std::ldexp(1.0, -p.shift);
    k.frac = make_frac_dev(args->box);
    for (int d = 0; d < 3; ++d)
        {
        k.L[d] = args->box.L[d];
        k.tilt[d] = args->box.tilt[d];
        k.periodic[d] = args->box.periodic[d];
        }
    k.head = reinterpret_cast<CpHead*>(base);
    k.id = walk_words(base, p.off_id);
    k.row_of = walk_words(base, p.off_row_of);
    k.block_sum = walk_words(base, p.off_block_sum);
    k.block_off = walk_words(base, p.off_block_off);
    k.acc = reinterpret_cast<long long*>(base + p.off_acc);
    k.table = args->d_table;
    k.summary = args->d_summary;
    const dim3 per_row((args->N + CP_BLOCK * CP_TRIPS - 1) / (CP_BLOCK * CP_TRIPS)), per_cluster((p.max_rows + CP_BLOCK - 1) / CP_BLOCK), block(CP_BLOCK);
    const dim3 per_word((uint32_t)(((uint64_t)p.max_rows * CP_WORDS + CP_BLOCK - 1) / CP_BLOCK));
    hipLaunchKernelGGL(cp_count_kernel, dim3(p.n_blocks), dim3(CP_SCAN_BLOCK), 0, st, k);
    if ((e = hipGetLastError()) != hipSuccess)
        return (int)e;
    hipLaunchKernelGGL(cp_offsets_kernel, dim3(1), dim3(CP_SCAN_BLOCK), 0, st, k);
    if ((e = hipGetLastError()) != hipSuccess)
        return (int)e;
    hipLaunchKernelGGL(cp_ids_kernel, dim3(p.n_blocks), dim3(CP_SCAN_BLOCK), 0, st, k);
    if ((e = hipGetLastError()) != hipSuccess)
        return (int)e;
    hipLaunchKernelGGL(cp_zero_kernel, per_word, block, 0, st, k);
    if ((e = hipGetLastError()) != hipSuccess)
        return (int)e;
    hipLaunchKernelGGL(cp_circular_kernel, per_row, block, 0, st, k);
    if ((e = hipGetLastError()) != hipSuccess)
        return (int)e;
    hipLaunchKernelGGL(cp_s0_kernel, per_cluster, block, 0, st, k);
    if ((e = hipGetLastError()) != hipSuccess)
        return (int)e;
    hipLaunchKernelGGL(cp_moments_kernel, per_row, block, 0, st, k);
    if ((e = hipGetLastError()) != hipSuccess)
        return (int)e;
    hipLaunchKernelGGL(cp_finalize_kernel, per_cluster, block, 0, st, k);
    if ((e = hipGetLastError()) != hipSuccess)
        return (int)e;
    hipLaunchKernelGGL(cp_summary_kernel, per_cluster, block, 0, st, (const CpHead*)k.head, (const double*)k.table, args->d_summary,
                       p.shift);
    return (int)hipGetLastError();
    }
