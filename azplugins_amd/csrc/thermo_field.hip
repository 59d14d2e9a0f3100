// thermo_field.hip -- the sums behind compute.ThermodynamicField: per bin of a 1-, 2- or 3-D grid (the bins of
// velocity_field.hip: field_bin.hpp) the row of AZP_THERMO_FIELD_NSUMS + ntypes doubles
//   0 n   1 M = sum m   2-4 P = sum m v   5-10 K = sum m v_a v_b   11-16 W = sum virial   17 U = sum energy
//   18... count per type
// (include/azp.h states the semantics). This project's, DESIGN 4.32.
//
// velocity_field.hip keeps the bins of a tile in LDS and re-reads every particle once per tile; at 18 + ntypes values
// per bin that does not scale. Here the particles are grouped by bin first and every particle is read ONCE:
//   tf_keys        one lane per row: wrap, mask, bin (field_bin.hpp) -> key = (bin << 32) | tag; a row that is not
//                  counted gets the bin AZP_THERMO_FIELD_NO_BIN, which sorts last.
//   (the caller sorts the keys: they are unique, so any sort gives the one order -- by bin, then by tag)
//   tf_head_count / tf_head_scan / tf_head_write
//                  a position p of the sorted keys is a head if its bin differs from that of p - 1. The heads are
//                  counted per workgroup, the counts scanned (block_exclusive_scan of azp_device.hpp), and every
//                  position learns the index s of its segment (= non-empty bin): seg_of[p] = s, seg_start[s] = p of
//                  the head, seg_start[number of segments] = the number of counted rows. Only the non-empty bins are
//                  enumerated: O(N), whatever the number of bins.
//   tf_level<FIRST>  the segmented sum, one launch per level of the tree. At level 1 the items of segment s are its
//                  c_1 = n_s particles at the sorted positions a_1 + i, a_1 = seg_start[s]; at level l + 1 they are
//                  the c_{l+1} = ceil(c_l / 64) partial rows at the slots a_{l+1} + i, a_{l+1} = floor(a_l / 32).
//                  (Two segments with more than 64 items never share a slot: for c >= 65, floor((a + c) / 32) >=
//                  floor(a / 32) + ceil(c / 64), and the next such segment starts at a + c or later. A segment with
//                  at most 64 items needs no slot: its sum is finished. Level l has at most S_l = S_{l-1} / 32 + 2
//                  slots, S_0 = N.)
//                  A wave owns a window of 64 consecutive items and takes, one after the other, the runs that START
//                  in its window: item i of a segment starts a run if i % 64 == 0 (one run per window where the bins
//                  hold more than 64 particles, up to 64 where they hold one each). For a run the 64 lanes gather the
//                  items i ... i + 63 of the segment (level 1: through the sorted permutation; zeros past the end of
//                  the segment), form the 18 terms in registers and reduce each with group_sum<64>: the balanced
//                  pairwise sum ((x0 + x1) + (x2 + x3)) + ... A segment with c_l <= 64 is finished: its row goes to
//                  d_out. Otherwise the run's sums go to slot a_{l+1} + i / 64, which also records s.
// The host launches ceil(log64 N) levels (at least 1); a level finds nothing to do for the segments that are
// finished. Nothing is read back, nothing is atomic. The order of the additions in a bin is the 64-ary tree of its
// members in tag order and nothing else: not N, not the other bins, not the order of the rows.
//
// The per-type counts are popcounts of lane ballots at level 1 (exact integers), stored as doubles and added through the
// same tree at the later levels: integers below 2^53 add exactly in any order.
//
// Terms (no contraction, in the order written): p_a = m v_a; K_ab = p_a v_b; W_c = ((0 + w_c of force 0) + w_c of
// force 1) + ... over the arrays with a virial; U likewise over the .w of every array.
//
// Bytes per particle: keys 32 (pos) + 4 (tag) + 8 (key); sort: torch's radix sort of N 8-byte keys; heads 2 x 8 + 4;
// level 1: 8 (order) + 4 (segment) + 32 (vel) + 32 (pos row, for the type) + per force 32 + per virial 48, gathered
// through the sorted permutation (rows that are sorted in space gather whole cache lines).
#include <algorithm>

#include "azp_device.hpp"
#include "field_bin.hpp"

namespace azp
{
constexpr uint32_t TF_BLOCK = 256;
constexpr uint32_t TF_WAVES = TF_BLOCK / WAVE;
constexpr uint32_t TF_NS = AZP_THERMO_FIELD_NSUMS;
constexpr uint32_t TF_NONE = 0xffffffffu;
constexpr uint32_t TF_MAX_LEVELS = 6;                   // 64^6 > 2^32
constexpr uint64_t TF_MAX_BINS = 2147483647ull;         // 2^31 - 1, as the velocity field

struct TFShape
    {
    uint64_t n_bins;
    uint32_t width;                  // TF_NS + ntypes
    uint32_t n_levels;
    uint32_t n_blocks;               // workgroups of the head kernels
    uint32_t slots[TF_MAX_LEVELS];   // slots[l]: slots that level l + 1 writes (l + 1 < n_levels)
    uint64_t off_seg_of, off_seg_start, off_block, off_slot_seg, off_part[TF_MAX_LEVELS];
    uint64_t slot_seg_words;
    uint64_t bytes;
    };

static int tf_shape(const azp_thermo_field_args* a, TFShape& s)
    {
    if (!a)
        return AZP_ERROR_INVALID_ARGUMENT;
    uint64_t nb = 1;
    for (int d = 0; d < 3; ++d)
        {
        if (a->num_bins[d] == 0)
            continue;
        nb *= a->num_bins[d];
        if (nb > TF_MAX_BINS)
            return AZP_ERROR_TOO_MANY_BINS;
        if (!(a->upper[d] > a->lower[d]))
            return AZP_ERROR_INVALID_ARGUMENT;
        }
    if (a->coordinates != AZP_COORDINATES_CARTESIAN && a->coordinates != AZP_COORDINATES_CYLINDRICAL)
        return AZP_ERROR_INVALID_ARGUMENT;
    if (a->n_forces > AZP_THERMO_MAX_FORCES || a->phases > (AZP_THERMO_FIELD_HEADS | AZP_THERMO_FIELD_LEVELS))
        return AZP_ERROR_INVALID_ARGUMENT;
    for (uint32_t f = 0; f < a->n_forces; ++f)
        if (!a->d_force[f])
            return AZP_ERROR_INVALID_ARGUMENT;
    s.n_bins = nb;
    s.width = TF_NS + a->ntypes;
    s.n_levels = 1;
    for (uint64_t reach = 64; reach < a->N; reach *= 64)
        ++s.n_levels;
    s.n_blocks = (uint32_t)(((uint64_t)a->N + TF_BLOCK - 1) / TF_BLOCK);
    uint64_t off = 0;
    auto take = [&off](uint64_t bytes) { const uint64_t o = off; off += (bytes + 255) & ~255ull; return o; };
    s.off_seg_of = take(4ull * a->N);
    s.off_seg_start = take(4ull * (std::min<uint64_t>(a->N, nb) + 2));
    s.off_block = take(4ull * s.n_blocks);
    uint64_t items = a->N;
    s.slot_seg_words = 0;
    for (uint32_t l = 0; l + 1 < s.n_levels; ++l)
        {
        s.slots[l] = (uint32_t)(items / 32 + 2);
        s.slot_seg_words += s.slots[l];
        items = s.slots[l];
        }
    s.off_slot_seg = take(4ull * s.slot_seg_words);
    for (uint32_t l = 0; l + 1 < s.n_levels; ++l)
        s.off_part[l] = take(8ull * s.width * s.slots[l]);
    s.bytes = off;
    return AZP_SUCCESS;
    }

struct TFKeyArgs
    {
    const double* pos;
    const uint32_t* tag;
    const uint8_t* mask;
    int64_t* keys;
    BoxDev box;
    double lo[3], hi[3];
    uint32_t nb[3];          // 0: not binned
    uint32_t N;
    uint32_t ntypes;
    };

template<int COORDS> __global__ void __launch_bounds__(TF_BLOCK) tf_keys(const TFKeyArgs a)
    {
    const uint64_t i64 = (uint64_t)blockIdx.x * TF_BLOCK + threadIdx.x;
    if (i64 >= a.N)
        return;
    const uint32_t i = (uint32_t)i64;
    const double4 p = load_scalar4(a.pos, i);
    bool ok = type_in_mask(a.mask, a.ntypes, p.w);
    double x = p.x, y = p.y, z = p.z;
    wrap_into_box(a.box, x, y, z);
    double px = 0.0, py = 0.0;   // (the rotated momentum of the velocity field: not used here)
    uint64_t bin = 0;
    ok = ok && bin_particle<COORDS>(a, x, y, z, px, py, bin);
    if (!ok)
        bin = AZP_THERMO_FIELD_NO_BIN;
    a.keys[i] = (int64_t)((bin << 32) | (uint64_t)a.tag[i]);
    }

__device__ __forceinline__ uint32_t tf_bin_of(int64_t key) { return (uint32_t)((uint64_t)key >> 32); }

// 1 if sorted position p starts a segment; `counted`: p holds a row that is counted
__device__ __forceinline__ uint32_t tf_is_head(const int64_t* keys, uint32_t N, uint64_t p, bool& counted)
    {
    counted = false;
    if (p >= N)
        return 0;
    const uint32_t b = tf_bin_of(keys[p]);
    counted = b != AZP_THERMO_FIELD_NO_BIN;
    return (counted && (p == 0 || tf_bin_of(keys[p - 1]) != b)) ? 1u : 0u;
    }

__global__ void __launch_bounds__(TF_BLOCK) tf_head_count(const int64_t* keys, uint32_t N, uint32_t* block_count)
    {
    __shared__ uint32_t s_wave[TF_WAVES];
    bool counted;
    const uint32_t flag = tf_is_head(keys, N, (uint64_t)blockIdx.x * TF_BLOCK + threadIdx.x, counted);
    uint32_t total;
    block_exclusive_scan<TF_WAVES>(flag, s_wave, total);
    if (threadIdx.x == 0)
        block_count[blockIdx.x] = total;
    }

// one workgroup: block_count becomes its exclusive prefix sum, in place
__global__ void __launch_bounds__(TF_BLOCK) tf_head_scan(uint32_t* block_count, uint32_t n_blocks)
    {
    __shared__ uint32_t s_wave[TF_WAVES];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_blocks; base += TF_BLOCK)
        {
        const uint32_t e = base + threadIdx.x;
        const uint32_t v = e < n_blocks ? block_count[e] : 0u;
        uint32_t total;
        const uint32_t before = block_exclusive_scan<TF_WAVES>(v, s_wave, total);
        if (e < n_blocks)
            block_count[e] = carry + before;
        carry += total;
        __syncthreads();   // (s_wave is written again in the next trip)
        }
    }

__global__ void __launch_bounds__(TF_BLOCK) tf_head_write(const int64_t* keys, uint32_t N, const uint32_t* block_offset,
                                                          uint32_t max_segments, uint32_t* seg_of, uint32_t* seg_start)
    {
    __shared__ uint32_t s_wave[TF_WAVES];
    const uint64_t p = (uint64_t)blockIdx.x * TF_BLOCK + threadIdx.x;
    bool counted;
    const uint32_t flag = tf_is_head(keys, N, p, counted);
    uint32_t total;
    const uint32_t s = block_offset[blockIdx.x] + block_exclusive_scan<TF_WAVES>(flag, s_wave, total) + flag;   // heads at or before p
    if (p >= N)
        return;
    // (s - 1 < max_segments = min(N, bins) for every counted row: the guard keeps a wrong key out of bounds of nothing)
    const bool ok = counted && s >= 1 && s <= max_segments;
    seg_of[p] = ok ? s - 1 : TF_NONE;
    if (ok && flag)
        seg_start[s - 1] = (uint32_t)p;
    if (ok && (p + 1 == N || tf_bin_of(keys[p + 1]) == AZP_THERMO_FIELD_NO_BIN))
        seg_start[s] = (uint32_t)p + 1;   // the end of the last segment
    }

struct TFLevelArgs
    {
    const int64_t* keys;      // sorted
    const int64_t* order;
    const uint32_t* seg_of;
    const uint32_t* seg_start;
    const double* vel;
    const double* pos;
    const double* force[AZP_THERMO_MAX_FORCES];
    const double* virial[AZP_THERMO_MAX_FORCES];
    const uint32_t* slot_seg_in;   // levels above 1: the segment of every item (TF_NONE: no item)
    const double* part_in;         // and the items, width columns of pitch n_items
    uint32_t* slot_seg_out;        // NULL at the last level
    double* part_out;
    double* out;
    uint64_t n_bins;
    uint32_t N;
    uint32_t ntypes;
    uint32_t n_forces;
    uint32_t level;                // 1 ...
    uint32_t n_items;              // N at level 1, else the slots of the level before
    uint32_t n_slots_out;
    };

#pragma clang fp contract(off)
template<bool FIRST> __global__ void __launch_bounds__(TF_BLOCK) tf_level(const TFLevelArgs a)
    {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint64_t base = ((uint64_t)blockIdx.x * TF_WAVES + threadIdx.x / WAVE) * WAVE;
    if (base >= a.n_items)
        return;   // (the whole wave)
    const uint64_t idx = base + lane;
    uint32_t s = TF_NONE;
    if (idx < a.n_items)
        s = FIRST ? a.seg_of[idx] : a.slot_seg_in[idx];
    // the items of segment s at this level: a_l ... a_l + c_l - 1
    uint32_t first = 0, count = 0, head = 0;
    if (s != TF_NONE)
        {
        head = a.seg_start[s];
        first = head;
        count = a.seg_start[s + 1] - head;
        for (uint32_t l = 1; l < a.level; ++l)
            {
            first /= 32;
            count = (count + 63) / 64;
            }
        }
    uint64_t runs = __ballot(s != TF_NONE && (((uint32_t)idx - first) & 63u) == 0);
    const uint32_t width = TF_NS + a.ntypes;
    while (runs)
        {
        const int r = __ffsll((unsigned long long)runs) - 1;
        runs &= runs - 1;
        const uint32_t s0 = (uint32_t)__shfl((int)s, r, WAVE);
        const uint32_t first0 = (uint32_t)__shfl((int)first, r, WAVE);
        const uint32_t count0 = (uint32_t)__shfl((int)count, r, WAVE);
        const uint32_t head0 = (uint32_t)__shfl((int)head, r, WAVE);
        const uint32_t i0 = (uint32_t)(base + r) - first0;          // the run's first item, counted in the segment
        const bool active = lane < count0 - i0;
        const uint64_t q = base + r + lane;                         // (< n_items where active)
        double t[TF_NS];
#pragma unroll
        for (uint32_t k = 0; k < TF_NS; ++k)
            t[k] = 0.0;
        uint32_t type = TF_NONE;
        if (active)
            {
            if (FIRST)
                {
                const uint32_t i = (uint32_t)a.order[q];
                const double4 v = load_scalar4(a.vel, i);
                type = (uint32_t)type_from_w(a.pos[4ull * i + 3]);
                const double m = v.w;
                const double px = m * v.x, py = m * v.y, pz = m * v.z;
                t[0] = 1.0; t[1] = m;
                t[2] = px; t[3] = py; t[4] = pz;
                t[5] = px * v.x; t[6] = px * v.y; t[7] = px * v.z;
                t[8] = py * v.y; t[9] = py * v.z; t[10] = pz * v.z;
                for (uint32_t f = 0; f < a.n_forces; ++f)
                    {
                    t[17] += a.force[f][4ull * i + 3];
                    const double* vir = a.virial[f];
                    if (vir)
                        {
#pragma unroll
                        for (uint32_t c = 0; c < 6; ++c)
                            t[11 + c] += vir[(uint64_t)c * a.N + i];
                        }
                    }
                }
            else
                {
#pragma unroll
                for (uint32_t k = 0; k < TF_NS; ++k)
                    t[k] = a.part_in[(uint64_t)k * a.n_items + q];
                }
            }
        // where the run's sums go: the row of the bin if the segment is finished, else slot a_{l+1} + i0 / 64
        const bool finished = count0 <= 64u;
        const uint64_t bin = tf_bin_of(a.keys[head0]);
        const uint64_t slot = (uint64_t)(first0 / 32) + i0 / 64;
        const bool in_bounds = finished ? bin < a.n_bins : (a.part_out != nullptr && slot < a.n_slots_out);
        double* dst = finished ? a.out + bin * width : a.part_out + slot;
        const uint64_t stride = finished ? 1 : a.n_slots_out;
        double mine = 0.0;
#pragma unroll
        for (uint32_t k = 0; k < TF_NS; ++k)
            {
            const double sum = group_sum<WAVE>(t[k]);
            mine = (lane == k) ? sum : mine;
            }
        if (in_bounds && lane < TF_NS)
            dst[lane * stride] = mine;
        for (uint32_t ty = 0; ty < a.ntypes; ++ty)
            {
            double c;
            if (FIRST)
                c = (double)__popcll((unsigned long long)__ballot(active && type == ty));
            else
                c = group_sum<WAVE>(active ? a.part_in[(uint64_t)(TF_NS + ty) * a.n_items + q] : 0.0);
            if (in_bounds && lane == 0)
                dst[(TF_NS + ty) * stride] = c;
            }
        if (!finished && in_bounds && lane == 0)
            a.slot_seg_out[slot] = s0;
        }
    }
#pragma clang fp contract(on)

static int tf_check_sums(const azp_thermo_field_args* a, TFShape& s)
    {
    const int rc = tf_shape(a, s);
    if (rc != AZP_SUCCESS)
        return rc;
    if (!a->d_out)
        return AZP_ERROR_INVALID_ARGUMENT;
    if (a->N == 0)
        return AZP_SUCCESS;
    if (!a->d_pos || !a->d_vel || !a->d_sorted_keys || !a->d_order || !a->d_scratch || a->scratch_bytes < s.bytes)
        return AZP_ERROR_INVALID_ARGUMENT;
    return AZP_SUCCESS;
    }

} // namespace azp

extern "C" int azp_thermo_field_scratch_size(const azp_thermo_field_args* args, uint64_t* bytes)
    {
    using namespace azp;
    if (!bytes)
        return AZP_ERROR_INVALID_ARGUMENT;
    TFShape s;
    const int rc = tf_shape(args, s);
    if (rc != AZP_SUCCESS)
        return rc;
    *bytes = s.bytes;
    return AZP_SUCCESS;
    }

extern "C" int azp_thermo_field_keys(const azp_thermo_field_args* args, void* stream)
    {
    using namespace azp;
    TFShape s;
    const int rc = tf_shape(args, s);
    if (rc != AZP_SUCCESS)
        return rc;
    if (args->N == 0)
        return AZP_SUCCESS;
    if (!args->d_pos || !args->d_tag || !args->d_keys)
        return AZP_ERROR_INVALID_ARGUMENT;
    TFKeyArgs k;
    k.pos = args->d_pos;
    k.tag = args->d_tag;
    k.mask = args->d_type_mask;
    k.keys = args->d_keys;
    k.box = make_box_dev(args->box);
    for (int d = 0; d < 3; ++d)
        {
        k.lo[d] = args->lower[d];
        k.hi[d] = args->upper[d];
        k.nb[d] = args->num_bins[d];
        }
    k.N = args->N;
    k.ntypes = args->ntypes;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (args->coordinates == AZP_COORDINATES_CARTESIAN)
        hipLaunchKernelGGL(tf_keys<AZP_COORDINATES_CARTESIAN>, dim3(s.n_blocks), dim3(TF_BLOCK), 0, st, k);
    else
        hipLaunchKernelGGL(tf_keys<AZP_COORDINATES_CYLINDRICAL>, dim3(s.n_blocks), dim3(TF_BLOCK), 0, st, k);
    return (int)hipGetLastError();
    }

extern "C" int azp_thermo_field_sums(const azp_thermo_field_args* args, void* stream)
    {
    using namespace azp;
    TFShape s;
    const int rc = tf_check_sums(args, s);
    if (rc != AZP_SUCCESS)
        return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // (phases: the probe times the heads and the tree apart; every other caller passes 0 = both)
    const bool heads = args->phases == 0 || (args->phases & AZP_THERMO_FIELD_HEADS);
    const bool levels = args->phases == 0 || (args->phases & AZP_THERMO_FIELD_LEVELS);
    hipError_t e = hipSuccess;
    // (the empty bins: every bin is written once here, the non-empty ones once more by the level that finishes them)
    if (levels)
        e = hipMemsetAsync(args->d_out, 0, s.n_bins * s.width * sizeof(double), st);
    if (e != hipSuccess || args->N == 0)
        return (int)e;
    char* scratch = static_cast<char*>(args->d_scratch);
    uint32_t* seg_of = reinterpret_cast<uint32_t*>(scratch + s.off_seg_of);
    uint32_t* seg_start = reinterpret_cast<uint32_t*>(scratch + s.off_seg_start);
    uint32_t* block = reinterpret_cast<uint32_t*>(scratch + s.off_block);
    uint32_t* slot_seg = reinterpret_cast<uint32_t*>(scratch + s.off_slot_seg);
    const uint32_t max_segments = (uint32_t)std::min<uint64_t>(args->N, s.n_bins);

    if (heads)
        {
        hipLaunchKernelGGL(tf_head_count, dim3(s.n_blocks), dim3(TF_BLOCK), 0, st, args->d_sorted_keys, args->N, block);
        hipLaunchKernelGGL(tf_head_scan, dim3(1), dim3(TF_BLOCK), 0, st, block, s.n_blocks);
        hipLaunchKernelGGL(tf_head_write, dim3(s.n_blocks), dim3(TF_BLOCK), 0, st, args->d_sorted_keys, args->N, block,
                           max_segments, seg_of, seg_start);
        e = hipGetLastError();
        if (e != hipSuccess)
            return (int)e;
        }
    if (!levels)
        return AZP_SUCCESS;
    if (s.slot_seg_words)
        {
        e = hipMemsetAsync(slot_seg, 0xff, 4ull * s.slot_seg_words, st);   // TF_NONE: a slot without an item
        if (e != hipSuccess)
            return (int)e;
        }

    TFLevelArgs k;
    k.keys = args->d_sorted_keys;
    k.order = args->d_order;
    k.seg_of = seg_of;
    k.seg_start = seg_start;
    k.vel = args->d_vel;
    k.pos = args->d_pos;
    for (uint32_t f = 0; f < AZP_THERMO_MAX_FORCES; ++f)
        {
        k.force[f] = f < args->n_forces ? args->d_force[f] : nullptr;
        k.virial[f] = f < args->n_forces ? args->d_virial[f] : nullptr;
        }
    k.out = args->d_out;
    k.n_bins = s.n_bins;
    k.N = args->N;
    k.ntypes = args->ntypes;
    k.n_forces = args->n_forces;
    k.slot_seg_in = nullptr;
    k.part_in = nullptr;
    k.n_items = args->N;
    uint32_t* slot_seg_level = slot_seg;
    for (uint32_t l = 0; l < s.n_levels; ++l)
        {
        const bool last = l + 1 == s.n_levels;
        k.level = l + 1;
        k.slot_seg_out = last ? nullptr : slot_seg_level;
        k.part_out = last ? nullptr : reinterpret_cast<double*>(scratch + s.off_part[l]);
        k.n_slots_out = last ? 0 : s.slots[l];
        const dim3 grid((uint32_t)(((uint64_t)k.n_items + TF_BLOCK - 1) / TF_BLOCK));
        if (l == 0)
            hipLaunchKernelGGL(tf_level<true>, grid, dim3(TF_BLOCK), 0, st, k);
        else
            hipLaunchKernelGGL(tf_level<false>, grid, dim3(TF_BLOCK), 0, st, k);
        e = hipGetLastError();
        if (e != hipSuccess)
            return (int)e;
        k.slot_seg_in = k.slot_seg_out;
        k.part_in = k.part_out;
        k.n_items = k.n_slots_out;
        if (!last)
            slot_seg_level += s.slots[l];
        }
    return AZP_SUCCESS;
    }
