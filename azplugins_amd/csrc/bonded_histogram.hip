// bonded_histogram.hip -- the counts behind compute.BondedDistribution: one histogram per group type of the bond
// lengths (arity 2: bonds and special pairs), the bending angles (3) or the dihedral angles (4) of a state. Not part of
// the reference; the semantics are defined in include/azp.h ("distributions of the bonded coordinates") and DESIGN 4.26.
//
// One lane per local row walks the per-particle table of the kind, the one the force kernels walk, and counts the
// entries in which its row is member 0 of the group: every group is counted once, by the rank that owns its first
// member, with no bookkeeping of its own. The partner positions are the only gathers. No force parameters are read and
// no forces are touched.
//
// Accumulation is integer throughout, as in rdf.hip: a uint32 histogram of the workgroup in LDS, n_types rows laid out
// as the output row (counts[num_bins], outside, total), incremented with integer LDS atomics and added to the output
// row at the end with 64-bit integer atomicAdd on the non-zero words. The `total` word of a type is not counted (it
// would be one address for all lanes): a second launch of one workgroup per type sums it from the finished row.
// Integer sums do not depend on the order of the adds: two calls give the same bits. A workgroup takes up to BH_TILES_PER_BLOCK tiles of 256 rows; a lane whose row has more than
// BH_LANE_MAX entries counts straight into the output row, so a word of the LDS histogram receives at most
// 256 x 256 x 65535 < 2^32 increments before the one flush. Where the histogram does not fit into the 64 KiB of LDS a
// workgroup can have (more than AZP_BONDED_HISTOGRAM_LDS_WORDS words), every lane counts straight into the output
// row (BhSink<false>): the same integers, by 64-bit integer atomics alone.
//
// Occupancy: the LDS path is bounded by its histogram (160 KiB per CU: 64 KiB leaves two workgroups, the usual few
// hundred words leave the register limit alone); bytes per row: the count, 8 - 16 B per entry, 32 B per partner.
#include <algorithm>
#include <cmath>

#include "azp_device.hpp"
#include "pair_kernel_host.hpp"

namespace azp
{
constexpr uint32_t BH_BLOCK = 256;
constexpr uint32_t BH_TILES_PER_BLOCK = 256;
constexpr uint32_t BH_LANE_MAX = 65535;
constexpr uint32_t BH_TARGET_BLOCKS = 2048; // 256 CUs x 8

struct BhKArgs
    {
    const double* pos;
    const void* table;
    const uint32_t* table_pos;
    const uint32_t* counts;
    unsigned long long* out;
    uint64_t pitch;
    BoxDev box;
    double lo, hi, scale;
    uint32_t N, n_max, n_types, num_bins;
    uint32_t tiles_per_block;
    };

// where a count goes: the workgroup's LDS histogram (uint32) or the output row itself (uint64)
template<bool LDS> struct BhSink;
template<> struct BhSink<true>
    {
    uint32_t* hist;
    unsigned long long* out;
    __device__ __forceinline__ void add(uint32_t word, bool direct) const
        {
        if (direct)
            atomicAdd(&out[word], 1ull);
        else
            atomicAdd(&hist[word], 1u);
        }
    };
template<> struct BhSink<false>
    {
    uint32_t* hist;
    unsigned long long* out;
    __device__ __forceinline__ void add(uint32_t word, bool) const { atomicAdd(&out[word], 1ull); }
    };

// one group of type `type` with coordinate x: its bin, or `outside`. (`total` is summed from the finished row by
// bonded_histogram_totals: counted here it would be ONE address for every lane that counts a group of the type.)
template<bool LDS>
__device__ __forceinline__ void bh_count(const BhKArgs& a, const BhSink<LDS>& sink, uint32_t type, double x, bool direct)
    {
    if (type >= a.n_types)
        return;
    const uint32_t base = type * (a.num_bins + 2);
    uint32_t word = base + a.num_bins; // outside (a NaN fails the test too)
    if (x >= a.lo && x < a.hi)
        word = base + min((uint32_t)((x - a.lo) * a.scale), a.num_bins - 1);
    sink.add(word, direct);
    }

// The coordinate of one table entry, ARITY by ARITY; false where this row is not member 0 of the group or the entry
// names a row that does not exist.
template<int ARITY> struct BhGeometry;

template<> struct BhGeometry<2>
    {
    static __device__ __forceinline__ bool coordinate(const BhKArgs& a, const double3& p, uint64_t at, uint32_t& type, double& x)
        {
        if (a.table_pos[at] != 0)
            return false;
        const azp_bond_entry e = static_cast<const azp_bond_entry*>(a.table)[at];
        if (e.idx >= a.n_max)
            return false;
        const double3 q = load_scalar3_of4(a.pos, e.idx);
        double dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
        min_image(a.box, dx, dy, dz);
        type = e.type;
        x = sqrt(dx * dx + dy * dy + dz * dz); // (IEEE, correctly rounded)
        return true;
        }
    };

template<> struct BhGeometry<3>
    {
    static __device__ __forceinline__ bool coordinate(const BhKArgs& a, const double3& p, uint64_t at, uint32_t& type, double& x)
        {
        const uint4 w = static_cast<const uint4*>(a.table)[at]; // azp_angle_entry: b, c, type, position
        if (w.w != 0 || w.x >= a.n_max || w.y >= a.n_max)
            return false;
        const double3 rb = load_scalar3_of4(a.pos, w.x), rc = load_scalar3_of4(a.pos, w.y);
        double abx = p.x - rb.x, aby = p.y - rb.y, abz = p.z - rb.z;
        double cbx = rc.x - rb.x, cby = rc.y - rb.y, cbz = rc.z - rb.z;
        min_image(a.box, abx, aby, abz);
        min_image(a.box, cbx, cby, cbz);
        const double nx = aby * cbz - abz * cby, ny = abz * cbx - abx * cbz, nz = abx * cby - aby * cbx;
        type = w.z;
        x = atan2(sqrt(nx * nx + ny * ny + nz * nz), abx * cbx + aby * cby + abz * cbz);
        return true;
        }
    };

template<> struct BhGeometry<4>
    {
    static __device__ __forceinline__ bool coordinate(const BhKArgs& a, const double3& p, uint64_t at, uint32_t& type, double& x)
        {
        const uint4 w = static_cast<const uint4*>(a.table)[at]; // azp_dihedral_entry: b, c, d, type | position << 30
        if ((w.w >> 30) != 0 || w.x >= a.n_max || w.y >= a.n_max || w.z >= a.n_max)
            return false;
        const double3 rb = load_scalar3_of4(a.pos, w.x), rc = load_scalar3_of4(a.pos, w.y), rd = load_scalar3_of4(a.pos, w.z);
        double b1x = rb.x - p.x, b1y = rb.y - p.y, b1z = rb.z - p.z;
        double b2x = rc.x - rb.x, b2y = rc.y - rb.y, b2z = rc.z - rb.z;
        double b3x = rd.x - rc.x, b3y = rd.y - rc.y, b3z = rd.z - rc.z;
        min_image(a.box, b1x, b1y, b1z);
        min_image(a.box, b2x, b2y, b2z);
        min_image(a.box, b3x, b3y, b3z);
        const double n1x = b1y * b2z - b1z * b2y, n1y = b1z * b2x - b1x * b2z, n1z = b1x * b2y - b1y * b2x;
        const double n2x = b2y * b3z - b2z * b3y, n2y = b2z * b3x - b2x * b3z, n2z = b2x * b3y - b2y * b3x;
        const double b2len = sqrt(b2x * b2x + b2y * b2y + b2z * b2z);
        type = w.w & 0x3fffffffu;
        x = atan2(b2len * (b1x * n2x + b1y * n2y + b1z * n2z), n1x * n2x + n1y * n2y + n1z * n2z);
        return true;
        }
    };

template<int ARITY, bool LDS>
__global__ void __launch_bounds__(BH_BLOCK) bonded_histogram_kernel(const BhKArgs a)
    {
    extern __shared__ uint32_t s_hist[];
    const uint32_t words = a.n_types * (a.num_bins + 2);
    if (LDS)
        {
        for (uint32_t k = threadIdx.x; k < words; k += BH_BLOCK)
            s_hist[k] = 0;
        __syncthreads();
        }
    const BhSink<LDS> sink = {s_hist, a.out};
    const uint64_t first = (uint64_t)blockIdx.x * a.tiles_per_block;
    for (uint32_t t = 0; t < a.tiles_per_block; ++t)
        {
        const uint64_t row = (first + t) * BH_BLOCK + threadIdx.x;
        if (row >= a.N)
            break; // (rows ascend with t: nothing further for this lane; no barrier inside the loop)
        const uint32_t idx = (uint32_t)row;
        const uint32_t n = a.counts[idx];
        if (n == 0)
            continue;
        const bool direct = n > BH_LANE_MAX;
        const double3 p = load_scalar3_of4(a.pos, idx);
        for (uint32_t s = 0; s < n; ++s)
            {
            uint32_t type;
            double x;
            if (BhGeometry<ARITY>::coordinate(a, p, (uint64_t)s * a.pitch + idx, type, x))
                bh_count(a, sink, type, x, direct);
            }
        }
    if (LDS)
        {
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < words; k += BH_BLOCK)
            {
            const uint32_t v = s_hist[k];
            if (v)
                atomicAdd(&a.out[k], (unsigned long long)v);
            }
        }
    }

// total = the sum of the counts and of `outside`, one workgroup per type over the finished row; thread 0 stores it
__global__ void __launch_bounds__(BH_BLOCK) bonded_histogram_totals(unsigned long long* __restrict__ out, uint32_t num_bins)
    {
    __shared__ unsigned long long s_sum[BH_BLOCK];
    unsigned long long* row = out + (uint64_t)blockIdx.x * (num_bins + 2);
    unsigned long long mine = 0;
    for (uint32_t k = threadIdx.x; k <= num_bins; k += BH_BLOCK)
        mine += row[k];
    s_sum[threadIdx.x] = mine;
    __syncthreads();
    for (uint32_t half = BH_BLOCK / 2; half > 0; half >>= 1)
        {
        if (threadIdx.x < half)
            s_sum[threadIdx.x] += s_sum[threadIdx.x + half];
        __syncthreads();
        }
    if (threadIdx.x == 0)
        row[num_bins + 1] = s_sum[0];
    }

template<int ARITY>
static int bh_launch(const BhKArgs& k, bool lds, uint32_t grid, hipStream_t st)
    {
    const uint32_t bytes = lds ? k.n_types * (k.num_bins + 2) * (uint32_t)sizeof(uint32_t) : 0u;
    LaunchInfo& li = last_launch();
    li.block_size = BH_BLOCK; li.tpp = 1; li.grid = grid; li.lds_bytes = bytes;
    if (lds)
        hipLaunchKernelGGL((bonded_histogram_kernel<ARITY, true>), dim3(grid), dim3(BH_BLOCK), bytes, st, k);
    else
        hipLaunchKernelGGL((bonded_histogram_kernel<ARITY, false>), dim3(grid), dim3(BH_BLOCK), 0, st, k);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return (int)e;
    hipLaunchKernelGGL(bonded_histogram_totals, dim3(k.n_types), dim3(BH_BLOCK), 0, st, k.out, k.num_bins);
    return (int)hipGetLastError();
    }
} // namespace azp

extern "C" int azp_bonded_histogram(const azp_bonded_histogram_args* args, void* stream)
    {
    using namespace azp;
    if (!args || args->arity < 2 || args->arity > 4 || args->num_bins < 1 || args->num_bins > AZP_RDF_MAX_BINS
        || args->n_types == 0 || args->path > 2)
        return AZP_ERROR_INVALID_ARGUMENT;
    const uint64_t words = (uint64_t)args->n_types * ((uint64_t)args->num_bins + 2);
    if (words > 0xFFFFFFFFull)
        return AZP_ERROR_INVALID_ARGUMENT;
    const bool fits = words <= AZP_BONDED_HISTOGRAM_LDS_WORDS;
    if (args->path == 1 && !fits)
        return AZP_ERROR_INVALID_ARGUMENT;
    BhKArgs k = {};
    if (args->arity == 2)
        {
        if (!std::isfinite(args->r_min) || !std::isfinite(args->r_max) || !(args->r_min >= 0.0) || !(args->r_max > args->r_min))
            return AZP_ERROR_INVALID_ARGUMENT;
        k.lo = args->r_min;
        k.hi = args->r_max;
        }
    else
        {
        k.lo = args->arity == 3 ? 0.0 : -M_PI;
        // ([0, pi] and [-pi, pi] are closed: no finite x lies at or above the upper limit of the test in bh_count)
        k.hi = INFINITY;
        }
    const double upper = args->arity == 2 ? args->r_max : M_PI;
    k.scale = (double)args->num_bins / (upper - k.lo);
    hipStream_t st = static_cast<hipStream_t>(stream);
    // N == 0 succeeds before any array is looked at (as launch_bonded); a row that is given is still zeroed
    if (args->N == 0)
        return args->d_out ? (int)hipMemsetAsync(args->d_out, 0, words * sizeof(uint64_t), st) : AZP_SUCCESS;
    if (!args->d_out)
        return AZP_ERROR_INVALID_ARGUMENT;
    const hipError_t e = hipMemsetAsync(args->d_out, 0, words * sizeof(uint64_t), st);
    if (e != hipSuccess)
        return (int)e;
    if (!args->d_pos || !args->d_table || !args->d_counts || (args->arity == 2 && !args->d_table_pos)
        || args->pitch < args->N || args->N > args->n_max)
        return AZP_ERROR_INVALID_ARGUMENT;
    k.pos = args->d_pos;
    k.table = args->d_table;
    k.table_pos = args->d_table_pos;
    k.counts = args->d_counts;
    k.out = reinterpret_cast<unsigned long long*>(args->d_out);
    k.pitch = args->pitch;
    k.box = make_box_dev(args->box);
    k.N = args->N;
    k.n_max = args->n_max;
    k.n_types = args->n_types;
    k.num_bins = args->num_bins;
    const uint32_t n_tiles = (uint32_t)(((uint64_t)args->N + BH_BLOCK - 1) / BH_BLOCK);
    k.tiles_per_block = std::min(std::max((n_tiles + BH_TARGET_BLOCKS - 1) / BH_TARGET_BLOCKS, 1u), BH_TILES_PER_BLOCK);
    const uint32_t grid = (n_tiles + k.tiles_per_block - 1) / k.tiles_per_block;
    const bool lds = fits && args->path != 2;
    switch (args->arity)
        {
    case 2: return bh_launch<2>(k, lds, grid, st);
    case 3: return bh_launch<3>(k, lds, grid, st);
    default: return bh_launch<4>(k, lds, grid, st);
        }
    }
