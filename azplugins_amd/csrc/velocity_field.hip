// velocity_field.hip -- mass and momentum summed per bin of a 1-, 2- or 3-D grid in Cartesian or cylindrical
// coordinates, and the mass-averaged velocity of every bin: one kernel family behind
// compute.VelocityCompute (the Cartesian case with num_bins = (0, 0, 0): one bin) and
// compute.{Cartesian,Cylindrical}VelocityFieldCompute.
//
// Semantics restated from the reference: the per-particle loop of src/VelocityFieldComputeGPU.cuh:35-71 and
// src/VelocityComputeGPU.cu:48-65, the bin index of src/BinningOperation.h (floor(((x - lo) / (hi - lo)) * n), in
// this order, no reciprocal), src/CartesianBinningOperation.h (momentum as it is) and
// src/CylindricalBinningOperation.h (z, then theta = atan2(y, x) in [0, 2 pi), then r; the momentum rotated by
// (x / r, y / r), or (1, 0) at r = 0). Rows [0, N) only: ghost rows are never counted.
//
// The reference adds every particle with a double atomicAdd into its bin; the order of those adds, and so the
// result, depends on scheduling, and with one bin every atomic hits one address. Here nothing is atomic:
//   vf_partial  grid = (bin tile, particle chunk). A workgroup reads its chunk of particles once and keeps the bins
//               of its tile. Inside a wave, the lanes that share the bin of the first pending lane are summed with
//               a fixed DPP / permute butterfly (group_sum<64>) and that lane adds the four sums (mass, px, py, pz)
//               to the wave's own LDS histogram; repeated until every lane is done (sorted particles touch few
//               bins per wave, so there are few rounds). The four wave histograms are added in wave order into
//               the workgroup's slab of the scratch buffer: slab[chunk][bin] (4 doubles).
//   vf_fold     sums the slabs of each bin in a fixed tree: lane l of a wave takes component l % 4 of the slabs
//               l / 4, l / 4 + 16, ... in turn, then a butterfly over the 16 slab groups.
//   vf_normalize  momentum / mass, or 0 where the mass is 0 (src/VelocityFieldCompute.h:262-278); on a decomposed
//               run it runs after the cross-rank reduction of the sums.
// Every particle, lane and slab is added in an order fixed by the data and the launch shape: two calls on the same
// state give bit-identical sums.
//
// Bytes: 64 per particle per tile (pos + vel), 32 per bin per chunk written and read once more by the fold, 32 per
// bin of output. The chunk count keeps the scratch within VF_SCRATCH_BUDGET (at least one chunk: the scratch of a
// field with more bins than the budget holds is bins x 32 B).
#include <algorithm>

#include "azp_device.hpp"
#include "field_bin.hpp"

namespace azp
{
constexpr uint32_t VF_BLOCK = 256;
constexpr uint32_t VF_WAVES = VF_BLOCK / WAVE;
constexpr uint32_t VF_TILE = 512;                       // bins per workgroup: 4 wave histograms x 512 x 32 B = 64 KiB LDS
constexpr uint32_t VF_MIN_CHUNK = 1024;                 // particles per chunk at least
constexpr uint32_t VF_TARGET_BLOCKS = 2048;             // workgroups of one vf_partial launch to aim for (256 CUs)
constexpr uint64_t VF_SCRATCH_BUDGET = 64ull << 20;     // bytes of slabs
constexpr uint64_t VF_MAX_BINS = 2147483647ull;         // 2^31 - 1 (the reference's MPI path: an int count)

struct VFShape
    {
    uint64_t n_bins;
    uint32_t n_tiles;
    uint32_t n_chunks;
    uint32_t chunk_len;
    };

static int vf_shape(const azp_velocity_field_args* a, VFShape& s)
    {
    uint64_t nb = 1;
    for (int d = 0; d < 3; ++d)
        {
        if (a->num_bins[d] == 0)
            continue;
        nb *= a->num_bins[d];
        if (nb > VF_MAX_BINS)
            return AZP_ERROR_TOO_MANY_BINS;
        if (!(a->upper[d] > a->lower[d]))
            return AZP_ERROR_INVALID_ARGUMENT;
        }
    if (a->coordinates != AZP_COORDINATES_CARTESIAN && a->coordinates != AZP_COORDINATES_CYLINDRICAL)
        return AZP_ERROR_INVALID_ARGUMENT;
    s.n_bins = nb;
    s.n_tiles = (uint32_t)((nb + VF_TILE - 1) / VF_TILE);
    const uint64_t by_budget = std::max<uint64_t>(1, VF_SCRATCH_BUDGET / (nb * 32ull));
    const uint64_t by_blocks = std::max<uint64_t>(1, VF_TARGET_BLOCKS / s.n_tiles);
    const uint64_t by_rows = std::max<uint64_t>(1, (a->N + VF_MIN_CHUNK - 1) / VF_MIN_CHUNK);
    s.n_chunks = (uint32_t)std::min(std::min(by_budget, by_blocks), by_rows);
    s.chunk_len = (uint32_t)((a->N + (uint64_t)s.n_chunks - 1) / s.n_chunks);
    return AZP_SUCCESS;
    }

struct VFKArgs
    {
    const double* pos;
    const double* vel;
    const uint8_t* mask;
    double* scratch;
    BoxDev box;
    double lo[3], hi[3];
    uint32_t nb[3];          // 0: not binned
    uint32_t N;
    uint32_t ntypes;
    uint32_t chunk_len;
    uint64_t n_bins;
    };

#pragma clang fp contract(off)
// (no contraction below, as in bin_1d / bin_particle of field_bin.hpp: the momentum terms and the sums are the plain
// IEEE operations in the order written)

template<int COORDS> __global__ void __launch_bounds__(VF_BLOCK) vf_partial(const VFKArgs a)
    {
    extern __shared__ __attribute__((aligned(16))) double s_hist[]; // VF_WAVES x tile_bins x 4
    const uint64_t tile_lo = (uint64_t)blockIdx.x * VF_TILE;
    const uint32_t tile_bins = (uint32_t)std::min<uint64_t>(VF_TILE, a.n_bins - tile_lo);
    const uint32_t chunk = blockIdx.y;
    const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    for (uint32_t e = tid; e < VF_WAVES * tile_bins * 4; e += VF_BLOCK)
        s_hist[e] = 0.0;
    __syncthreads();
    double* hist = s_hist + (size_t)wave * tile_bins * 4;

    const uint32_t p0 = (uint32_t)std::min<uint64_t>(a.N, (uint64_t)chunk * a.chunk_len);
    const uint32_t p1 = (uint32_t)std::min<uint64_t>(a.N, (uint64_t)p0 + a.chunk_len);
    // (the loop bound is the same for every thread: all 64 lanes of a wave take part in every butterfly)
    for (uint32_t base = p0; base < p1; base += VF_BLOCK)
        {
        const uint32_t i = base + tid;
        bool ok = i < p1;
        uint32_t local = 0;
        double m = 0.0, px = 0.0, py = 0.0, pz = 0.0;
        if (ok)
            {
            const double4 p = load_scalar4(a.pos, i);
            const double4 v = load_scalar4(a.vel, i);
            const uint32_t t = (uint32_t)type_from_w(p.w);
            if (a.mask)
                ok = t < a.ntypes && a.mask[t] != 0;
            double x = p.x, y = p.y, z = p.z;
            wrap_into_box(a.box, x, y, z);
            m = v.w;
            px = v.x * m; py = v.y * m; pz = v.z * m;
            uint64_t bin = 0;
            ok = ok && bin_particle<COORDS>(a, x, y, z, px, py, bin);
            ok = ok && bin >= tile_lo && bin < tile_lo + tile_bins;
            local = (uint32_t)(bin - tile_lo);
            }
        uint64_t pending = __ballot(ok);
        while (pending)
            {
            const int leader = __ffsll((unsigned long long)pending) - 1;
            const uint32_t b0 = (uint32_t)__shfl((int)local, leader, WAVE);
            const bool mine = ok && local == b0;
            pending &= ~(uint64_t)__ballot(mine);
            const double sm = group_sum<WAVE>(mine ? m : 0.0);
            const double sx = group_sum<WAVE>(mine ? px : 0.0);
            const double sy = group_sum<WAVE>(mine ? py : 0.0);
            const double sz = group_sum<WAVE>(mine ? pz : 0.0);
            ok = ok && !mine;
            if ((int)lane == leader)
                {
                double* h = hist + 4 * (size_t)b0;
                h[0] += sm; h[1] += sx; h[2] += sy; h[3] += sz;
                }
            }
        }
    __syncthreads();
    double* slab = a.scratch + ((uint64_t)chunk * a.n_bins + tile_lo) * 4;
    const uint32_t n = tile_bins * 4;
    for (uint32_t e = tid; e < n; e += VF_BLOCK)
        {
        double s = s_hist[e];
        for (uint32_t w = 1; w < VF_WAVES; ++w)
            s += s_hist[(size_t)w * n + e];
        slab[e] = s;
        }
    }

// one wave per bin: lane l sums component l % 4 over the slabs l / 4, l / 4 + 16, ...; butterfly over the 16 groups
__global__ void __launch_bounds__(VF_BLOCK) vf_fold(const double* scratch, uint64_t n_bins, uint32_t n_chunks, double* sums)
    {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t c = lane & 3u, g = lane >> 2;
    const uint64_t stride = (uint64_t)gridDim.x * VF_WAVES;
    for (uint64_t bin = (uint64_t)blockIdx.x * VF_WAVES + threadIdx.x / WAVE; bin < n_bins; bin += stride)
        {
        double s = 0.0;
        // (unrolled: eight independent loads in flight per lane; the adds keep their order)
#pragma unroll 8
        for (uint32_t k = g; k < n_chunks; k += 16)
            s += scratch[((uint64_t)k * n_bins + bin) * 4 + c];
        s += __shfl_xor(s, 4, WAVE);
        s += __shfl_xor(s, 8, WAVE);
        s += __shfl_xor(s, 16, WAVE);
        s += __shfl_xor(s, 32, WAVE);
        if (g == 0)
            sums[bin * 4 + c] = s;
        }
    }

__global__ void __launch_bounds__(VF_BLOCK) vf_normalize(const double* sums, uint64_t n_bins, double* velocity)
    {
    const uint64_t stride = (uint64_t)gridDim.x * VF_BLOCK;
    for (uint64_t bin = (uint64_t)blockIdx.x * VF_BLOCK + threadIdx.x; bin < n_bins; bin += stride)
        {
        const double m = sums[4 * bin];
        double vx = 0.0, vy = 0.0, vz = 0.0;
        if (m > 0.0)
            {
            vx = sums[4 * bin + 1] / m;
            vy = sums[4 * bin + 2] / m;
            vz = sums[4 * bin + 3] / m;
            }
        velocity[3 * bin] = vx;
        velocity[3 * bin + 1] = vy;
        velocity[3 * bin + 2] = vz;
        }
    }
#pragma clang fp contract(on)

static uint32_t grid_for(uint64_t items, uint64_t per_block)
    {
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((items + per_block - 1) / per_block, 65536));
    }

} // namespace azp

extern "C" int azp_velocity_field_scratch_size(const azp_velocity_field_args* args, uint64_t* bytes)
    {
    using namespace azp;
    if (!args || !bytes)
        return AZP_ERROR_INVALID_ARGUMENT;
    VFShape s;
    const int rc = vf_shape(args, s);
    if (rc != AZP_SUCCESS)
        return rc;
    *bytes = (uint64_t)s.n_chunks * s.n_bins * 32ull;
    return AZP_SUCCESS;
    }

extern "C" int azp_velocity_field_sums(const azp_velocity_field_args* args, void* stream)
    {
    using namespace azp;
    if (!args || !args->d_sums)
        return AZP_ERROR_INVALID_ARGUMENT;
    VFShape s;
    const int rc = vf_shape(args, s);
    if (rc != AZP_SUCCESS)
        return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (args->N == 0)
        return (int)hipMemsetAsync(args->d_sums, 0, s.n_bins * 32ull, st);
    if (!args->d_pos || !args->d_vel || !args->d_scratch || args->scratch_bytes < (uint64_t)s.n_chunks * s.n_bins * 32ull)
        return AZP_ERROR_INVALID_ARGUMENT;
    VFKArgs k;
    k.pos = args->d_pos;
    k.vel = args->d_vel;
    k.mask = args->d_type_mask;
    k.scratch = static_cast<double*>(args->d_scratch);
    k.box = make_box_dev(args->box);
    for (int d = 0; d < 3; ++d)
        {
        k.lo[d] = args->lower[d];
        k.hi[d] = args->upper[d];
        k.nb[d] = args->num_bins[d];
        }
    k.N = args->N;
    k.ntypes = args->ntypes;
    k.chunk_len = s.chunk_len;
    k.n_bins = s.n_bins;
    const size_t lds = (size_t)VF_WAVES * std::min<uint64_t>(VF_TILE, s.n_bins) * 32;
    const dim3 grid(s.n_tiles, s.n_chunks);
    if (args->coordinates == AZP_COORDINATES_CARTESIAN)
        hipLaunchKernelGGL(vf_partial<AZP_COORDINATES_CARTESIAN>, grid, dim3(VF_BLOCK), lds, st, k);
    else
        hipLaunchKernelGGL(vf_partial<AZP_COORDINATES_CYLINDRICAL>, grid, dim3(VF_BLOCK), lds, st, k);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return (int)e;
    hipLaunchKernelGGL(vf_fold, dim3(grid_for(s.n_bins, VF_WAVES)), dim3(VF_BLOCK), 0, st, k.scratch, s.n_bins, s.n_chunks,
                       args->d_sums);
    return (int)hipGetLastError();
    }

extern "C" int azp_velocity_field_normalize(const double* d_sums, uint64_t n_bins, double* d_velocity, void* stream)
    {
    using namespace azp;
    if (n_bins == 0)
        return AZP_SUCCESS;
    if (!d_sums || !d_velocity || n_bins > VF_MAX_BINS)
        return AZP_ERROR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(vf_normalize, dim3(grid_for(n_bins, VF_BLOCK)), dim3(VF_BLOCK), 0, static_cast<hipStream_t>(stream), d_sums,
                       n_bins, d_velocity);
    return (int)hipGetLastError();
    }
