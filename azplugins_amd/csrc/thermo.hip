// thermo.hip -- the sums behind compute.ThermodynamicQuantities: one pass over the particles of a group gives a row
// of AZP_THERMO_NSUMS = 20 doubles
//   0      particle count
//   1-3    m v                      (linear momentum)
//   4-9    m v_a v_b                (xx, xy, xz, yy, yz, zz)
//   10-15  per-particle virial      (same order, every force array added)
//   16     potential energy         (the .w of every force array)
//   17     rotational kinetic energy: sum_k s_k^2 / (2 I_k) over the axes with I_k != 0, s = 1/2 conj(q) p
//   18     number of non-zero inertia components
//   19     0
// from which the host takes temperature, pressure tensor and energies (HOOMD: ComputeThermo; its source is not
// available here, the definitions are those of compute.py). Rows [0, N) only: ghost rows are never counted. An
// optional per-type byte mask selects the group (the type is read from pos.w, as velocity_field.hip does).
//
// The sums are the reproducible two-stage sum of azp_reduce.hpp (thermo_partial: this file's particle loop, then
// reduce_block_store; reduce_fold): its header states the order of the additions and their depth. A term here passes
// at most A = 7 additions before it reaches its lane's accumulator (across the AZP_THERMO_MAX_FORCES force arrays of
// its particle), so the depth is 86 up to N = 2^24 and 182 up to N = 2^26.
//
// The terms themselves are plain IEEE operations in the order written (no contraction), so a host restatement
// reproduces every term bit for bit: m v_a v_b = (m v_a) v_b; s_x = 0.5 ((q_s p_x - p_s q_x) - (q_y p_z - q_z p_y)) and
// cyclic; the rotational term 0.5 (s_k s_k / I_k).
//
// Bytes per particle: 32 (vel) + per force 32 (the force row: 8 are used, the row's sectors are fetched) + per
// virial 48 (six coalesced streams) + 88 with the rotational arrays (orientation 32, angmom 32, inertia 24) + 32
// (pos) when a mask is given. The north-star liquid (one pair force with virial): 112 B, 117 MB at N = 2^20.
#include "azp_reduce.hpp"

namespace azp
{
constexpr uint32_t TH_BLOCK = REDUCE_BLOCK;
constexpr uint32_t TH_NS = AZP_THERMO_NSUMS;
constexpr uint32_t TH_LIVE = 19;             // slots that are summed (19 is the pad)

struct THKArgs
    {
    const double* vel;
    const double* pos;
    const uint8_t* mask;
    const double* force[AZP_THERMO_MAX_FORCES];
    const double* virial[AZP_THERMO_MAX_FORCES];
    const double* orientation;
    const double* angmom;
    const double* inertia;
    double* scratch;
    uint32_t N;
    uint32_t ntypes;
    uint32_t n_forces;
    uint32_t per_lane;
    };

#pragma clang fp contract(off)
__global__ void __launch_bounds__(TH_BLOCK) thermo_partial(const THKArgs a)
    {
    __shared__ double s_wave[REDUCE_WAVES * TH_NS];
    const uint32_t tid = threadIdx.x;
    double acc[TH_LIVE];
#pragma unroll
    for (uint32_t k = 0; k < TH_LIVE; ++k)
        acc[k] = 0.0;
    const uint64_t base = (uint64_t)blockIdx.x * TH_BLOCK * a.per_lane;
    // (the bound is the same for every thread: all 64 lanes of a wave reach the butterfly)
    for (uint32_t j = 0; j < a.per_lane; ++j)
        {
        const uint64_t i64 = base + (uint64_t)j * TH_BLOCK + tid;
        if (i64 >= a.N)
            continue;
        const uint32_t i = (uint32_t)i64;
        if (a.mask)
            {
            const uint32_t t = (uint32_t)type_from_w(a.pos[4ull * i + 3]);
            if (!(t < a.ntypes && a.mask[t] != 0))
                continue;
            }
        const double4 v = load_scalar4(a.vel, i);
        const double m = v.w;
        const double px = m * v.x, py = m * v.y, pz = m * v.z;
        acc[0] += 1.0;
        acc[1] += px; acc[2] += py; acc[3] += pz;
        acc[4] += px * v.x; acc[5] += px * v.y; acc[6] += px * v.z;
        acc[7] += py * v.y; acc[8] += py * v.z; acc[9] += pz * v.z;
        if (a.n_forces)
            {
            double w[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            double e = 0.0;
            for (uint32_t f = 0; f < a.n_forces; ++f)
                {
                e += a.force[f][4ull * i + 3];
                const double* vir = a.virial[f];
                if (vir)
                    {
#pragma unroll
                    for (uint32_t c = 0; c < 6; ++c)
                        w[c] += vir[(uint64_t)c * a.N + i];
                    }
                }
#pragma unroll
            for (uint32_t c = 0; c < 6; ++c)
                acc[10 + c] += w[c];
            acc[16] += e;
            }
        if (a.orientation)
            {
            const double4 q = load_scalar4(a.orientation, i);
            const double4 p = load_scalar4(a.angmom, i);
            const double I[3] = {a.inertia[3ull * i], a.inertia[3ull * i + 1], a.inertia[3ull * i + 2]};
            // vector part of conj(q) p / 2, scalar parts first (q.x, p.x)
            const double s[3] = {0.5 * ((q.x * p.y - p.x * q.y) - (q.z * p.w - q.w * p.z)),
                                 0.5 * ((q.x * p.z - p.x * q.z) - (q.w * p.y - q.y * p.w)),
                                 0.5 * ((q.x * p.w - p.x * q.w) - (q.y * p.z - q.z * p.y))};
            double ke = 0.0, ndof = 0.0;
#pragma unroll
            for (uint32_t k = 0; k < 3; ++k)
                if (I[k] != 0.0)
                    {
                    ke += 0.5 * (s[k] * s[k] / I[k]);
                    ndof += 1.0;
                    }
            acc[17] += ke;
            acc[18] += ndof;
            }
        }
    reduce_block_store<TH_LIVE>(acc, s_wave, a.scratch, 0, gridDim.x, blockIdx.x);
    if (tid == TH_LIVE)
        a.scratch[(uint64_t)TH_LIVE * gridDim.x + blockIdx.x] = 0.0;
    }
#pragma clang fp contract(on)

static int th_check(const azp_thermo_args* a)
    {
    if (!a || a->n_forces > AZP_THERMO_MAX_FORCES || !a->d_vel)
        return AZP_ERROR_INVALID_ARGUMENT;
    const int n_rot = (a->d_orientation != nullptr) + (a->d_angmom != nullptr) + (a->d_inertia != nullptr);
    if (n_rot != 0 && n_rot != 3)
        return AZP_ERROR_INVALID_ARGUMENT;
    if (a->d_type_mask && !a->d_pos)
        return AZP_ERROR_INVALID_ARGUMENT;
    for (uint32_t f = 0; f < a->n_forces; ++f)
        if (!a->d_force[f])
            return AZP_ERROR_INVALID_ARGUMENT;
    return AZP_SUCCESS;
    }

} // namespace azp

extern "C" int azp_thermo_scratch_size(const azp_thermo_args* args, uint64_t* bytes)
    {
    using namespace azp;
    if (!bytes)
        return AZP_ERROR_INVALID_ARGUMENT;
    const int rc = th_check(args);
    if (rc != AZP_SUCCESS)
        return rc;
    *bytes = (uint64_t)reduce_shape(args->N).n_blocks * TH_NS * sizeof(double);
    return AZP_SUCCESS;
    }

extern "C" int azp_thermo_sums(const azp_thermo_args* args, void* stream)
    {
    using namespace azp;
    const int rc = th_check(args);
    if (rc != AZP_SUCCESS)
        return rc;
    if (!args->d_out)
        return AZP_ERROR_INVALID_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (args->N == 0)
        return (int)hipMemsetAsync(args->d_out, 0, TH_NS * sizeof(double), st);
    const ReduceShape s = reduce_shape(args->N);
    if (!args->d_scratch || args->scratch_bytes < (uint64_t)s.n_blocks * TH_NS * sizeof(double))
        return AZP_ERROR_INVALID_ARGUMENT;
    THKArgs k;
    k.vel = args->d_vel;
    k.pos = args->d_pos;
    k.mask = args->d_type_mask;
    for (uint32_t f = 0; f < AZP_THERMO_MAX_FORCES; ++f)
        {
        k.force[f] = f < args->n_forces ? args->d_force[f] : nullptr;
        k.virial[f] = f < args->n_forces ? args->d_virial[f] : nullptr;
        }
    k.orientation = args->d_orientation;
    k.angmom = args->d_angmom;
    k.inertia = args->d_inertia;
    k.scratch = static_cast<double*>(args->d_scratch);
    k.N = args->N;
    k.ntypes = args->ntypes;
    k.n_forces = args->n_forces;
    k.per_lane = s.per_lane;
    hipLaunchKernelGGL(thermo_partial, dim3(s.n_blocks), dim3(TH_BLOCK), 0, st, k);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return (int)e;
    // one wave per slot, the pad included
    hipLaunchKernelGGL(reduce_fold<false>, dim3(TH_NS), dim3(WAVE), 0, st, k.scratch, s.n_blocks, args->d_out);
    return (int)hipGetLastError();
    }
