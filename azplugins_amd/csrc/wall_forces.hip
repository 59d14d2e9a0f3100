// wall_forces.hip -- wall potentials (azplugins_amd.wall): LJ 9-3 (src/WallEvaluatorLJ93.h:50-150) and colloid
// (src/WallEvaluatorColloid.h:52-195) walls on planes, spheres and cylinders, any number of walls (<= AZP_WALL_MAX)
// in one launch. The reference's headers define V(r) only; geometry, cutoff and extrapolation are defined in
// include/azp.h ("wall potentials") and DESIGN 4.13.
//
//   wall_force_kernel   pure streaming like barrier_kernel: 32 B in, 32 B out per particle, one lane per particle,
//                       the per-type rows (8 doubles) in LDS. The walls are part of the kernel arguments, so the loop
//                       over them is wave-uniform and each wall's data arrives by scalar loads. A particle is
//                       rejected on its distance d before any evaluator arithmetic (most particles of a real system
//                       are out of range of every wall).
//   wall_net_partial    the force on each wall, -sum_i F_i^(w), and its energy: blockIdx.y is the wall; the reproducible
//                       two-stage sum of azp_reduce.hpp (its header states the order and the depth), four slots per
//                       wall, finished by reduce_fold<true>, which changes the sign of the three force slots. One
//                       term per particle and slot goes straight to the lane's accumulator (A = 0 in the header's
//                       depth). Two calls on the same state give the same bits.
//
// The signed distance is computed without contraction, sums left to right, with the correctly rounded square root, so
// a host restatement has the same d to the bit (the force varies as d^-10 near a wall: an ulp of rho is 1e-13 of the
// force at d = 0.01). The evaluators are free to contract and use the refined reciprocal.
#include "azp_reduce.hpp"
#include "pair_kernel_host.hpp"

namespace azp
{
constexpr uint32_t WALL_ROW = AZP_WALL_PARAM_DOUBLES;
constexpr uint32_t WALL_NET_BLOCK = REDUCE_BLOCK;
constexpr uint32_t WALL_NET_WAVES = REDUCE_WAVES;

struct WallRow
    {
    double c0, c1, r_cut, r_extrap, shift, v_e, f_e, a;
    };

struct WallKArgs
    {
    double* force;
    const double* pos;
    const double* params;
    double* scratch;
    BoxDev box;
    uint32_t N;
    uint32_t ntypes;
    uint32_t n_walls;
    uint32_t per_lane;
    azp_wall walls[AZP_WALL_MAX];
    };

// V(d) = eps [(2/15) (sigma/d)^9 - (sigma/d)^3], F = -V'(d) = eps [(6/5) (sigma/d)^9 - 3 (sigma/d)^3] / d, from eps = c0
// and sigma = c1 as they were given. They are NOT folded into eps sigma^9 and eps sigma^3: at the force's zero,
// d = 0.86 sigma, the two terms are 13 x the energy that is left, so the rounding of a folded coefficient alone is
// 2 - 4e-15 of the result. Measured against mpmath in float64 on the host, on the parity tests' particles: 6.2e-15 for
// the folded form, 3.7e-15 for this one, 3.3e-15 for the NumPy restatement, and between this form and the restatement,
// whose roundings it shares, 5e-16 (folded: 7.7e-15, over the 7.2e-15 the tests allow). Two IEEE divisions, for
// particles in range only.
struct EvalWallLJ93
    {
    __device__ __forceinline__ static void eval(const WallRow& r, double d, double& E, double& F)
        {
        const double s = r.c1 / d;
        const double s3 = s * s * s;
        const double s9 = s3 * s3 * s3;
        E = r.c0 * ((2.0 / 15.0) * s9 - s3);
        F = r.c0 * (1.2 * s9 - 3.0 * s3) / d;
        }
    };

// V(z) = C1 [(7a - z) / (z - a)^7 + (7a + z) / (z + a)^7] - C2 [2az / (z^2 - a^2) + ln((z - a) / (z + a))],
// F = -V'(z) = 6 C1 [(8a - z) / (z - a)^8 + (8a + z) / (z + a)^8] - 4 C2 a^3 / (z^2 - a^2)^2 (derivation: azp_host.cpp).
// One reciprocal, w = 1 / (z^2 - a^2); 1 / (z - a) = (z + a) w and 1 / (z + a) = (z - a) w. The logarithm is taken as
// log1p(-2a / (z + a)): far from the wall the two C2 terms cancel to (4/3) (a/z)^3 and the rounding of the
// logarithm's argument is what is left; in this form it enters scaled by 2a / (z + a) < 1 (measured on the fixture's
// inputs in float64: 1.6e-14 of the result against 6.1e-14 for log((z - a) / (z + a)) from the shared reciprocal).
// 0 < z <= a gives a non-finite result (w of zero or the logarithm of a negative number), as the reference does.
struct EvalWallColloid
    {
    __device__ __forceinline__ static void eval(const WallRow& r, double z, double& E, double& F)
        {
        const double a = r.a;
        const double m = z - a, p = z + a;
        const double w = fast_rcp(m * p);
        const double mi = p * w, pi = m * w;
        const double mi2 = mi * mi, pi2 = pi * pi;
        const double mi7 = mi2 * mi2 * mi2 * mi, pi7 = pi2 * pi2 * pi2 * pi;
        const double aw = a * w;
        E = r.c0 * ((7.0 * a - z) * mi7 + (7.0 * a + z) * pi7) - r.c1 * (2.0 * z * aw + log1p(-2.0 * a * pi));
        F = 6.0 * r.c0 * ((8.0 * a - z) * (mi7 * mi) + (8.0 * a + z) * (pi7 * pi)) - 4.0 * r.c1 * a * (aw * aw);
        }
    };

#pragma clang fp contract(off)
// Signed distance to the wall. (sx, sy, sz) / rho is the radial unit vector of a sphere or cylinder.
__device__ __forceinline__ double wall_distance(const azp_wall& w, double x, double y, double z, double& sx, double& sy,
                                                double& sz, double& rho)
    {
    const double dx = x - w.origin[0], dy = y - w.origin[1], dz = z - w.origin[2];
    if (w.kind == AZP_WALL_PLANE)
        {
        sx = w.axis[0]; sy = w.axis[1]; sz = w.axis[2];
        rho = 1.0;
        return (w.axis[0] * dx + w.axis[1] * dy) + w.axis[2] * dz;
        }
    sx = dx; sy = dy; sz = dz;
    if (w.kind == AZP_WALL_CYLINDER)
        {
        const double t = (dx * w.axis[0] + dy * w.axis[1]) + dz * w.axis[2];
        sx = dx - t * w.axis[0]; sy = dy - t * w.axis[1]; sz = dz - t * w.axis[2];
        }
    rho = sqrt((sx * sx + sy * sy) + sz * sz);
    return w.inside ? w.radius - rho : rho - w.radius;
    }
#pragma clang fp contract(on)

// Adds what wall w does to a particle of row r at the wrapped position (x, y, z).
template<class Eval>
__device__ __forceinline__ void wall_term(const WallRow& r, const azp_wall& w, double x, double y, double z, double& fx,
                                          double& fy, double& fz, double& e)
    {
    double sx, sy, sz, rho;
    const double d = wall_distance(w, x, y, z, sx, sy, sz, rho);
    const bool linear = r.r_extrap > 0.0 && d < r.r_extrap;
    const bool standard = !linear && d > 0.0 && d < r.r_cut;
    if (!(linear || standard))
        return;
    double E, F;
    if (linear)
        {
        E = (r.v_e - r.shift) + r.f_e * (r.r_extrap - d);
        F = r.f_e;
        }
    else
        {
        Eval::eval(r, d, E, F);
        E -= r.shift;
        }
    if (w.kind != AZP_WALL_PLANE)
        {
        // u = -+s / rho (inside / outside); rho == 0: u = 0, the energy still counts
        const double g = (rho > 0.0) ? (w.inside ? -1.0 : 1.0) / rho : 0.0;
        F *= g;
        }
    fx += F * sx; fy += F * sy; fz += F * sz;
    e += E;
    }

__device__ __forceinline__ void wall_stage_rows(const WallKArgs& a, double* s_rows)
    {
    for (uint32_t t = threadIdx.x; t < a.ntypes * WALL_ROW; t += blockDim.x)
        s_rows[t] = a.params[t];
    __syncthreads();
    }

// Position of row idx wrapped into the box and the parameter row of its type (a type outside the table: zeros).
__device__ __forceinline__ WallRow wall_load(const WallKArgs& a, const double* s_rows, uint32_t idx, double& x, double& y, double& z)
    {
    const double4 p = load_scalar4(a.pos, idx);
    x = p.x; y = p.y; z = p.z;
    wrap_into_box(a.box, x, y, z);
    const uint32_t type = (uint32_t)type_from_w(p.w);
    WallRow r = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (type < a.ntypes)
        {
        const double2* q = reinterpret_cast<const double2*>(s_rows + (size_t)type * WALL_ROW);
        const double2 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
        r = WallRow {q0.x, q0.y, q1.x, q1.y, q2.x, q2.y, q3.x, q3.y};
        }
    return r;
    }

template<class Eval> __global__ void __launch_bounds__(256) wall_force_kernel(const WallKArgs a)
    {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    double* s_rows = reinterpret_cast<double*>(s_raw);
    wall_stage_rows(a, s_rows);
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.N)
        return;
    double x, y, z;
    const WallRow r = wall_load(a, s_rows, idx, x, y, z);
    double fx = 0.0, fy = 0.0, fz = 0.0, e = 0.0;
    for (uint32_t w = 0; w < a.n_walls; ++w)
        wall_term<Eval>(r, a.walls[w], x, y, z, fx, fy, fz, e);
    store_scalar4(a.force, idx, fx, fy, fz, e);
    }

// grid (n_blocks, n_walls); dynamic LDS: the rows, then WALL_NET_WAVES x 4 doubles
template<class Eval> __global__ void __launch_bounds__(WALL_NET_BLOCK) wall_net_partial(const WallKArgs a)
    {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    double* s_rows = reinterpret_cast<double*>(s_raw);
    double* s_wave = s_rows + (size_t)a.ntypes * WALL_ROW;
    wall_stage_rows(a, s_rows);
    const uint32_t tid = threadIdx.x;
    const azp_wall& wall = a.walls[blockIdx.y];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const uint64_t base = (uint64_t)blockIdx.x * WALL_NET_BLOCK * a.per_lane;
    // (the bound is the same for every thread: all 64 lanes of a wave reach the butterfly)
    for (uint32_t j = 0; j < a.per_lane; ++j)
        {
        const uint64_t i64 = base + (uint64_t)j * WALL_NET_BLOCK + tid;
        if (i64 >= a.N)
            continue;
        double x, y, z;
        const WallRow r = wall_load(a, s_rows, (uint32_t)i64, x, y, z);
        double f[4] = {0.0, 0.0, 0.0, 0.0};
        wall_term<Eval>(r, wall, x, y, z, f[0], f[1], f[2], f[3]);
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k)
            acc[k] += f[k];
        }
    reduce_block_store<4>(acc, s_wave, a.scratch, blockIdx.y * 4, gridDim.x, blockIdx.x);
    }

// what does not depend on the arrays: walls, block size, table size
static int wall_check(const azp_wall_args* a)
    {
    if (!a || a->n_walls == 0 || a->n_walls > AZP_WALL_MAX)
        return AZP_ERROR_INVALID_ARGUMENT;
    for (uint32_t w = 0; w < a->n_walls; ++w)
        if (a->walls[w].kind > AZP_WALL_CYLINDER)
            return AZP_ERROR_INVALID_ARGUMENT;
    if (a->block_size % 64 || a->block_size > 256)
        return AZP_ERROR_INVALID_ARGUMENT;
    if (sizeof(double) * WALL_ROW * (size_t)a->ntypes + sizeof(double) * 4 * WALL_NET_WAVES > 64 * 1024)
        return AZP_ERROR_TOO_MANY_TYPES;
    return AZP_SUCCESS;
    }

static void wall_fill(WallKArgs& k, const azp_wall_args* a)
    {
    k.force = a->d_force;
    k.pos = a->d_pos;
    k.params = a->d_params;
    k.scratch = nullptr;
    k.box = make_box_dev(a->box);
    k.N = a->N;
    k.ntypes = a->ntypes;
    k.n_walls = a->n_walls;
    k.per_lane = 1;
    for (uint32_t w = 0; w < AZP_WALL_MAX; ++w)
        {
        if (w < a->n_walls)
            k.walls[w] = a->walls[w];
        else
            k.walls[w] = azp_wall {AZP_WALL_PLANE, 0u, {0.0, 0.0, 0.0}, {0.0, 0.0, 1.0}, 0.0};
        }
    }

template<class Eval> static int launch_wall_forces(const azp_wall_args* args, void* stream)
    {
    const int rc = wall_check(args);
    if (rc != AZP_SUCCESS)
        return rc;
    if (args->N == 0)
        return AZP_SUCCESS;
    if (!args->d_force || !args->d_pos || !args->d_params || args->ntypes == 0)
        return AZP_ERROR_INVALID_ARGUMENT;
    const uint32_t bs = args->block_size ? args->block_size : 256u;
    const size_t lds = sizeof(double) * WALL_ROW * (size_t)args->ntypes;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (args->d_virial)
        {
        hipError_t e = hipMemsetAsync(args->d_virial, 0, sizeof(double) * 6 * args->virial_pitch, s);
        if (e != hipSuccess)
            return (int)e;
        }
    WallKArgs k;
    wall_fill(k, args);
    const uint32_t grid = (args->N + bs - 1) / bs;
    LaunchInfo& li = last_launch();
    li.block_size = bs; li.tpp = 1; li.grid = grid; li.lds_bytes = (uint32_t)lds;
    hipLaunchKernelGGL(wall_force_kernel<Eval>, dim3(grid), dim3(bs), lds, s, k);
    return (int)hipGetLastError();
    }

static uint64_t wall_net_scratch_bytes(const azp_wall_args* a)
    {
    return (uint64_t)reduce_shape(a->N).n_blocks * 4 * a->n_walls * sizeof(double);
    }

template<class Eval>
static int launch_wall_net(const azp_wall_args* args, double* d_out, void* d_scratch, uint64_t scratch_bytes, void* stream)
    {
    const int rc = wall_check(args);
    if (rc != AZP_SUCCESS)
        return rc;
    if (!d_out)
        return AZP_ERROR_INVALID_ARGUMENT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (args->N == 0)
        return (int)hipMemsetAsync(d_out, 0, sizeof(double) * 4 * args->n_walls, s);
    if (!args->d_pos || !args->d_params || args->ntypes == 0 || !d_scratch || scratch_bytes < wall_net_scratch_bytes(args))
        return AZP_ERROR_INVALID_ARGUMENT;
    const ReduceShape shape = reduce_shape(args->N);
    WallKArgs k;
    wall_fill(k, args);
    k.force = nullptr;
    k.scratch = static_cast<double*>(d_scratch);
    k.per_lane = shape.per_lane;
    const size_t lds = sizeof(double) * WALL_ROW * (size_t)args->ntypes + sizeof(double) * 4 * WALL_NET_WAVES;
    hipLaunchKernelGGL(wall_net_partial<Eval>, dim3(shape.n_blocks, args->n_walls), dim3(WALL_NET_BLOCK), lds, s, k);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return (int)e;
    hipLaunchKernelGGL(reduce_fold<true>, dim3(4 * args->n_walls), dim3(WAVE), 0, s, k.scratch, shape.n_blocks, d_out);
    return (int)hipGetLastError();
    }
} // namespace azp

extern "C" int azp_wall_forces_lj93(const azp_wall_args* args, void* stream)
    {
    return azp::launch_wall_forces<azp::EvalWallLJ93>(args, stream);
    }
extern "C" int azp_wall_forces_colloid(const azp_wall_args* args, void* stream)
    {
    return azp::launch_wall_forces<azp::EvalWallColloid>(args, stream);
    }
extern "C" int azp_wall_net_forces_scratch_size(const azp_wall_args* args, uint64_t* bytes)
    {
    if (!bytes)
        return AZP_ERROR_INVALID_ARGUMENT;
    const int rc = azp::wall_check(args);
    if (rc != AZP_SUCCESS)
        return rc;
    *bytes = azp::wall_net_scratch_bytes(args);
    return AZP_SUCCESS;
    }
extern "C" int azp_wall_net_forces_lj93(const azp_wall_args* args, double* d_out, void* d_scratch, uint64_t scratch_bytes, void* stream)
    {
    return azp::launch_wall_net<azp::EvalWallLJ93>(args, d_out, d_scratch, scratch_bytes, stream);
    }
extern "C" int azp_wall_net_forces_colloid(const azp_wall_args* args, double* d_out, void* d_scratch, uint64_t scratch_bytes, void* stream)
    {
    return azp::launch_wall_net<azp::EvalWallColloid>(args, d_out, d_scratch, scratch_bytes, stream);
    }
