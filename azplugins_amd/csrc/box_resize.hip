// box_resize.hip -- the particles of a box that changes during a run (gfx950): HOOMD's hoomd.update.BoxResize
// restated (the reference holds no box-resize code; the semantics are in include/azp.h and DESIGN 4.22).
//
// One launch over the N rows, one row per lane: a 16-byte-pair load of pos, the type's byte of the mask, the affine map
// r' = M r of a selected row (M = H_new H_old^-1, upper triangular, made on the host in float64: no division here),
// the wrap into the NEW box of every row, one store of pos and a read-modify-write of the three image counters. No
// LDS, no atomics; the result does not depend on the launch shape.
#include "azp_device.hpp"

namespace azp
{
struct BoxResizeKArgs
    {
    double* pos;
    int32_t* image;
    const uint8_t* mask;
    uint32_t N, ntypes;
    double m00, m01, m02, m11, m12, m22;
    BoxDev box;
    // the shifts of one image along z and y carried into the other axes, rounded once: Lz yz, Lz xz, Ly xy
    double lz_yz, lz_xz, ly_xy;
    };

// A row that kept its position may lie several images outside a box that has shrunk: take it back by a whole number of
// lattice vectors per periodic axis, the number read off its fractional coordinate (rint: a row on a half-integer
// stays up to one image outside, which the one-shift wrap behind this settles with the [-L/2, L/2) convention). z first,
// then y, then x, carrying the tilts in the order wrap_into_box carries them. Returns the shifts for the image counters.
__device__ __forceinline__ int3 shift_by_fraction(const BoxResizeKArgs& a, double& x, double& y, double& z)
    {
    const BoxDev& b = a.box;
    int3 n = make_int3(0, 0, 0);
    if (b.pz)
        {
        const double k = rint(z * b.Lzinv);
        z = __builtin_fma(-k, b.Lz, z);
        y = __builtin_fma(-k, a.lz_yz, y);
        x = __builtin_fma(-k, a.lz_xz, x);
        n.z = (int)k;
        }
    if (b.py)
        {
        const double k = rint((y - z * b.yz) * b.Lyinv);
        y = __builtin_fma(-k, b.Ly, y);
        x = __builtin_fma(-k, a.ly_xy, x);
        n.y = (int)k;
        }
    if (b.px)
        {
        const double k = rint((x - y * b.xy - z * (b.xz - b.xy * b.yz)) * b.Lxinv);
        x = __builtin_fma(-k, b.Lx, x);
        n.x = (int)k;
        }
    return n;
    }

__global__ void __launch_bounds__(256) box_resize_kernel(const BoxResizeKArgs a)
    {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.N)
        return;
    const double4 p = load_scalar4(a.pos, idx);
    double x = p.x, y = p.y, z = p.z;
    bool selected = true;
    if (a.mask)
        {
        const uint32_t t = (uint32_t)type_from_w(p.w);
        selected = t < a.ntypes && a.mask[t] != 0; // (a type beyond the mask is not read)
        }
    if (selected)
        {
        x = __builtin_fma(a.m02, z, __builtin_fma(a.m01, y, a.m00 * x));
        y = __builtin_fma(a.m12, z, a.m11 * y);
        z = a.m22 * z;
        }
    else
        {
        const int3 n = shift_by_fraction(a, x, y, z);
        if (a.image && (n.x | n.y | n.z))
            {
            a.image[3 * idx + 0] += n.x;
            a.image[3 * idx + 1] += n.y;
            a.image[3 * idx + 2] += n.z;
            }
        }
    wrap_with_image(a.box, x, y, z, a.image, idx);
    store_scalar4(a.pos, idx, x, y, z, p.w);
    }
} // namespace azp

extern "C" int azp_box_resize(const azp_box_resize_args* args, void* stream)
    {
    using namespace azp;
    if (!args)
        return AZP_ERROR_INVALID_ARGUMENT;
    if (args->N == 0)
        return AZP_SUCCESS;
    if (!args->d_pos || (args->d_type_mask && args->ntypes == 0))
        return AZP_ERROR_INVALID_ARGUMENT;
    for (int k = 0; k < 3; ++k)
        if (!(args->box.L[k] > 0.0) || !(args->box.L[k] <= 1.7976931348623157e308) || !(args->box.tilt[k] == args->box.tilt[k]))
            return AZP_ERROR_INVALID_ARGUMENT; // (NaN compares false)
    for (int k = 0; k < 6; ++k)
        if (!(args->M[k] - args->M[k] == 0.0)) // NaN or infinite
            return AZP_ERROR_INVALID_ARGUMENT;
    const uint32_t bs = args->block_size ? args->block_size : 256u;
    if (bs % 64 || bs > 256)
        return AZP_ERROR_INVALID_ARGUMENT;
    BoxResizeKArgs k;
    k.pos = args->d_pos;
    k.image = args->d_image;
    k.mask = args->d_type_mask;
    k.N = args->N;
    k.ntypes = args->ntypes;
    k.m00 = args->M[0]; k.m01 = args->M[1]; k.m02 = args->M[2];
    k.m11 = args->M[3]; k.m12 = args->M[4]; k.m22 = args->M[5];
    k.box = make_box_dev(args->box);
    k.lz_yz = k.box.Lz * k.box.yz;
    k.lz_xz = k.box.Lz * k.box.xz;
    k.ly_xy = k.box.Ly * k.box.xy;
    hipLaunchKernelGGL(box_resize_kernel, dim3((args->N + bs - 1) / bs), dim3(bs), 0, static_cast<hipStream_t>(stream), k);
    return (int)hipGetLastError();
    }
