// field_bin.hpp -- the bin of a particle in a 1-, 2- or 3-D grid in Cartesian or cylindrical coordinates: the one
// arithmetic behind velocity_field.hip and thermo_field.hip (the reference's src/BinningOperation.h,
// src/CartesianBinningOperation.h and src/CylindricalBinningOperation.h restated). The argument struct of the caller
// carries lo[3], hi[3] and nb[3] (0: not binned).
#pragma once

#include "azp_device.hpp"

namespace azp
{
#pragma clang fp contract(off)
// (no contraction below: the bin of a particle on a bin edge, r = sqrt(x x + y y) and the rotated momentum are the
// plain IEEE operations of the reference's host path, so tests can place particles exactly on bin edges)

// floor(((x - lo) / (hi - lo)) * n) in [0, n), else false (src/BinningOperation.h)
__device__ __forceinline__ bool bin_1d(double x, double lo, double hi, uint32_t n, uint32_t& b)
    {
    const double f = floor(((x - lo) / (hi - lo)) * (double)n);
    if (!(f >= 0.0 && f < (double)n))
        return false;
    b = (uint32_t)f;
    return true;
    }

// raveled bin of the particle and its (transformed) momentum; false if it lies outside the grid
template<int COORDS, class Args>
__device__ __forceinline__ bool bin_particle(const Args& a, double x, double y, double z, double& px, double& py,
                                             uint64_t& bin)
    {
    uint32_t b[3] = {0, 0, 0};
    if (COORDS == AZP_COORDINATES_CARTESIAN)
        {
        if (a.nb[0] && !bin_1d(x, a.lo[0], a.hi[0], a.nb[0], b[0])) return false;
        if (a.nb[1] && !bin_1d(y, a.lo[1], a.hi[1], a.nb[1], b[1])) return false;
        if (a.nb[2] && !bin_1d(z, a.lo[2], a.hi[2], a.nb[2], b[2])) return false;
        }
    else
        {
        if (a.nb[2] && !bin_1d(z, a.lo[2], a.hi[2], a.nb[2], b[2])) return false;
        if (a.nb[1])
            {
            double theta = atan2(y, x);
            if (theta < 0.0)
                theta += 2.0 * M_PI;
            if (!bin_1d(theta, a.lo[1], a.hi[1], a.nb[1], b[1])) return false;
            }
        const double r = sqrt(x * x + y * y);
        if (a.nb[0] && !bin_1d(r, a.lo[0], a.hi[0], a.nb[0], b[0])) return false;
        double c = 1.0, s = 0.0;
        if (r > 0.0)
            {
            c = x / r;
            s = y / r;
            }
        const double pr = c * px + s * py;
        const double pt = -s * px + c * py;
        px = pr;
        py = pt;
        }
    const uint64_t ny = a.nb[1] ? a.nb[1] : 1u, nz = a.nb[2] ? a.nb[2] : 1u;
    bin = (uint64_t)b[2] + nz * ((uint64_t)b[1] + ny * (uint64_t)b[0]);
    return true;
    }
#pragma clang fp contract(on)

} // namespace azp
