// thermostat.hip -- the thermostats of ConstantVolume (azplugins_amd.thermostats: Berendsen, Bussi, MTTK; names and
// parameter keys of hoomd.md.methods.thermostats). HOOMD-blue's source is not available here: the scheme is DEFINED
// in include/azp.h and DESIGN 4.18, and tests/thermostat_ref.py restates it in numpy.
//
// A thermostat is a scalar map (K, state, t) -> alpha that acts once per step, on the full-step velocities v(t), ahead
// of step one. The kernels, their bytes and why the advance is a kernel of its own: controlled_verlet.hpp. This file is
// the policy: one sum, K = sum 1/2 m |v|^2, which reads no force (the kinetic pass moves 32 B per particle); dt by
// value; no halt; the steer v = alpha v with alpha from the state; the advance that draws the random numbers,
// computes alpha and updates the state. alpha goes through exp / log / cos / sqrt of the device library, which differ
// from a host's by a few ulp (tests/thermostat_ref.ALPHA_REL).
#include "thermostat.hpp"

extern "C" int azp_thermostat_partials_size(uint32_t N, uint64_t* bytes) { return azp::cv_partials_size<azp::Thermostat>(N, bytes); }
extern "C" int azp_thermostat_kinetic(const azp_thermostat_args* args, void* stream)
    {
    return azp::launch_cv<azp::Thermostat>(azp::CV_MEASURE, args, stream);
    }
extern "C" int azp_thermostat_step_two(const azp_thermostat_args* args, void* stream)
    {
    return azp::launch_cv<azp::Thermostat>(azp::CV_STEP_TWO, args, stream);
    }
extern "C" int azp_thermostat_advance(const azp_thermostat_args* args, void* stream)
    {
    return azp::launch_cv<azp::Thermostat>(azp::CV_ADVANCE, args, stream);
    }
extern "C" int azp_thermostat_step_one(const azp_thermostat_args* args, void* stream)
    {
    return azp::launch_cv<azp::Thermostat>(azp::CV_STEP_ONE, args, stream);
    }
