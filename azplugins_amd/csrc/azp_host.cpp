// azp_host.cpp -- host-only parts of the C ABI: parameter-struct construction
// and inspection (what the reference's pybind11::dict constructors and
// asDict()/toPython() do), status strings, launch bookkeeping.
#include <cmath>
#include <cstring>

#include "../../include/azp.h"
#include "pair_kernel_host.hpp"

extern "C" {

// src/PairEvaluatorPerturbedLennardJones.h:33-45
void azp_plj_params_make(double epsilon, double sigma, double attraction_scale_factor, azp_plj_params* out)
    {
    const double sigma_2 = sigma * sigma;
    const double sigma_4 = sigma_2 * sigma_2;
    out->sigma_6 = sigma_2 * sigma_4;
    out->epsilon_x_4 = 4.0 * epsilon;
    out->attraction_scale_factor = attraction_scale_factor;
    out->rwcasq = std::pow(2.0, 1. / 3.) * sigma_2;
    }
// src/PairEvaluatorPerturbedLennardJones.h:47-54
void azp_plj_params_unpack(const azp_plj_params* p, double* epsilon, double* sigma, double* attraction_scale_factor)
    {
    *sigma = std::pow(p->sigma_6, 1. / 6.);
    *epsilon = p->epsilon_x_4 / 4.0;
    *attraction_scale_factor = p->attraction_scale_factor;
    }
// src/PairEvaluatorColloid.h:28-46
void azp_colloid_params_make(double A, double a_1, double a_2, double sigma, azp_colloid_params* out)
    {
    out->A = A;
    out->a_1 = a_1;
    out->a_2 = a_2;
    out->sigma_3 = sigma * sigma * sigma;
    }
void azp_colloid_params_unpack(const azp_colloid_params* p, double* A, double* a_1, double* a_2, double* sigma)
    {
    *A = p->A;
    *a_1 = p->a_1;
    *a_2 = p->a_2;
    *sigma = std::cbrt(p->sigma_3);
    }
// src/AnisoPairEvaluatorTwoPatchMorse.h:40-60
void azp_tpm_params_make(double M_d, double M_r, double r_eq, double omega, double alpha, int repulsion,
                         azp_tpm_params* out)
    {
    std::memset(out, 0, sizeof(*out));
    out->M_d = M_d;
    out->M_rinv = 1.0 / M_r;
    out->r_eq = r_eq;
    out->omega = omega;
    out->alpha = alpha;
    out->repulsion = repulsion ? 1 : 0;
    }
void azp_tpm_params_unpack(const azp_tpm_params* p, double* M_d, double* M_r, double* r_eq, double* omega,
                           double* alpha, int* repulsion)
    {
    *M_d = p->M_d;
    *M_r = 1.0 / p->M_rinv;
    *r_eq = p->r_eq;
    *omega = p->omega;
    *alpha = p->alpha;
    *repulsion = p->repulsion ? 1 : 0;
    }
// src/BondEvaluatorDoubleWell.h:33-49
void azp_dw_params_make(double r_0, double r_1, double U_1, double U_tilt, azp_dw_params* out)
    {
    out->r_1 = r_1;
    out->r_diff = r_1 - r_0;
    out->U_1 = U_1;
    out->U_tilt = U_tilt;
    }
void azp_dw_params_unpack(const azp_dw_params* p, double* r_0, double* r_1, double* U_1, double* U_tilt)
    {
    *r_0 = p->r_1 - p->r_diff;
    *r_1 = p->r_1;
    *U_1 = p->U_1;
    *U_tilt = p->U_tilt;
    }
// src/BondEvaluatorQuartic.h:36-66
void azp_quartic_params_make(double k, double r_0, double b_1, double b_2, double U_0, double sigma, double epsilon,
                             double delta, azp_quartic_params* out)
    {
    out->k = k;
    out->r_0 = r_0;
    out->b_1 = b_1;
    out->b_2 = b_2;
    out->U_0 = U_0;
    out->delta = delta;
    const double sigma_2 = sigma * sigma;
    const double sigma_4 = sigma_2 * sigma_2;
    out->sigma_6 = sigma_2 * sigma_4;
    out->epsilon_x_4 = 4.0 * epsilon;
    }
void azp_quartic_params_unpack(const azp_quartic_params* p, double* k, double* r_0, double* b_1, double* b_2,
                               double* U_0, double* sigma, double* epsilon, double* delta)
    {
    *k = p->k;
    *r_0 = p->r_0;
    *b_1 = p->b_1;
    *b_2 = p->b_2;
    *U_0 = p->U_0;
    *sigma = std::pow(p->sigma_6, 1. / 6.);
    *epsilon = p->epsilon_x_4 / 4.0;
    *delta = p->delta;
    }

// ---- special pairs (include/azp.h, "special pair forces"): LJ folds 4 eps sigma^12, 4 eps sigma^6 and r_cut^2 ----
void azp_special_pair_lj_params_make(double epsilon, double sigma, double r_cut, azp_special_pair_lj_params* out)
    {
    const double s2 = sigma * sigma;
    const double s6 = s2 * s2 * s2;
    out->lj1 = 4.0 * epsilon * s6 * s6;
    out->lj2 = 4.0 * epsilon * s6;
    out->r_cutsq = r_cut * r_cut;
    out->_pad = 0.0;
    }
void azp_special_pair_lj_params_unpack(const azp_special_pair_lj_params* p, double* epsilon, double* sigma, double* r_cut)
    {
    const bool set = p->lj1 != 0.0 && p->lj2 != 0.0;
    *sigma = set ? std::pow(p->lj1 / p->lj2, 1. / 6.) : 0.0;
    *epsilon = set ? p->lj2 * p->lj2 / (4.0 * p->lj1) : 0.0;
    *r_cut = std::sqrt(p->r_cutsq);
    }

// ---- angle potentials (include/azp.h, "angle forces"): harmonic keeps (k, t0), cosine squared folds cos t0 ----
void azp_angle_harmonic_params_make(double k, double t0, azp_angle_harmonic_params* out)
    {
    out->k = k;
    out->t0 = t0;
    }
void azp_angle_harmonic_params_unpack(const azp_angle_harmonic_params* p, double* k, double* t0)
    {
    *k = p->k;
    *t0 = p->t0;
    }
void azp_angle_cossq_params_make(double k, double t0, azp_angle_cossq_params* out)
    {
    out->k = k;
    out->cos_t0 = std::cos(t0);
    }
void azp_angle_cossq_params_unpack(const azp_angle_cossq_params* p, double* k, double* t0)
    {
    *k = p->k;
    *t0 = std::acos(p->cos_t0);
    }

// ---- dihedral potentials (include/azp.h, "dihedral forces"): periodic folds cos phi0 and sin phi0, OPLS keeps k1..k4 ----
void azp_dihedral_periodic_params_make(double k, int d, unsigned int n, double phi0, azp_dihedral_periodic_params* out)
    {
    out->k = k;
    out->cos_phi0 = std::cos(phi0);
    out->sin_phi0 = std::sin(phi0);
    out->d = d;
    out->n = n;
    }
void azp_dihedral_periodic_params_unpack(const azp_dihedral_periodic_params* p, double* k, int* d, unsigned int* n, double* phi0)
    {
    *k = p->k;
    *d = p->d;
    *n = p->n;
    *phi0 = std::atan2(p->sin_phi0, p->cos_phi0);
    }
void azp_dihedral_opls_params_make(double k1, double k2, double k3, double k4, azp_dihedral_opls_params* out)
    {
    out->k1 = k1;
    out->k2 = k2;
    out->k3 = k3;
    out->k4 = k4;
    }
void azp_dihedral_opls_params_unpack(const azp_dihedral_opls_params* p, double* k1, double* k2, double* k3, double* k4)
    {
    *k1 = p->k1;
    *k2 = p->k2;
    *k3 = p->k3;
    *k4 = p->k4;
    }

// ---- wall potentials: one type's dict folded into its parameter row (include/azp.h, "wall potentials") ----
// V and F = -dV/dr in plain IEEE double, in the order written: tests/wall_ref.py restates the two folds and agrees
// to a few ulp. src/WallEvaluatorLJ93.h:34-48 gives V and F / r for LJ93, src/WallEvaluatorColloid.h:36-41 for the
// colloid; F of the colloid is our own derivative of V:
//   d/dz (7a - z) / (z - a)^7 = 6 (z - 8a) / (z - a)^8,   d/dz (7a + z) / (z + a)^7 = -6 (z + 8a) / (z + a)^8,
//   d/dz [2az / (z^2 - a^2) + ln((z - a) / (z + a))] = -4 a^3 / (z^2 - a^2)^2.
static void wall_lj93_at(double epsilon, double sigma, double r, double* V, double* F)
    {
    const double s = sigma / r;
    const double s3 = s * s * s;
    const double s9 = s3 * s3 * s3;
    *V = epsilon * ((2.0 / 15.0) * s9 - s3);
    *F = epsilon * (1.2 * s9 - 3.0 * s3) / r;
    }

static void wall_colloid_at(double C1, double C2, double a, double z, double* V, double* F)
    {
    const double m = z - a, p = z + a;
    const double m2 = m * m, p2 = p * p;
    const double m4 = m2 * m2, p4 = p2 * p2;
    const double m7 = m4 * m2 * m, p7 = p4 * p2 * p;
    const double q = z * z - a * a;
    *V = C1 * ((7.0 * a - z) / m7 + (7.0 * a + z) / p7) - C2 * (2.0 * a * z / q + std::log(m / p));
    *F = 6.0 * C1 * ((8.0 * a - z) / (m7 * m) + (8.0 * a + z) / (p7 * p)) - 4.0 * C2 * (a * a * a) / (q * q);
    }

static int wall_row_check(double r_cut, double r_extrap, int shift_mode, double* row)
    {
    if (!row)
        return AZP_ERROR_INVALID_ARGUMENT;
    for (int k = 0; k < AZP_WALL_PARAM_DOUBLES; ++k)
        row[k] = 0.0;
    if (!(r_cut >= 0.0) || !(r_extrap >= 0.0) || (r_cut > 0.0 && r_extrap >= r_cut)
        || (shift_mode != AZP_SHIFT_NONE && shift_mode != AZP_SHIFT_SHIFT))
        return AZP_ERROR_INVALID_ARGUMENT;
    return AZP_SUCCESS;
    }

int azp_wall_lj93_params_make(double epsilon, double sigma, double r_cut, double r_extrap, int shift_mode, double* row)
    {
    const int rc = wall_row_check(r_cut, r_extrap, shift_mode, row);
    if (rc != AZP_SUCCESS)
        return rc;
    if (epsilon == 0.0 || r_cut == 0.0)
        return AZP_SUCCESS; // feels nothing: a row of zeros
    row[0] = epsilon; // (not folded into epsilon sigma^9, epsilon sigma^3: see EvalWallLJ93 in wall_forces.hip)
    row[1] = sigma;
    row[2] = r_cut;
    row[3] = r_extrap;
    double V, F;
    if (shift_mode == AZP_SHIFT_SHIFT)
        {
        wall_lj93_at(epsilon, sigma, r_cut, &V, &F);
        row[4] = V; // the reference evaluates it per particle ("could be cached once per type", WallEvaluatorLJ93.h:126)
        }
    if (r_extrap > 0.0)
        wall_lj93_at(epsilon, sigma, r_extrap, &row[5], &row[6]);
    return AZP_SUCCESS;
    }

int azp_wall_colloid_params_make(double A, double sigma, double a, double r_cut, double r_extrap, int shift_mode, double* row)
    {
    const int rc = wall_row_check(r_cut, r_extrap, shift_mode, row);
    if (rc != AZP_SUCCESS)
        return rc;
    if (A == 0.0 || !(a > 0.0) || r_cut == 0.0)
        return AZP_SUCCESS;
    if (r_cut <= a || (r_extrap > 0.0 && r_extrap <= a))
        return AZP_ERROR_INVALID_ARGUMENT;
    const double s2 = sigma * sigma;
    const double C1 = A * (s2 * s2 * s2) / 7560.0, C2 = A / 6.0;
    row[0] = C1;
    row[1] = C2;
    row[2] = r_cut;
    row[3] = r_extrap;
    row[7] = a;
    double V, F;
    if (shift_mode == AZP_SHIFT_SHIFT)
        {
        wall_colloid_at(C1, C2, a, r_cut, &V, &F);
        row[4] = V;
        }
    if (r_extrap > 0.0)
        wall_colloid_at(C1, C2, a, r_extrap, &row[5], &row[6]);
    return AZP_SUCCESS;
    }

// ---- tabulated potentials (include/azp.h, azp_table_params): samples -> rows {U_k, U_{k+1} - U_k, F_k, F_{k+1} - F_k} ----
// Each difference is ONE IEEE subtraction (tests/table_ref.py restates it bit for bit); the pair form's implicit zero at
// r_end is the minuend of the last row.
int azp_table_pack(double r_min, double r_end, const double* U, const double* F, uint32_t width, int closed, double* out_rows)
    {
    if (!U || !F || !out_rows || width < (closed ? 2u : 1u))
        return AZP_ERROR_INVALID_ARGUMENT;
    if (!std::isfinite(r_min) || !std::isfinite(r_end) || !(r_min >= 0.0) || !(r_end > r_min))
        return AZP_ERROR_INVALID_ARGUMENT;
    for (uint32_t k = 0; k < width; ++k)
        if (!std::isfinite(U[k]) || !std::isfinite(F[k]))
            return AZP_ERROR_INVALID_ARGUMENT;
    const uint32_t n = closed ? width - 1 : width;
    for (uint32_t k = 0; k < n; ++k)
        {
        const double U1 = (k + 1 < width) ? U[k + 1] : 0.0, F1 = (k + 1 < width) ? F[k + 1] : 0.0;
        double* row = out_rows + 4 * (size_t)k;
        row[0] = U[k];
        row[1] = U1 - U[k];
        row[2] = F[k];
        row[3] = F1 - F[k];
        }
    return AZP_SUCCESS;
    }

int azp_version(void)
    {
    return AZP_VERSION_MAJOR * 1000 + AZP_VERSION_MINOR;
    }

const char* azp_status_string(int status)
    {
    switch (status)
        {
    case AZP_SUCCESS: return "success";
    case AZP_ERROR_INVALID_ARGUMENT: return "invalid argument";
    case AZP_ERROR_TOO_MANY_TYPES: return "per-type-pair coefficient table exceeds 160 KiB of LDS";
    case AZP_ERROR_NO_DEVICE: return "no HIP device";
    case AZP_ERROR_TOO_MANY_BINS: return "more than 2^31 - 1 bins";
    default: return status > 0 ? "HIP runtime error (value is hipError_t)" : "unknown status";
        }
    }

void azp_last_launch(uint32_t* block_size, uint32_t* threads_per_particle, uint32_t* grid, uint32_t* lds_bytes)
    {
    const azp::LaunchInfo& li = azp::last_launch();
    if (block_size) *block_size = li.block_size;
    if (threads_per_particle) *threads_per_particle = li.tpp;
    if (grid) *grid = li.grid;
    if (lds_bytes) *lds_bytes = li.lds_bytes;
    }

} // extern "C"

namespace azp
{
LaunchInfo& last_launch()
    {
    static thread_local LaunchInfo li = {0, 0, 0, 0};
    return li;
    }
} // namespace azp
