// steinhardt_device.hpp -- the arithmetic of compute.Steinhardt / compute.SolidLiquid that has to be the same wherever it
// runs: one bond's spherical harmonics as fixed-point words (the term), and a particle's q_lm, q_l and normalised q_lm
// from its sums (the finish). __host__ __device__ and free of HIP types, so that a host program can compile it with a
// plain C++ compiler (tests/test_steinhardt.py does). Semantics: include/azp.h, DESIGN 4.28.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define AZP_HD __host__ __device__
#else
#define AZP_HD
#endif

namespace azp
{
constexpr uint32_t ST_MAX_TERMS = 4;   // AZP_STEINHARDT_MAX_TERMS
constexpr uint32_t ST_MAX_L = 12;      // AZP_STEINHARDT_MAX_L
constexpr double ST_FIXED = 1099511627776.0;          // 2^40
constexpr double ST_FIXED_INV = 1.0 / 1099511627776.0; // 2^-40, exact

// The l of a call. A particle owns `words` int64: term t at offset[t], its component m at offset[t] + 2 m (Re) and
// offset[t] + 2 m + 1 (Im; the word of m = 0 stays 0).
struct SteinhardtTerms
    {
    uint32_t n_terms, l_max, words;
    uint32_t l[ST_MAX_TERMS];
    uint32_t offset[ST_MAX_TERMS];
    int32_t term_of_l[ST_MAX_L + 1];           // -1: l is not asked for
    double norm[ST_MAX_TERMS][ST_MAX_L + 1];   // N_lm = sqrt((2l+1)/(4 pi) (l-m)!/(l+m)!), from the caller
    double rcp[ST_MAX_L + 1];                  // rcp[k] = 1.0 / k, correctly rounded (rcp[0] unused)
    };

// false: not 1 .. 4 distinct l in 1 .. 12
inline bool steinhardt_make_terms(uint32_t n_terms, const uint32_t* l, const double norm[][ST_MAX_L + 1], SteinhardtTerms& s)
    {
    if (n_terms < 1 || n_terms > ST_MAX_TERMS)
        return false;
    s.n_terms = n_terms;
    s.l_max = 0;
    s.words = 0;
    for (uint32_t k = 0; k <= ST_MAX_L; ++k)
        {
        s.term_of_l[k] = -1;
        s.rcp[k] = k ? 1.0 / (double)k : 0.0;
        }
    for (uint32_t t = 0; t < ST_MAX_TERMS; ++t)
        {
        s.l[t] = 0;
        s.offset[t] = 0;
        for (uint32_t m = 0; m <= ST_MAX_L; ++m)
            s.norm[t][m] = 0.0;
        }
    for (uint32_t t = 0; t < n_terms; ++t)
        {
        if (l[t] < 1 || l[t] > ST_MAX_L || s.term_of_l[l[t]] >= 0)
            return false;
        s.l[t] = l[t];
        s.term_of_l[l[t]] = (int32_t)t;
        s.offset[t] = s.words;
        s.words += 2 * (l[t] + 1);
        if (l[t] > s.l_max)
            s.l_max = l[t];
        for (uint32_t m = 0; m <= l[t]; ++m)
            {
            if (!(norm[t][m] > 0.0) || !(norm[t][m] < 2.0))  // (every N_lm lies in (0, sqrt(25 / (4 pi))]; a NaN fails both)
                return false;
            s.norm[t][m] = norm[t][m];
            }
        }
    return true;
    }

// The term of one bond (x, y, z), rsq = x^2 + y^2 + z^2 as the caller summed it: emit(word, value) for every (l, m >= 0)
// asked for, value = llrint(Re or Im of Y_lm * 2^40). Y_lm = N_lm Q_l^m(z / r) ((x + i y) / r)^m: no trigonometry, no
// pole (Q_l^m = P_l^m / (1 - z^2)^(m / 2) is a polynomial). r = sqrt(rsq) and the three quotients are IEEE; the powers of
// (x + i y) / r by repeated complex multiplication; Q by the upward recurrence in l at fixed m,
//   Q_m^m = (-1)^m (2m - 1)!!,  (l + 1 - m) Q_(l+1)^m = (2l + 1) z Q_l^m - (l + m) Q_(l-1)^m,
// the division by l + 1 - m as a multiplication with rcp[l + 1 - m]. A bond of length 0 has no direction: no term.
template<class Emit>
AZP_HD inline void steinhardt_term(const SteinhardtTerms& s, double x, double y, double z, double rsq, Emit&& emit)
    {
    if (!(rsq > 0.0))
        return;
    const double r = sqrt(rsq);
    const double ux = x / r, uy = y / r, uz = z / r;
    double cm = 1.0, sm = 0.0;  // ((x + i y) / r)^m
    double qmm = 1.0;           // Q_m^m
    double fm = 0.0;            // m as a double
    for (uint32_t m = 0; m <= s.l_max; ++m)
        {
        if (m)
            {
            const double c = cm * ux - sm * uy;
            sm = cm * uy + sm * ux;
            cm = c;
            qmm *= -(2.0 * fm - 1.0);
            }
        double ql = qmm, qprev = 0.0, fl = fm;
        for (uint32_t l = m;; ++l)
            {
            const int32_t t = s.term_of_l[l];
            if (t >= 0)
                {
                const double f = s.norm[t][m] * ql;
                const uint32_t w = s.offset[t] + 2 * m;
                emit(w, (long long)llrint(f * cm * ST_FIXED));
                if (m)
                    emit(w + 1, (long long)llrint(f * sm * ST_FIXED));
                }
            if (l == s.l_max)
                break;
            const double qn = ((2.0 * fl + 1.0) * uz * ql - (fl + fm) * qprev) * s.rcp[l + 1 - m];
            qprev = ql;
            ql = qn;
            fl += 1.0;
            }
        fm += 1.0;
        }
    }

// q_lm component from its fixed-point sum: double(S) 2^-40 / denom, 0 where denom == 0 (denom = N_b, or N_b + 1 for the
// neighbour average)
AZP_HD inline double steinhardt_component(long long sum, double denom)
    {
    return denom > 0.0 ? (double)sum * ST_FIXED_INV / denom : 0.0;
    }

// sum over m = -l .. l of |q_lm|^2 from the stored m >= 0: |q_l0|^2 + 2 sum_{m>0} |q_lm|^2, added in the order m = 0, 1, ..
AZP_HD inline double steinhardt_norm_sq(const long long* w, uint32_t l, double denom)
    {
    double acc = 0.0;
    for (uint32_t m = 0; m <= l; ++m)
        {
        const double re = steinhardt_component(w[2 * m], denom), im = steinhardt_component(w[2 * m + 1], denom);
        const double t = re * re + im * im;
        acc += m ? 2.0 * t : t;
        }
    return acc;
    }

// q_l = sqrt(4 pi / (2l + 1) sum_m |q_lm|^2)
AZP_HD inline double steinhardt_ql(const long long* w, uint32_t l, double denom)
    {
    return sqrt(4.0 * 3.14159265358979323846 / (2.0 * (double)l + 1.0) * steinhardt_norm_sq(w, l, denom));
    }
} // namespace azp
