// cheb_coef.h -- the host arithmetic of the Chebyshev polynomial preconditioner of the iterative A^-1 operator (itsolve.hip): the
// coefficients of the recurrence, the Gershgorin bound on the spectrum of G A, the rule for which operators the fused step kernel
// (k_cheb_step_csr) takes, and the z panel a sweep starts in.  No HIP in here: the library compiles it for the host, tests/cpp/cheb_coef_host.cpp stands alone on it, and
// tests/cheb_reference.py restates it in numpy.
//
// z = p_K(G A) G r with the spectrum of G A in (0, hi] and the polynomial fitted to [lo, hi]:
//   theta = (hi + lo) / 2, delta = (hi - lo) / 2, sigma = theta / delta, rho_0 = 1 / sigma,
//   rho_{k+1} = 1 / (2 sigma - rho_k), a_k = rho_{k+1} rho_k, b_k = 2 rho_{k+1} / delta          (k = 0 .. K-1)
//   d = z = G r / theta;  K times:  d <- a_k d + b_k G (r - A z),  z <- z + d.
// The residual polynomial 1 - lambda p_K(lambda) is T_{K+1}((theta - lambda) / delta) / T_{K+1}(sigma): at most 1 / T_{K+1}(sigma) in
// size on [lo, hi], and between 0 and 1 on (0, lo), so p_K(G A) G is definite whenever the spectrum of G A lies in (0, hi].
#ifndef RAILS_CHEB_COEF_H
#define RAILS_CHEB_COEF_H

#include <cmath>
#include <cstdint>

constexpr int RAILS_CHEB_MAX_DEGREE = 64;

// the interval and the K coefficient pairs; false when the interval is not 0 < lo < hi (finite) or K is outside 0 .. 64
inline bool rails_cheb_coef(double lo, double hi, int K, double *theta, double *a, double *b)
{
    if (!(lo > 0.0) || !(hi > lo) || !(hi - hi == 0.0) || K < 0 || K > RAILS_CHEB_MAX_DEGREE) return false;
    const double th = 0.5 * (hi + lo), delta = 0.5 * (hi - lo), sigma = th / delta;
    double rho = 1.0 / sigma;
    for (int k = 0; k < K; ++k) {
        const double next = 1.0 / (2.0 * sigma - rho);
        a[k] = next * rho;
        b[k] = 2.0 * next / delta;
        rho = next;
    }
    *theta = th;
    return true;
}

// max_i |g_i| sum_j |a_ij| over the rows of a CSR matrix: an upper bound on the spectral radius of diag(g) A (g = nullptr: g_i = 1, the
// bound for +-A)
inline double rails_cheb_gershgorin(int64_t m, const int64_t *rowptr, const double *val, const double *g)
{
    double hi = 0.0;
    for (int64_t i = 0; i < m; ++i) {
        double s = 0.0;
        for (int64_t q = rowptr[i]; q < rowptr[i + 1]; ++q) s += std::fabs(val[q]);
        s *= g ? std::fabs(g[i]) : 1.0;
        if (!(s <= hi)) hi = s; // a NaN shows
    }
    return hi;
}

// The fused step gathers rows of a work panel at `base + row * ld * 8 + column * 8` with 24-bit row numbers and 32-bit byte offsets
// (k_spmm_narrow's scheme, spmm.hip), so it takes: a stored CSR operator, without ghost rows, of fewer than 2^24 rows, with work panels
// (m rows of ld doubles) below 4 GiB.  Anything else takes the unfused step (rails_spmm, then one pass).
inline bool rails_cheb_fused_eligible(bool stored_csr, int64_t n_ghost, int64_t m, int64_t ld)
{
    if (!stored_csr || n_ghost != 0 || m < 1 || ld < 1) return false;
    if (m >= (int64_t)1 << 24 || ld * 8 >= (int64_t)1 << 24) return false;
    return (uint64_t)m * (uint64_t)ld * 8u < 0xffffff00ull;
}

// The ghost-row form of the fused step (a row-partitioned operator with its halo plan set): column c < m is a row of the work panel
// (stride ld), column c >= m is row c - m of the operator's ghost buffer (n_ghost rows of ldg doubles, filled by the exchange the object
// makes before the step) -- k_spmm_narrow's select between two bases and two strides, each with 24-bit row numbers and 32-bit byte
// offsets.  So: a stored CSR operator, 1 <= m < 2^24 local rows and fewer than 2^24 ghost rows, both row strides times 8 below 2^24, the
// panel and the ghost buffer below 4 GiB each.
inline bool rails_cheb_fused_ghost_eligible(bool stored_csr, int64_t m, int64_t n_ghost, int64_t ld, int64_t ldg)
{
    if (!stored_csr || m < 1 || n_ghost < 0 || ld < 1 || ldg < 1) return false;
    if (m >= (int64_t)1 << 24 || n_ghost >= (int64_t)1 << 24) return false;
    if (ld * 8 >= (int64_t)1 << 24 || ldg * 8 >= (int64_t)1 << 24) return false;
    return (uint64_t)m * (uint64_t)ld * 8u < 0xffffff00ull && (uint64_t)n_ghost * (uint64_t)ldg * 8u < 0xffffff00ull;
}

// The z panel a sweep starts in, 0 the primary and 1 the other one, when `steps` steps follow its start: a fused step reads one z panel and
// writes the other (every block reads rows that other blocks own), so an odd number of them starts in the other panel and the last one
// writes the primary; an unfused step updates z in place, in the primary.
inline int rails_cheb_start_panel(bool fused, int steps) { return fused ? steps & 1 : 0; }

#endif
