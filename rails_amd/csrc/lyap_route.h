// lyap_route.h -- everything in the projected Lyapunov solve (rails_sb03md, lyap_dense.cpp) that DECIDES without computing: which route
// a call may take, which of the iterative routes it attempts and how long a route that failed rests, whether the factored ADI route may
// build on the call before, and Wachspress' shift parameters.  Plain arithmetic and state: no LAPACK, no I/O.  Checked on the host alone
// by tests/cpp/lyap_route_host.cpp.
#pragma once
#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

namespace lyap {

// ---- the gates (`on` is the route's switch of the environment)
// Symmetric A: the eigen-decomposition route.  The size decides whether A is measured at all, the measurement (largest modulus amax,
// largest |a_ij - a_ji| asym) whether it is symmetric to rounding.
inline bool symmetry_is_measured(int n, bool on) { return on && n >= 8; }
inline bool symmetric_to_rounding(double asym, double amax) { return amax > 0.0 && asym <= 1e-13 * amax; }
// The iterative routes (factored ADI, squared Smith): below 32 rows Bartels-Stewart costs less than their set-up.
inline bool iterative_gate(int n, bool on) { return on && n >= 32; }
// dtrsyl3 (level 3) instead of dtrsyl in the Schur route: 2-4x faster at n = 128..256, same equation.
inline bool blocked_sylvester_gate(int n, bool on) { return on && n >= 64; }
// The ADI steps as explicit operators (one product per term) instead of a pair of triangular solves.
inline bool explicit_steps_gate(int n, bool on) { return on && n >= 64; }

// ---- which iterative route a call attempts, and the rests (one state per thread)
// A route that failed is not asked again for kRestCalls calls.  The Smith rest is counted first and the ADI rest only on calls whose
// Smith rest has run out: after one call in which both failed, Bartels-Stewart answers 30 calls, then Smith is tried on every call
// while the ADI rest counts down -- and if Smith keeps failing, each of those is followed by another 30 calls of Bartels-Stewart.
constexpr int kRestCalls = 30;
struct Rests {
    int adi = 0, smith = 0;
    void set(int calls) { adi = smith = calls > 0 ? calls : 0; }
};
enum class Route { Adi, Smith, Schur, Done };
enum class Outcome { Solved, Failed, NotApplicable }; // NotApplicable: the problem is not of the route's kind -- nothing is held against the route

// The first route of a call of n rows that the symmetric route did not answer (a call it answered never gets here).  Calls that do not
// pass iterative_gate leave the rests alone.
inline Route first_route(Rests &r, int n, bool on)
{
    if (!iterative_gate(n, on)) return Route::Schur;
    if (r.smith > 0) {
        --r.smith;
        return Route::Schur;
    }
    if (r.adi > 0) {
        --r.adi;
        return Route::Smith;
    }
    return Route::Adi;
}
// The route after `tried` (Adi or Smith) ended with `o`; Done = the call has its answer.
inline Route next_route(Rests &r, Route tried, Outcome o)
{
    if (o == Outcome::Solved) return Route::Done;
    if (tried == Route::Adi) {
        if (o == Outcome::Failed) r.adi = kRestCalls;
        return Route::Smith;
    }
    r.smith = kRestCalls;
    return Route::Schur;
}

// ---- the factored ADI route: building on the call before
// What a successful call keeps beside its matrix and its shifted operators.
struct AdiKept {
    int n = 0, L = 0;            // rows, number of shifts
    bool tr = false;             // the form of the equation
    bool explicit_form = false;  // the operators are kept as inverses (not as LU factors)
    double a = 0.0, b = 0.0;     // the extent of the spectrum the shifts were chosen for
    std::vector<double> shift;
};
// May a call (form tr, n rows, operators in the form explicit_steps) extend what was kept?  By shape only: the caller then compares the
// leading block.  allowed: switch on and not the from-scratch retry; can_extend: the library has what the bordered update needs.
inline bool inherit_shape(const AdiKept &k, bool allowed, bool can_extend, bool tr, int n, bool explicit_steps)
{
    return allowed && can_extend && k.n >= 32 && k.tr == tr && n >= k.n && n - k.n <= 64 && k.L >= 1 && k.explicit_form == explicit_steps;
}
// Do shifts chosen for [a, b] still cover a spectrum now measured as [a_now, b_now]?  (After a restart it widens quickly as the space
// grows: shifts chosen for [9.5, 19] took 32 terms, then did not converge at all, on a matrix whose spectrum had reached [1.3, 20].)
inline bool shifts_still_cover(double a, double b, double a_now, double b_now) { return a_now >= 0.8 * a && b_now <= 1.15 * b; }

// ---- Wachspress' optimal real ADI parameters for [a, b]
// With L = 2^s of them one sweep damps every mode by rho_L ~ 4 exp(-pi^2 L / ln(4 b/a)).  A factorisation costs about four 16-column
// solves, so L is the power of two (at most 8) with the smallest 4 L + (terms needed for 1e-8.5 in Z, i.e. 1e-17 in X).
// 0: the spectrum is spread too far (b/a > 1e5) for this route.
inline int wachspress_count(double a, double b)
{
    if (b / a > 1e5) return 0;
    const double kappa = b / a, pi = 3.14159265358979323846;
    double best_cost = 1e300;
    int L = 1;
    for (int cand = 1; cand <= 8; cand *= 2) {
        double rho = cand == 1 ? (std::sqrt(kappa) - 1.0) / (std::sqrt(kappa) + 1.0) : std::min(0.999, 4.0 * std::exp(-pi * pi * cand / std::log(4.0 * kappa)));
        double sweeps = std::ceil(std::log(3e-9) / std::log(std::max(rho, 1e-300)));
        double cost = 4.0 * cand + cand * std::max(1.0, sweeps);
        if (cost < best_cost) best_cost = cost, L = cand;
    }
    return L;
}
// The L parameters, ascending: the 2L parameters of [a, b] follow from the L parameters x of [sqrt(ab), (a+b)/2] as x +- sqrt(x^2 - ab).
inline std::vector<double> wachspress_shifts(double a, double b, int L)
{
    // intervals down the recursion, then the parameters back up
    std::vector<std::pair<double, double>> iv(1, std::make_pair(a, b));
    for (int l = L; l > 1; l /= 2) iv.push_back(std::make_pair(std::sqrt(iv.back().first * iv.back().second), 0.5 * (iv.back().first + iv.back().second)));
    std::vector<double> shift(1, std::sqrt(iv.back().first * iv.back().second));
    for (int lev = (int)iv.size() - 2; lev >= 0; --lev) {
        const double ab = iv[lev].first * iv[lev].second;
        std::vector<double> up;
        for (double x : shift) {
            const double d = std::sqrt(std::max(0.0, x * x - ab));
            up.push_back(x + d);
            up.push_back(x - d);
        }
        shift.swap(up);
    }
    std::sort(shift.begin(), shift.end());
    return shift;
}
// The term loop's limits: terms, and columns of Z (n rows).
inline int max_terms(int L) { return std::max(64, 16 * L); }
inline int max_cols(int n) { return 8 * n; }

} // namespace lyap
