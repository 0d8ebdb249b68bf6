// What the projected Lyapunov solve decides without computing (rails_amd/csrc/lyap_route.h: the gates of the routes, which iterative route
// a call attempts and how long a failed one rests, whether the factored ADI route may build on the call before, Wachspress' shifts) alone,
// on the host: no HIP, no library, no LAPACK.  Built by rails_amd/csrc/Makefile into rails_amd/lib/lyap_route_host, run by
// tests/test_lyap_route_host.py (which also builds it once more, as host code, under the address and undefined-behaviour sanitizers).
// Prints ALL PASSED at the end.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "lyap_route.h"

using namespace lyap;

static int failed = 0, checks = 0;
static long long at = 0; // where in a loop a check failed
static double ratio = 0.0;
#define CHECK(cond)                                                                                                                            \
    do {                                                                                                                                       \
        ++checks;                                                                                                                              \
        if (!(cond)) {                                                                                                                         \
            ++failed;                                                                                                                          \
            if (failed <= 20) std::printf("line %d (at %lld, b/a %g): %s\n", __LINE__, at, ratio, #cond);                                      \
        }                                                                                                                                      \
    } while (0)

// ---- the rests.  The rule as it stood inside rails_sb03md (one expression with comma operators, on two per-thread counters), written
// out as statements: what a call attempted, whether an iterative route answered, and the counters afterwards.
struct OldRule {
    int smith_pause = 0, lowrank_pause = 0;
};
struct Attempts {
    bool adi = false, smith = false, iterative_answer = false;
    bool operator==(const Attempts &o) const { return adi == o.adi && smith == o.smith && iterative_answer == o.iterative_answer; }
};
enum What { ADI_OK, ADI_NA_SMITH_OK, ADI_FAILS_SMITH_OK, ADI_NA_BOTH_FAIL, BOTH_FAIL }; // what the routes would say if asked
static Attempts old_call(OldRule &s, int n, bool on, What w)
{
    Attempts t;
    if (!(on && n >= 32)) return t;
    if (s.smith_pause > 0) {
        --s.smith_pause;
        return t;
    }
    bool ok = false;
    if (s.lowrank_pause > 0)
        --s.lowrank_pause;
    else {
        t.adi = true;
        ok = w == ADI_OK;
        if (!ok) s.lowrank_pause = (w == ADI_NA_SMITH_OK || w == ADI_NA_BOTH_FAIL) ? 0 : 30;
    }
    if (!ok) {
        t.smith = true;
        ok = w == ADI_NA_SMITH_OK || w == ADI_FAILS_SMITH_OK || w == ADI_OK; // (Smith takes what ADI takes)
    }
    if (ok)
        t.iterative_answer = true;
    else
        s.smith_pause = 30;
    return t;
}
// ... and a call as rails_sb03md makes it with the header
static Attempts new_call(Rests &r, int n, bool on, What w)
{
    Attempts t;
    Route route = first_route(r, n, on);
    while (route == Route::Adi || route == Route::Smith) {
        Outcome o;
        if (route == Route::Adi) {
            t.adi = true;
            o = w == ADI_OK ? Outcome::Solved : (w == ADI_NA_SMITH_OK || w == ADI_NA_BOTH_FAIL) ? Outcome::NotApplicable : Outcome::Failed;
        } else {
            t.smith = true;
            o = (w == ADI_NA_BOTH_FAIL || w == BOTH_FAIL) ? Outcome::Failed : Outcome::Solved;
        }
        route = next_route(r, route, o);
    }
    t.iterative_answer = route == Route::Done;
    CHECK(route == Route::Done || route == Route::Schur);
    return t;
}

static void test_rests()
{
    // at least 1000 double failures in a row: both are tried at call 0; then Bartels-Stewart answers 30 calls and Smith is tried on the
    // 31st, again and again, and the ADI rest is counted down only on those calls: ADI is next tried at call 31 * 31 = 961, not at call 31
    {
        Rests r;
        OldRule s;
        for (at = 0; at < 1100; ++at) {
            const Attempts t = new_call(r, 96, true, BOTH_FAIL);
            CHECK(t == old_call(s, 96, true, BOTH_FAIL));
            CHECK(t.smith == (at % 31 == 0));
            CHECK(t.adi == (at == 0 || at == 961));
            CHECK(!t.iterative_answer);
            CHECK(r.smith == 30 - (int)(at % 31));
            CHECK(r.adi == (at < 961 ? 30 - (int)(at / 31) : 30 - (int)((at - 961) / 31)));
            CHECK(r.adi == s.lowrank_pause && r.smith == s.smith_pause);
        }
    }
    // ADI fails, Smith answers: Smith is asked 30 more times, then ADI again
    {
        Rests r;
        for (at = 0; at < 70; ++at) {
            const Attempts t = new_call(r, 32, true, ADI_FAILS_SMITH_OK);
            CHECK(t.smith && t.iterative_answer && t.adi == (at % 31 == 0) && r.smith == 0 && r.adi == 30 - (int)(at % 31));
        }
    }
    // "not applicable" never rests ADI, whether Smith answers or not
    {
        Rests r;
        for (at = 0; at < 40; ++at) {
            const Attempts t = new_call(r, 64, true, ADI_NA_SMITH_OK);
            CHECK(t.adi && t.smith && t.iterative_answer && r.adi == 0 && r.smith == 0);
        }
        for (at = 0; at < 70; ++at) {
            const Attempts t = new_call(r, 64, true, ADI_NA_BOTH_FAIL);
            CHECK(t.adi == (at % 31 == 0) && t.smith == t.adi && !t.iterative_answer && r.adi == 0 && r.smith == 30 - (int)(at % 31));
        }
    }
    // set_pause: both counters; 0 and below clear them
    {
        Rests r;
        r.set(5);
        CHECK(r.adi == 5 && r.smith == 5);
        for (at = 0; at < 12; ++at) { // 5 calls of Bartels-Stewart, 5 of Smith alone, then ADI
            const Attempts t = new_call(r, 80, true, ADI_OK);
            CHECK(t.adi == (at >= 10) && t.smith == (at >= 5 && at < 10) && t.iterative_answer == (at >= 5));
        }
        new_call(r, 80, true, BOTH_FAIL);
        CHECK(r.adi == 30 && r.smith == 30);
        r.set(0);
        CHECK(r.adi == 0 && r.smith == 0);
        CHECK(new_call(r, 80, true, ADI_OK).adi);
        r.set(7);
        r.set(-3);
        CHECK(r.adi == 0 && r.smith == 0);
    }
    // calls below 32 rows, calls with the switch off (and calls the symmetric route answered: they never ask) leave the state alone
    {
        Rests r;
        r.adi = 3, r.smith = 2;
        at = 0;
        CHECK(first_route(r, 31, true) == Route::Schur && r.adi == 3 && r.smith == 2);
        CHECK(first_route(r, 500, false) == Route::Schur && r.adi == 3 && r.smith == 2);
        CHECK(first_route(r, 32, true) == Route::Schur && r.adi == 3 && r.smith == 1);
        CHECK(first_route(r, 1, true) == Route::Schur && r.adi == 3 && r.smith == 1);
        CHECK(first_route(r, 32, true) == Route::Schur && r.adi == 3 && r.smith == 0);
        CHECK(first_route(r, 32, true) == Route::Smith && r.adi == 2 && r.smith == 0);
    }
    // any sequence: outcomes, sizes and set_pause from a fixed generator, against the rule as it stood
    {
        Rests r;
        OldRule s;
        uint64_t x = 88172645463325252ull;
        for (at = 0; at < 200000; ++at) {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;
            const What w = (x >> 20) % 100 < 70 ? BOTH_FAIL : (What)((x >> 8) % 5);
            const int n = (x >> 40) % 16 == 0 ? 31 : 32 + (int)((x >> 44) % 200);
            if ((x >> 30) % 997 == 0) {
                const int calls = (int)((x >> 50) % 9) - 2;
                r.set(calls);
                s.smith_pause = s.lowrank_pause = calls > 0 ? calls : 0;
            }
            CHECK(new_call(r, n, true, w) == old_call(s, n, true, w));
            CHECK(r.adi == s.lowrank_pause && r.smith == s.smith_pause);
        }
    }
}

static void test_gates()
{
    at = 0;
    CHECK(!symmetry_is_measured(7, true) && symmetry_is_measured(8, true) && !symmetry_is_measured(8, false) && !symmetry_is_measured(300, false));
    CHECK(symmetric_to_rounding(1e-13, 1.0) && !symmetric_to_rounding(1.0000001e-13, 1.0) && symmetric_to_rounding(0.0, 5.0) && !symmetric_to_rounding(0.0, 0.0));
    CHECK(symmetric_to_rounding(3e-13, 4.0) && !symmetric_to_rounding(5e-13, 4.0));
    CHECK(!iterative_gate(31, true) && iterative_gate(32, true) && !iterative_gate(32, false) && !iterative_gate(1000, false));
    CHECK(!blocked_sylvester_gate(63, true) && blocked_sylvester_gate(64, true) && !blocked_sylvester_gate(64, false));
    CHECK(!explicit_steps_gate(63, true) && explicit_steps_gate(64, true) && !explicit_steps_gate(64, false));
    CHECK(kRestCalls == 30);
}

static void test_inheritance()
{
    at = 0;
    AdiKept k;
    CHECK(!inherit_shape(k, true, true, false, 100, true) && !inherit_shape(k, true, true, false, 0, false)); // nothing kept yet
    k.n = 100, k.L = 2, k.tr = true, k.explicit_form = true;
    CHECK(inherit_shape(k, true, true, true, 100, true));  // the same size again
    CHECK(inherit_shape(k, true, true, true, 116, true));
    CHECK(inherit_shape(k, true, true, true, 164, true));  // a border of 64 rows
    CHECK(!inherit_shape(k, true, true, true, 165, true)); // ... of 65
    CHECK(!inherit_shape(k, true, true, false, 116, true)); // the other trans
    CHECK(!inherit_shape(k, true, true, true, 99, true));   // a smaller matrix
    CHECK(!inherit_shape(k, true, true, true, 116, false)); // kept as inverses, wanted as LU factors
    CHECK(!inherit_shape(k, false, true, true, 116, true)); // switched off, or the retry from scratch
    CHECK(!inherit_shape(k, true, false, true, 116, true)); // a library without dlaswp / dtrsm
    k.L = 0;
    CHECK(!inherit_shape(k, true, true, true, 116, true));
    k.L = 1, k.explicit_form = false, k.tr = false;
    k.n = 31;
    CHECK(!inherit_shape(k, true, true, false, 40, false)); // kept from a call below 32 rows
    k.n = 32;
    CHECK(inherit_shape(k, true, true, false, 40, false));
    CHECK(!inherit_shape(k, true, true, false, 64, true)); // kept as LU factors, wanted as inverses (48 -> 64)
    // the inherited shifts cover a spectrum that has moved a little
    CHECK(shifts_still_cover(2.0, 10.0, 2.0, 10.0) && shifts_still_cover(2.0, 10.0, 1.6, 11.5) && shifts_still_cover(2.0, 10.0, 5.0, 6.0));
    CHECK(!shifts_still_cover(2.0, 10.0, 1.59, 10.0) && !shifts_still_cover(2.0, 10.0, 2.0, 11.51) && !shifts_still_cover(9.5, 19.0, 1.3, 20.0));
    CHECK(!shifts_still_cover(2.0, 10.0, NAN, 10.0) && !shifts_still_cover(2.0, 10.0, 2.0, NAN));
    CHECK(max_terms(1) == 64 && max_terms(4) == 64 && max_terms(8) == 128 && max_cols(200) == 1600);
}

// The same recursion in long double, and with it a first-order bound *err on the relative error of the parameters computed in double.
// x - sqrt(x^2 - ab) is ill-conditioned where x^2 is close to ab (narrow intervals, the lower levels of many shifts on a small b/a) and
// where the root is close to x (a large b/a), and a level hands its error to the one above; with eps = 2^-52, E the bound so far:
//   the ends of the interval at depth k carry at most k eps each (a root of a product, a mean), the single parameter below them (k + 1) eps;
//   s = x^2 - ab is off by at most sigma x^2, sigma = 2 E + (2 k + 1.5) eps (ab <= x^2);  d = sqrt(s) by sigma x^2 / (2 d) + eps d / 2;
//   p = x -+ d by E x + sigma x^2 / (2 d) + eps d / 2 + eps p / 2, the largest relative to p for p = x - d.
// Where s is not well above sigma x^2 the bound does not hold to first order: *err is infinite there (nothing is asserted).
static std::vector<long double> shifts_long(long double a, long double b, int L, long double *err)
{
    const long double eps = DBL_EPSILON;
    std::vector<std::pair<long double, long double>> iv(1, std::make_pair(a, b));
    for (int l = L; l > 1; l /= 2) iv.push_back(std::make_pair(sqrtl(iv.back().first * iv.back().second), 0.5L * (iv.back().first + iv.back().second)));
    std::vector<long double> p(1, sqrtl(iv.back().first * iv.back().second));
    long double E = (long double)iv.size() * eps;
    for (int lev = (int)iv.size() - 2; lev >= 0; --lev) {
        std::vector<long double> up;
        long double E_up = 0.0L;
        const long double sigma = 2.0L * E + (2.0L * lev + 1.5L) * eps;
        for (long double x : p) {
            const long double s = x * x - iv[lev].first * iv[lev].second, d = sqrtl(std::max(0.0L, s));
            up.push_back(x + d);
            up.push_back(x - d);
            E_up = std::max(E_up, s > 16.0L * sigma * x * x ? (E * x + sigma * x * x / (2.0L * d) + 0.5L * eps * d) / (x - d) + 0.5L * eps : (long double)INFINITY);
        }
        p.swap(up);
        E = E_up;
    }
    std::sort(p.begin(), p.end());
    *err = E;
    return p;
}

static void test_shifts()
{
    const double eps = DBL_EPSILON;
    double worst_pair = 0.0, worst_pair_rel = 0.0, worst_long = 0.0, worst_long_rel = 0.0;
    int unbounded = 0;
    for (double a : {0.3, 1.0, 7.7, 1.3e-3})
        for (double r : {1.5, 2.0, 3.0, 10.0, 47.0, 100.0, 1e3, 1e4, 9.9e4, 1e5})
            for (int L = 1; L <= 8; L *= 2) {
                const double b = a * r;
                ratio = r, at = L;
                long double err = 0.0L;
                const std::vector<double> p = wachspress_shifts(a, b, L);
                const std::vector<long double> q = shifts_long(a, b, L, &err);
                CHECK((int)p.size() == L && (int)q.size() == L);
                if (L == 1) CHECK(p[0] == std::sqrt(a * b));
                unbounded += std::isinf((double)err);
                for (int i = 0; i < L; ++i) {
                    if (i > 0) CHECK(p[i] > p[i - 1]);
                    CHECK(p[i] >= a && p[i] <= b);
                    // the two of a pair are x + d and x - d with d^2 = fl(x^2 - ab): their product misses ab by the roundings of x^2, ab, the
                    // difference and the root -- a few ulps OF x^2, x = (p_i + p_j) / 2, which is above ab by up to (a + b)^2 / (4 a b)
                    const double x = 0.5 * (p[i] + p[L - 1 - i]), pair = std::fabs(p[i] * p[L - 1 - i] - a * b), pair_allowed = 4.0 * eps * x * x;
                    CHECK(pair <= pair_allowed);
                    worst_pair = std::max(worst_pair, pair / (eps * a * b)), worst_pair_rel = std::max(worst_pair_rel, pair / pair_allowed);
                    const double dl = (double)(fabsl(p[i] - q[i]) / q[i]);
                    CHECK(dl <= 2.0 * (double)err);
                    worst_long = std::max(worst_long, dl / eps);
                    if (!std::isinf((double)err)) worst_long_rel = std::max(worst_long_rel, dl / (2.0 * (double)err));
                }
            }
    std::printf("shifts: |p_i p_(L+1-i) - ab| at most %.1f ulps of ab, %.2f of what 4 ulps of x^2 allow; against long double at most %.3g ulps, %.2f of the bound (%d cases without one)\n",
                worst_pair, worst_pair_rel, worst_long, worst_long_rel, unbounded);
    // the number of shifts against the cost formula, restated: 4 L for the factorisations + L per sweep, sweeps to 3e-9 at the rate
    // rho_1 = (sqrt(k) - 1) / (sqrt(k) + 1), rho_L = 4 exp(-pi^2 L / ln(4 k)); the first of equal costs wins
    int seen[9] = {0};
    for (int g = 0; g <= 4000; ++g) {
        const double a = 0.7, b = a * std::pow(10.0, 0.002 + 4.997 * g / 4000.0), kappa = b / a;
        ratio = kappa, at = g;
        int want = 0;
        double best = 0.0;
        for (int cand = 1; cand <= 8; cand *= 2) {
            const double rho = cand == 1 ? (std::sqrt(kappa) - 1.0) / (std::sqrt(kappa) + 1.0) : std::min(0.999, 4.0 * std::exp(-M_PI * M_PI * cand / std::log(4.0 * kappa)));
            const double cost = 4.0 * cand + cand * std::max(1.0, std::ceil(std::log(3e-9) / std::log(std::max(rho, 1e-300))));
            if (want == 0 || cost < best) best = cost, want = cand;
        }
        const int L = wachspress_count(a, b);
        CHECK(b / a <= 1e5 && L == want);
        if (L >= 1 && L <= 8) ++seen[L];
    }
    at = 0;
    CHECK(seen[1] > 0 && seen[2] > 0 && seen[4] > 0); // (the grid meets every count the formula ever picks: below b/a = 1e5 eight shifts never pay)
    CHECK(wachspress_count(1.0, 1e5) >= 1 && wachspress_count(1.0, 1.0000001e5) == 0 && wachspress_count(3.0, 3e7) == 0);
    std::printf("counts over the grid of b/a: L = 1: %d, 2: %d, 4: %d, 8: %d\n", seen[1], seen[2], seen[4], seen[8]);
}

int main()
{
    test_gates();
    test_rests();
    test_inheritance();
    test_shifts();
    std::printf("%d checks, %d failed\n", checks, failed);
    if (!failed) std::printf("ALL PASSED\n");
    return failed ? 1 : 0;
}
