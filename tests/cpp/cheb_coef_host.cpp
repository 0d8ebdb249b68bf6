// The arithmetic of the Chebyshev polynomial preconditioner (rails_amd/csrc/cheb_coef.h) alone, on the host: no HIP, no library.  Built
// by rails_amd/csrc/Makefile into rails_amd/lib/cheb_coef_host, run by tests/test_cheb_coef_host.py (which also builds it once more, as
// host code, under the address and undefined-behaviour sanitizers).  Prints ALL PASSED at the end.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "cheb_coef.h"

static int failed = 0, checks = 0;
#define CHECK(cond)                                                                                                                            \
    do {                                                                                                                                       \
        ++checks;                                                                                                                              \
        if (!(cond)) {                                                                                                                         \
            ++failed;                                                                                                                          \
            std::printf("line %d: %s\n", __LINE__, #cond);                                                                                     \
        }                                                                                                                                      \
    } while (0)

typedef long double ld;

// T_n(x) for any real x by the three-term recurrence
static ld cheb_t(int n, ld x)
{
    ld t0 = 1.0L, t1 = x;
    if (n == 0) return t0;
    for (int k = 1; k < n; ++k) {
        const ld t2 = 2.0L * x * t1 - t0;
        t0 = t1;
        t1 = t2;
    }
    return t1;
}

// the scalar form of the application: z = p_K(lambda) r for r = 1 with the coefficients given; returns the residual 1 - lambda z
static ld scalar_residual(ld lambda, ld theta, int K, const double *a, const double *b)
{
    ld d = 1.0L / theta, z = d;
    for (int k = 0; k < K; ++k) {
        d = (ld)a[k] * d + (ld)b[k] * (1.0L - lambda * z);
        z += d;
    }
    return 1.0L - lambda * z;
}

int main()
{
    const double eps = std::numeric_limits<double>::epsilon();
    const double intervals[][2] = {{0.0625, 2.0}, {0.02, 2.0}, {1.0, 30.0}, {0.19, 1.9}, {7.9 / 4.0, 7.9}};
    for (const auto &iv : intervals) {
        const double lo = iv[0], hi = iv[1];
        for (int K : {0, 1, 2, 4, 5, 8, 64}) {
            double theta = 0.0, a[RAILS_CHEB_MAX_DEGREE], b[RAILS_CHEB_MAX_DEGREE];
            CHECK(rails_cheb_coef(lo, hi, K, &theta, a, b));
            // the coefficients against a long double evaluation of the same recurrence
            const ld th = ((ld)hi + (ld)lo) / 2, delta = ((ld)hi - (ld)lo) / 2, sigma = th / delta;
            CHECK(std::fabs((double)(th - theta)) <= eps * (double)th);
            ld rho = 1.0L / sigma;
            for (int k = 0; k < K; ++k) {
                const ld next = 1.0L / (2.0L * sigma - rho);
                CHECK(std::fabs((double)(next * rho - a[k])) <= 8 * eps * (double)(next * rho));
                CHECK(std::fabs((double)(2.0L * next / delta - b[k])) <= 8 * eps * (double)(2.0L * next / delta));
                // rho_k = T_k(sigma) / T_{k+1}(sigma)
                CHECK(std::fabs((double)(next - cheb_t(k + 1, sigma) / cheb_t(k + 2, sigma))) <= 64 * eps * (double)next);
                rho = next;
            }
            if (K > 8) continue; // (the closed form below loses its digits to T_65(sigma) ~ 1e30 long before the recurrence does)
            // the residual polynomial is T_{K+1}((theta - lambda) / delta) / T_{K+1}(sigma) on a grid of [lo, hi], ends included
            const ld tk = cheb_t(K + 1, sigma);
            for (int i = 0; i <= 64; ++i) {
                const ld lambda = (ld)lo + ((ld)hi - (ld)lo) * i / 64;
                const ld want = cheb_t(K + 1, (th - lambda) / delta) / tk;
                const ld got = scalar_residual(lambda, th, K, a, b);
                CHECK(std::fabs((double)(got - want)) <= 1e-12);
                CHECK(std::fabs((double)got) <= (double)(1.0L / tk) * (1 + 1e-10) + 1e-13);
            }
            // positive and below 1 on (0, lo): p_K(lambda) lambda lies in (0, 1) there, the preconditioner is definite
            for (int i = 1; i < 64; ++i) {
                const ld lambda = (ld)lo * i / 64;
                const ld got = scalar_residual(lambda, th, K, a, b);
                CHECK(got > 0.0L && got < 1.0L);
            }
        }
    }
    // refusals: an empty or reversed interval, a lower end that is not positive, a non-finite end, a degree outside 0 .. 64
    {
        double theta, a[RAILS_CHEB_MAX_DEGREE + 1], b[RAILS_CHEB_MAX_DEGREE + 1];
        const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
        CHECK(!rails_cheb_coef(1.0, 1.0, 2, &theta, a, b));
        CHECK(!rails_cheb_coef(2.0, 1.0, 2, &theta, a, b));
        CHECK(!rails_cheb_coef(0.0, 1.0, 2, &theta, a, b));
        CHECK(!rails_cheb_coef(-1.0, 1.0, 2, &theta, a, b));
        CHECK(!rails_cheb_coef(1.0, inf, 2, &theta, a, b));
        CHECK(!rails_cheb_coef(nan, 1.0, 2, &theta, a, b));
        CHECK(!rails_cheb_coef(1.0, nan, 2, &theta, a, b));
        CHECK(!rails_cheb_coef(0.5, 1.0, -1, &theta, a, b));
        CHECK(!rails_cheb_coef(0.5, 1.0, RAILS_CHEB_MAX_DEGREE + 1, &theta, a, b));
        CHECK(rails_cheb_coef(0.5, 1.0, RAILS_CHEB_MAX_DEGREE, &theta, a, b));
    }

    // the Gershgorin bound: the 1-D Laplacian of either sign (rows 2 1 / 1 2 1 / 1 2), then a matrix with an uneven diagonal
    {
        const std::vector<int64_t> rowptr = {0, 2, 5, 7};
        const std::vector<double> val = {-2, 1, 1, -2, 1, 1, -2};
        std::vector<double> pos(val);
        for (double &v : pos) v = -v;
        CHECK(rails_cheb_gershgorin(3, rowptr.data(), val.data(), nullptr) == 4.0);
        CHECK(rails_cheb_gershgorin(3, rowptr.data(), pos.data(), nullptr) == 4.0);
        const std::vector<double> g = {-0.5, -0.5, -0.5}, gp = {0.5, 0.5, 0.5}; // the Jacobi diagonal's inverse, either sign
        CHECK(rails_cheb_gershgorin(3, rowptr.data(), val.data(), g.data()) == 2.0);
        CHECK(rails_cheb_gershgorin(3, rowptr.data(), pos.data(), gp.data()) == 2.0);
        // rows (4 -1), (-1 10 -3), (-3 0.5): sums 5, 14, 3.5; with g = 1 / diagonal: 1.25, 1.4, 7
        const std::vector<double> v2 = {4, -1, -1, 10, -3, -3, 0.5}, g2 = {0.25, 0.1, 2.0};
        CHECK(rails_cheb_gershgorin(3, rowptr.data(), v2.data(), nullptr) == 14.0);
        CHECK(rails_cheb_gershgorin(3, rowptr.data(), v2.data(), g2.data()) == 7.0);
        // an empty row, no rows at all, a NaN entry
        const std::vector<int64_t> rp2 = {0, 0, 1};
        const std::vector<double> v3 = {-3.0};
        CHECK(rails_cheb_gershgorin(2, rp2.data(), v3.data(), nullptr) == 3.0);
        CHECK(rails_cheb_gershgorin(0, rp2.data(), v3.data(), nullptr) == 0.0);
        const std::vector<double> v4 = {std::numeric_limits<double>::quiet_NaN()};
        CHECK(std::isnan(rails_cheb_gershgorin(2, rp2.data(), v4.data(), nullptr)));
    }

    // which operators the fused step takes, at the edges of the rule
    {
        const int64_t one = 1;
        CHECK(rails_cheb_fused_eligible(true, 0, 1, 16));
        CHECK(rails_cheb_fused_eligible(true, 0, 4096, 32));
        CHECK(!rails_cheb_fused_eligible(false, 0, 4096, 32)); // a callback, an LU handle, an iterative handle
        CHECK(!rails_cheb_fused_eligible(true, 1, 4096, 32));  // ghost rows
        CHECK(rails_cheb_fused_eligible(true, 0, (one << 24) - 1, 16));
        CHECK(!rails_cheb_fused_eligible(true, 0, one << 24, 16)); // 2^24 rows
        // 4 GiB less the last row's reach: 2^24 - 2 rows of 32 doubles (256 bytes) stay below, one more does not; rows of 512 doubles
        // (4 KiB) get there at 2^20
        CHECK(rails_cheb_fused_eligible(true, 0, (one << 24) - 2, 32));
        CHECK(!rails_cheb_fused_eligible(true, 0, (one << 24) - 1, 32));
        CHECK(rails_cheb_fused_eligible(true, 0, (one << 20) - 1, 512));
        CHECK(!rails_cheb_fused_eligible(true, 0, one << 20, 512));
        CHECK(!rails_cheb_fused_eligible(true, 0, 16, one << 21)); // a row stride beyond the 24-bit multiply
        CHECK(!rails_cheb_fused_eligible(true, 0, 0, 16));
        CHECK(!rails_cheb_fused_eligible(true, 0, 16, 0));
    }

    // the z panel a sweep starts in: following the ping-pong of the steps from there ends in the primary panel (0); unfused steps never
    // leave it
    for (int steps = 0; steps <= 17; ++steps) {
        for (int fused = 0; fused <= 1; ++fused) {
            int at = rails_cheb_start_panel(fused != 0, steps);
            CHECK(at == 0 || at == 1);
            if (!fused) CHECK(at == 0);
            for (int k = 0; k < steps; ++k)
                if (fused) at ^= 1; // a fused step reads one panel and writes the other
            CHECK(at == 0);
        }
    }

    std::printf("%d checks, %d failed\n", checks, failed);
    if (!failed) std::printf("ALL PASSED\n");
    return failed ? 1 : 0;
}
