// The scalar step of the iterative A^-1 operator (rails_amd/csrc/iter_scalars.h) alone, on the host: no HIP, no library.  Built by
// rails_amd/csrc/Makefile into rails_amd/lib/iter_scalars_host, run by tests/test_iter_scalars_host.py.  Prints ALL PASSED at the end.
#include <cmath>
#include <cstdio>
#include <limits>

#include "iter_scalars.h"

static int failed = 0, checks = 0;
#define CHECK(cond)                                                                                                                            \
    do {                                                                                                                                       \
        ++checks;                                                                                                                              \
        if (!(cond)) {                                                                                                                         \
            ++failed;                                                                                                                          \
            std::printf("line %d: %s\n", __LINE__, #cond);                                                                                     \
        }                                                                                                                                      \
    } while (0)

static bool zero_coefficients(const rails_iter_col &c) { return c.alpha == 0.0 && c.beta == 0.0 && c.omega == 0.0; }
static bool stopped_with(const rails_iter_col &c, int flag) { return c.flags == flag; }

int main()
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const double tol2 = 1e-20;
    rails_iter_col c;

    // the finite test
    CHECK(rails_iter_finite(0.0) && rails_iter_finite(-3.5) && rails_iter_finite(1e308));
    CHECK(!rails_iter_finite(nan) && !rails_iter_finite(inf) && !rails_iter_finite(-inf));

    // start: an ordinary column, a zero right-hand side, NaN, no iterations allowed, r.z = 0
    rails_iter_start(c, 4.0, -2.0, 100);
    CHECK(c.flags == RAILS_ITER_ACTIVE && c.rho == -2.0 && c.bb == 4.0 && c.rr == 4.0 && c.iter == 0 && zero_coefficients(c));
    rails_iter_start(c, 0.0, 0.0, 100);
    CHECK(stopped_with(c, RAILS_ITER_CONVERGED) && c.iter == 0 && zero_coefficients(c));
    rails_iter_start(c, nan, 1.0, 100);
    CHECK(stopped_with(c, RAILS_ITER_NONFINITE) && zero_coefficients(c));
    rails_iter_start(c, inf, inf, 100);
    CHECK(stopped_with(c, RAILS_ITER_NONFINITE));
    rails_iter_start(c, 1.0, nan, 100);
    CHECK(stopped_with(c, RAILS_ITER_NONFINITE));
    rails_iter_start(c, 1.0, 1.0, 0);
    CHECK(stopped_with(c, RAILS_ITER_MAXIT) && c.iter == 0);
    rails_iter_start(c, 1.0, 0.0, 10);
    CHECK(stopped_with(c, RAILS_ITER_BREAKDOWN));

    // CG alpha: both signs of a definite operator, a zero and a sign-changing denominator, NaN
    rails_iter_start(c, 4.0, 4.0, 100);
    rails_iter_cg_alpha(c, 8.0, 1.0);
    CHECK(c.flags == RAILS_ITER_ACTIVE && c.alpha == 0.5);
    rails_iter_start(c, 4.0, -4.0, 100); // Jacobi on a negative definite operator: rho and p.q both negative
    rails_iter_cg_alpha(c, -8.0, 1.0);
    CHECK(c.flags == RAILS_ITER_ACTIVE && c.alpha == 0.5);
    rails_iter_start(c, 4.0, 4.0, 100); // no preconditioner, negative definite: rho = r.r > 0, p.q < 0, sign -1
    rails_iter_cg_alpha(c, -8.0, -1.0);
    CHECK(c.flags == RAILS_ITER_ACTIVE && c.alpha == -0.5);
    rails_iter_start(c, 4.0, 4.0, 100);
    rails_iter_cg_alpha(c, 0.0, 1.0);
    CHECK(stopped_with(c, RAILS_ITER_BREAKDOWN) && c.iter == 1 && zero_coefficients(c));
    rails_iter_start(c, 4.0, 4.0, 100);
    rails_iter_cg_alpha(c, -1.0, 1.0);
    CHECK(stopped_with(c, RAILS_ITER_BREAKDOWN) && c.iter == 1 && zero_coefficients(c));
    rails_iter_start(c, 4.0, 4.0, 100);
    rails_iter_cg_alpha(c, 1.0, -1.0);
    CHECK(stopped_with(c, RAILS_ITER_BREAKDOWN));
    rails_iter_start(c, 4.0, 4.0, 100);
    rails_iter_cg_alpha(c, nan, 1.0);
    CHECK(stopped_with(c, RAILS_ITER_NONFINITE) && zero_coefficients(c));

    // CG beta: continue, freeze exactly at the tolerance, just above it, the cap, NaN
    rails_iter_start(c, 4.0, 4.0, 100);
    rails_iter_cg_alpha(c, 8.0, 1.0);
    rails_iter_cg_beta(c, 1.0, 1.0, tol2, 100);
    CHECK(c.flags == RAILS_ITER_ACTIVE && c.beta == 0.25 && c.rho == 1.0 && c.iter == 1 && c.rr == 1.0);
    rails_iter_cg_alpha(c, 2.0, 1.0);
    rails_iter_cg_beta(c, 1e-21, 4.0 * tol2, tol2, 100); // r.r == tol^2 b.b: converged
    CHECK(stopped_with(c, RAILS_ITER_CONVERGED) && c.iter == 2 && zero_coefficients(c));
    rails_iter_start(c, 4.0, 4.0, 100);
    rails_iter_cg_alpha(c, 8.0, 1.0);
    rails_iter_cg_beta(c, 1e-21, std::nextafter(4.0 * tol2, 1.0), tol2, 100);
    CHECK(c.flags == RAILS_ITER_ACTIVE);
    rails_iter_start(c, 4.0, 4.0, 2);
    rails_iter_cg_alpha(c, 8.0, 1.0);
    rails_iter_cg_beta(c, 1.0, 1.0, tol2, 2);
    CHECK(c.flags == RAILS_ITER_ACTIVE);
    rails_iter_cg_alpha(c, 8.0, 1.0);
    rails_iter_cg_beta(c, 0.5, 0.5, tol2, 2);
    CHECK(stopped_with(c, RAILS_ITER_MAXIT) && c.iter == 2 && zero_coefficients(c) && c.rr == 0.5);
    rails_iter_start(c, 4.0, 4.0, 100);
    rails_iter_cg_alpha(c, 8.0, 1.0);
    rails_iter_cg_beta(c, 1.0, nan, tol2, 100);
    CHECK(stopped_with(c, RAILS_ITER_NONFINITE) && zero_coefficients(c));
    rails_iter_start(c, 4.0, 4.0, 100);
    rails_iter_cg_alpha(c, 8.0, 1.0);
    rails_iter_cg_beta(c, 0.0, 1.0, tol2, 100);
    CHECK(stopped_with(c, RAILS_ITER_BREAKDOWN));

    // a frozen column gets exactly zero coefficients from every later step and keeps its count, its residual and its flag
    rails_iter_start(c, 4.0, 4.0, 100);
    rails_iter_cg_alpha(c, 8.0, 1.0);
    rails_iter_cg_beta(c, 0.0, 0.0, tol2, 100);
    CHECK(stopped_with(c, RAILS_ITER_CONVERGED) && c.iter == 1);
    for (int k = 0; k < 3; ++k) {
        c.alpha = c.beta = c.omega = 7.0; // whatever was there
        rails_iter_cg_alpha(c, 3.0, 1.0);
        CHECK(zero_coefficients(c));
        c.alpha = c.beta = c.omega = 7.0;
        rails_iter_cg_beta(c, 3.0, 3.0, tol2, 100);
        CHECK(zero_coefficients(c) && stopped_with(c, RAILS_ITER_CONVERGED) && c.iter == 1 && c.rr == 0.0);
        c.alpha = c.beta = c.omega = 7.0;
        rails_iter_bi_alpha(c, 3.0);
        CHECK(zero_coefficients(c));
        c.alpha = c.beta = c.omega = 7.0;
        rails_iter_bi_omega(c, 3.0, 3.0);
        CHECK(zero_coefficients(c));
        c.alpha = c.beta = c.omega = 7.0;
        rails_iter_bi_end(c, nan, nan, tol2, 100);
        CHECK(zero_coefficients(c) && stopped_with(c, RAILS_ITER_CONVERGED) && c.iter == 1);
    }

    // BiCGStab: one full iteration, then each zero denominator
    rails_iter_start(c, 4.0, 4.0, 100);
    rails_iter_bi_alpha(c, 8.0);
    CHECK(c.flags == RAILS_ITER_ACTIVE && c.alpha == 0.5);
    rails_iter_bi_omega(c, 3.0, 6.0);
    CHECK(c.flags == RAILS_ITER_ACTIVE && c.omega == 0.5);
    rails_iter_bi_end(c, 2.0, 1.0, tol2, 100);
    CHECK(c.flags == RAILS_ITER_ACTIVE && c.beta == 0.5 && c.rho == 2.0 && c.iter == 1 && c.rr == 1.0);
    rails_iter_start(c, 4.0, 4.0, 100);
    rails_iter_bi_alpha(c, 0.0); // r^.v = 0
    CHECK(stopped_with(c, RAILS_ITER_BREAKDOWN) && c.iter == 1 && zero_coefficients(c));
    rails_iter_start(c, 4.0, 4.0, 100);
    rails_iter_bi_alpha(c, 8.0);
    rails_iter_bi_omega(c, 0.0, 0.0); // t.t = 0: decided at the end of the iteration
    CHECK((c.flags & RAILS_ITER_ACTIVE) && (c.flags & RAILS_ITER_PENDING) && c.omega == 0.0 && c.alpha == 0.5);
    rails_iter_bi_end(c, 1.0, 1.0, tol2, 100);
    CHECK(stopped_with(c, RAILS_ITER_BREAKDOWN) && c.iter == 1 && zero_coefficients(c));
    rails_iter_start(c, 4.0, 4.0, 100);
    rails_iter_bi_alpha(c, 8.0);
    rails_iter_bi_omega(c, 0.0, 0.0); // ... and the half step was the solution: converged, not broken down
    rails_iter_bi_end(c, 0.0, 0.0, tol2, 100);
    CHECK(stopped_with(c, RAILS_ITER_CONVERGED) && c.iter == 1);
    rails_iter_start(c, 4.0, 4.0, 100);
    rails_iter_bi_alpha(c, 8.0);
    rails_iter_bi_omega(c, 3.0, 6.0);
    rails_iter_bi_end(c, 0.0, 1.0, tol2, 100); // r^.r = 0
    CHECK(stopped_with(c, RAILS_ITER_BREAKDOWN));
    rails_iter_start(c, 4.0, 4.0, 100);
    rails_iter_bi_alpha(c, 8.0);
    rails_iter_bi_omega(c, 0.0, 6.0); // t.s = 0: omega = 0, the next beta would divide by it
    rails_iter_bi_end(c, 1.0, 1.0, tol2, 100);
    CHECK(stopped_with(c, RAILS_ITER_BREAKDOWN));
    rails_iter_start(c, 4.0, 4.0, 100);
    rails_iter_bi_alpha(c, nan);
    CHECK(stopped_with(c, RAILS_ITER_NONFINITE));
    rails_iter_start(c, 4.0, 4.0, 100);
    rails_iter_bi_alpha(c, 8.0);
    rails_iter_bi_omega(c, inf, 1.0);
    CHECK(stopped_with(c, RAILS_ITER_NONFINITE) && zero_coefficients(c));
    rails_iter_start(c, 4.0, 4.0, 1);
    rails_iter_bi_alpha(c, 8.0);
    rails_iter_bi_omega(c, 3.0, 6.0);
    rails_iter_bi_end(c, 2.0, 1.0, tol2, 1); // the cap
    CHECK(stopped_with(c, RAILS_ITER_MAXIT) && c.iter == 1 && zero_coefficients(c));
    rails_iter_start(c, 4.0, 4.0, 1);
    rails_iter_bi_alpha(c, 8.0);
    rails_iter_bi_omega(c, 3.0, 6.0);
    rails_iter_bi_end(c, 2.0, 4.0 * tol2, tol2, 1); // convergence wins over the cap
    CHECK(stopped_with(c, RAILS_ITER_CONVERGED));

    std::printf("%d checks, %d failed\n", checks, failed);
    std::printf(failed ? "FAILED\n" : "ALL PASSED\n");
    return failed ? 1 : 0;
}
