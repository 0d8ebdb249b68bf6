// iter_scalars.h -- the scalar step of the iterative A^-1 operator (itsolve.hip): per column, the coefficients of the CG and BiCGStab
// recurrences, the guards against dividing by zero, the breakdown rules, the non-finite test, the convergence test and the freeze.
// Plain arithmetic on one column's record: the one-workgroup scalar kernel compiles it for the device, tests/cpp/iter_scalars_host.cpp
// for the host (no HIP, no library), and tests/iter_reference.py restates it in numpy.
//
// A column is ACTIVE until it stops; it stops exactly once, with one of the other flags, and from then on every step gives it
// alpha = beta = omega = 0, so that the update passes leave its x and r as they are whatever is queued after it (the result of a
// solve does not depend on how often the host looks).  `iter` is the iteration in which the column stopped.
#ifndef RAILS_ITER_SCALARS_H
#define RAILS_ITER_SCALARS_H

#include <stdint.h>

#if defined(__HIPCC__)
#define RAILS_ITER_HD __host__ __device__ inline
#else
#define RAILS_ITER_HD inline
#endif

enum {
    RAILS_ITER_ACTIVE = 1,     // still iterating
    RAILS_ITER_CONVERGED = 2,  // r.r <= tol^2 b.b
    RAILS_ITER_MAXIT = 4,      // stopped at max_iterations with its last iterate
    RAILS_ITER_BREAKDOWN = 8,  // a denominator vanished (or, CG, has the wrong sign: the operator is not definite)
    RAILS_ITER_NONFINITE = 16, // an inner product is not finite
    RAILS_ITER_PENDING = 32    // BiCGStab: t.t = 0 in this iteration; breakdown unless the half step already converged
};

struct rails_iter_col {
    double rho, alpha, beta, omega; // rho: r.z (CG), r^.r (BiCGStab)
    double bb, rr;                  // squared norm of b, current squared residual of the recurrence
    int32_t iter, flags;
};

RAILS_ITER_HD bool rails_iter_finite(double x) { return x - x == 0.0; }

RAILS_ITER_HD void rails_iter_freeze(rails_iter_col &c, int flag)
{
    c.flags = (c.flags & ~(RAILS_ITER_ACTIVE | RAILS_ITER_PENDING)) | flag;
    c.alpha = c.beta = c.omega = 0.0;
}

// start of a column: x = 0, r = b; bb = b.b, rho0 = r.z (CG) or r^.r = b.b (BiCGStab)
RAILS_ITER_HD void rails_iter_start(rails_iter_col &c, double bb, double rho0, int max_iterations)
{
    c.rho = rho0;
    c.alpha = c.beta = c.omega = 0.0;
    c.bb = c.rr = bb;
    c.iter = 0;
    c.flags = RAILS_ITER_ACTIVE;
    if (!rails_iter_finite(bb) || !rails_iter_finite(rho0))
        rails_iter_freeze(c, RAILS_ITER_NONFINITE);
    else if (bb == 0.0)
        rails_iter_freeze(c, RAILS_ITER_CONVERGED); // zero right-hand side: x = 0 after 0 iterations
    else if (max_iterations <= 0)
        rails_iter_freeze(c, RAILS_ITER_MAXIT);
    else if (rho0 == 0.0)
        rails_iter_freeze(c, RAILS_ITER_BREAKDOWN);
}

// CG, after p.q: alpha = rho / p.q.  sign: the sign p.q / rho must have, +1 with the Jacobi preconditioner (rho = r.D^-1 r carries the
// sign of a definite operator itself), the sign of the operator's diagonal without it (rho = r.r > 0, p.q = p.Ap < 0 for our
// negative definite Laplacians; the recurrences are the same for (A, b) and (-A, -b)).
RAILS_ITER_HD void rails_iter_cg_alpha(rails_iter_col &c, double pq, double sign)
{
    if (!(c.flags & RAILS_ITER_ACTIVE)) {
        c.alpha = c.beta = c.omega = 0.0;
        return;
    }
    if (!rails_iter_finite(pq)) {
        c.iter++;
        rails_iter_freeze(c, RAILS_ITER_NONFINITE);
    } else if (pq == 0.0 || ((pq > 0.0) != (sign * c.rho > 0.0))) {
        c.iter++;
        rails_iter_freeze(c, RAILS_ITER_BREAKDOWN);
    } else
        c.alpha = c.rho / pq;
}

// CG, after the update: the tests, then beta = r.z_new / r.z_old
RAILS_ITER_HD void rails_iter_cg_beta(rails_iter_col &c, double rz, double rr, double tol2, int max_iterations)
{
    if (!(c.flags & RAILS_ITER_ACTIVE)) {
        c.alpha = c.beta = c.omega = 0.0;
        return;
    }
    c.iter++;
    c.rr = rr;
    if (!rails_iter_finite(rr) || !rails_iter_finite(rz))
        rails_iter_freeze(c, RAILS_ITER_NONFINITE);
    else if (rr <= tol2 * c.bb)
        rails_iter_freeze(c, RAILS_ITER_CONVERGED);
    else if (c.iter >= max_iterations)
        rails_iter_freeze(c, RAILS_ITER_MAXIT);
    else if (rz == 0.0)
        rails_iter_freeze(c, RAILS_ITER_BREAKDOWN);
    else {
        c.beta = rz / c.rho;
        c.rho = rz;
    }
}

// BiCGStab, after r^.v: alpha = rho / r^.v
RAILS_ITER_HD void rails_iter_bi_alpha(rails_iter_col &c, double rhv)
{
    if (!(c.flags & RAILS_ITER_ACTIVE)) {
        c.alpha = c.beta = c.omega = 0.0;
        return;
    }
    if (!rails_iter_finite(rhv)) {
        c.iter++;
        rails_iter_freeze(c, RAILS_ITER_NONFINITE);
    } else if (rhv == 0.0) {
        c.iter++;
        rails_iter_freeze(c, RAILS_ITER_BREAKDOWN);
    } else
        c.alpha = c.rho / rhv;
}

// BiCGStab, after t.s and t.t: omega = t.s / t.t.  t.t = 0 leaves omega = 0 and the decision to the end of the iteration: the half
// step x + alpha p^ may be the solution (s = 0), which is convergence, not breakdown.
RAILS_ITER_HD void rails_iter_bi_omega(rails_iter_col &c, double ts, double tt)
{
    if (!(c.flags & RAILS_ITER_ACTIVE)) {
        c.alpha = c.beta = c.omega = 0.0;
        return;
    }
    if (!rails_iter_finite(ts) || !rails_iter_finite(tt)) {
        c.iter++;
        rails_iter_freeze(c, RAILS_ITER_NONFINITE);
    } else if (tt == 0.0) {
        c.omega = 0.0;
        c.flags |= RAILS_ITER_PENDING;
    } else
        c.omega = ts / tt;
}

// BiCGStab, after the update: the tests, then beta = (rho_new / rho_old) (alpha / omega)
RAILS_ITER_HD void rails_iter_bi_end(rails_iter_col &c, double rhr, double rr, double tol2, int max_iterations)
{
    if (!(c.flags & RAILS_ITER_ACTIVE)) {
        c.alpha = c.beta = c.omega = 0.0;
        return;
    }
    c.iter++;
    c.rr = rr;
    if (!rails_iter_finite(rr) || !rails_iter_finite(rhr))
        rails_iter_freeze(c, RAILS_ITER_NONFINITE);
    else if (rr <= tol2 * c.bb)
        rails_iter_freeze(c, RAILS_ITER_CONVERGED);
    else if (c.flags & RAILS_ITER_PENDING)
        rails_iter_freeze(c, RAILS_ITER_BREAKDOWN);
    else if (c.iter >= max_iterations)
        rails_iter_freeze(c, RAILS_ITER_MAXIT);
    else if (rhr == 0.0 || c.omega == 0.0)
        rails_iter_freeze(c, RAILS_ITER_BREAKDOWN);
    else {
        c.beta = (rhr / c.rho) * (c.alpha / c.omega);
        c.rho = rhr;
    }
}

#endif
