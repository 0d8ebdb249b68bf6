// lyap_dense.cpp -- the projected (dense, host) continuous Lyapunov solve of the C ABI, with the argument meaning of the reference's shim
//   rails_sb03md  <- RAILS::sb03md      (src/SlicotWrapper.hpp:14-16, src/SlicotWrapper.cpp:8-49)
// SLICOT is not available anywhere in the image.  Four routes lead to the same X: the eigen-decomposition for symmetric A, the factored
// ADI iteration and the squared Smith iteration (both verified by their residual) for nonsymmetric A of 32 rows and more, and
// Bartels-Stewart on dgees + dtrsyl3 / dtrsyl, which answers whatever the others did not.  Which of them a call attempts is decided in
// lyap_route.h; LAPACK comes through host_lapack.h.
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "host_lapack.h"
#include "lyap_route.h"
#include "rails_hip.h"

using lyap::Outcome;
using lyap::Route;

namespace {

// The switches of the environment, read once per process.  RAILS_SB03MD_SMITH switches both iterative routes.
struct Switches {
    bool symmetric = env_flag("RAILS_SB03MD_SYMMETRIC", true), iterative = env_flag("RAILS_SB03MD_SMITH", true), blocked = env_flag("RAILS_SB03MD_BLOCKED", true),
         inherit = env_flag("RAILS_SB03MD_ADI_INHERIT", true), explicit_steps = env_flag("RAILS_SB03MD_ADI_INVERSE", true), trace = getenv("RAILS_SB03MD_TRACE") != nullptr;
};
const Switches &switches()
{
    static const Switches s{};
    return s;
}

// A call's problem, op(A) X + X op(A)' = C, and where its result goes.  X holds the right-hand side until a route has its answer: a
// route that fails leaves A and X as they were.  M and C are loaded (once) for the iterative routes only.
struct Problem {
    bool tr;
    int n, lda;
    double *A;
    std::vector<double> M, C; // n x n: M = op(A), C = (X + X') / 2
};
struct Result {
    double *X;
    int ldx, *info;
    double *scale;
};
void load(Problem &P, const Result &R)
{
    const int n = P.n;
    P.C.resize((size_t)n * n);
    P.M.resize((size_t)n * n);
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) {
            P.M[i + (size_t)j * n] = P.tr ? P.A[i + (size_t)j * P.lda] : P.A[j + (size_t)i * P.lda];
            P.C[i + (size_t)j * n] = 0.5 * (R.X[i + (size_t)j * R.ldx] + R.X[j + (size_t)i * R.ldx]);
        }
}
void store(const Result &R, int n, const std::vector<double> &Y)
{
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) R.X[i + (size_t)j * R.ldx] = Y[i + (size_t)j * n];
}

double sumsq(const double *z, size_t len)
{
    double s2 = 0.0;
    for (size_t q = 0; q < len; ++q) s2 += z[q] * z[q];
    return s2;
}
double fro(const std::vector<double> &Z) { return std::sqrt(sumsq(Z.data(), Z.size())); }

// Y (n x n) <- (Y + Y') / 2
void symmetrise(int n, std::vector<double> &Y)
{
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < j; ++i) {
            const double v = 0.5 * (Y[i + (size_t)j * n] + Y[j + (size_t)i * n]);
            Y[i + (size_t)j * n] = v;
            Y[j + (size_t)i * n] = v;
        }
}

// The fence of the iterative routes: ||M Y + Y M' - C||_F <= 2e-15 (2 ||M|| ||Y|| + ||C||), the level Bartels-Stewart reaches, for a
// symmetric Y (Y M' = (M Y)').  One pass measures the squared norms; the product ||M|| ||Y|| is the caller's (each route keeps the
// arithmetic it always had: `my`).  W is n x n scratch.
struct Fence {
    double r2, m2, y2, c2; // squared Frobenius norms of the residual, M, Y and C
    double residual() const { return std::sqrt(r2); }
    double allowed(double my) const { return 2e-15 * (2.0 * my + std::sqrt(c2)); }
    bool holds(double my) const { return residual() <= allowed(my); }
};
Fence residual_fence(const Problem &P, const std::vector<double> &Y, std::vector<double> &W)
{
    const int n = P.n;
    gemm('N', 'N', n, n, n, P.M.data(), n, Y.data(), n, W.data(), n);
    Fence f = {0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) {
            const double r = W[i + (size_t)j * n] + W[j + (size_t)i * n] - P.C[i + (size_t)j * n];
            f.r2 += r * r;
            f.m2 += P.M[i + (size_t)j * n] * P.M[i + (size_t)j * n];
            f.y2 += Y[i + (size_t)j * n] * Y[i + (size_t)j * n];
            f.c2 += P.C[i + (size_t)j * n] * P.C[i + (size_t)j * n];
        }
    return f;
}

// ---- symmetric A (projections of symmetric operators: Laplacians, stencils): its Schur form is its eigen-decomposition A = Q L Q', and
// the triangular Sylvester solve collapses to Y_ij = F_ij / (l_i + l_j).  Same equation, same result up to rounding, about a third of the
// cost of dgees + dtrsyl.  Only for A symmetric to rounding; eigen-solver trouble or l_i + l_j = 0 leave the call to the general routes.
Outcome route_symmetric(Problem &P, const Result &R)
{
    const int n = P.n, lda = P.lda;
    double *A = P.A;
    double amax = 0.0, asym = 0.0;
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < j; ++i) {
            const double a = A[i + (size_t)j * lda], b = A[j + (size_t)i * lda];
            amax = std::max(amax, std::max(std::fabs(a), std::fabs(b)));
            asym = std::max(asym, std::fabs(a - b));
        }
    for (int i = 0; i < n; ++i) amax = std::max(amax, std::fabs(A[i + (size_t)i * lda]));
    if (!lyap::symmetric_to_rounding(asym, amax)) return Outcome::NotApplicable;
    std::vector<double> Q((size_t)n * n), lam(n), F((size_t)n * n), W((size_t)n * n);
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) Q[i + (size_t)j * n] = 0.5 * (A[i + (size_t)j * lda] + A[j + (size_t)i * lda]);
    int sinfo = 0;
    sym_eig('V', 'U', n, Q.data(), n, lam.data(), 0, &sinfo);
    if (sinfo != 0) return Outcome::Failed;
    gemm('T', 'N', n, n, n, Q.data(), n, R.X, R.ldx, W.data(), n);
    gemm('N', 'N', n, n, n, W.data(), n, Q.data(), n, F.data(), n);
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) {
            const double den = lam[i] + lam[j];
            if (!(std::fabs(den) > 1e-300)) return Outcome::Failed;
            F[i + (size_t)j * n] /= den;
        }
    gemm('N', 'N', n, n, n, Q.data(), n, F.data(), n, W.data(), n);
    gemm('N', 'T', n, n, n, W.data(), n, Q.data(), n, F.data(), n);
    store(R, n, F);
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) A[i + (size_t)j * lda] = (i == j) ? lam[i] : 0.0; // the (diagonal) Schur form, as the general path leaves it
    *R.scale = 1.0;
    return Outcome::Solved;
}

// ---- squared Smith iteration for M X + X M' = C (M stable): with p > 0, S = M - p I,
//     X = Md X Md' + Cd,   Md = S^-1 (M + p I) = I + 2 p S^-1,   Cd = -2 p S^-1 C S^-T,
// and X = sum_j Md^j Cd Md'^j is summed by squaring: Y <- Y + Ak Y Ak', Ak <- Ak^2.  With p = -trace(M)/n the spectral radius of
// Md is small whenever the spectrum of M is clustered relative to its distance from the imaginary axis -- the projections V'AV
// of diagonally dominant operators (the benchmark's: rho ~ 0.1-0.25, 4-6 squarings).  All level-3 BLAS: ~40 n^3 flops at GEMM
// speed against the ~25 n^3 flops of the Hessenberg QR sweeps at a fifth of it (2.5 vs 6.9 ms at n = 160).  The result is
// VERIFIED (residual_fence), and anything else (slow convergence, an unstable M, a failed check) fails: Bartels-Stewart then answers.
Outcome route_smith(Problem &P, const Result &R)
{
    const HostLapack &lp = host_lapack();
    if (!lp.dgetrf || !lp.dgetrs) return Outcome::Failed;
    const int n = P.n;
    const size_t nn = (size_t)n * n;
    std::vector<double> S(nn), Ak(nn), Y(nn), T1(nn), T2(nn);
    double trace = 0.0;
    for (int j = 0; j < n; ++j) trace += P.M[j + (size_t)j * n];
    const double p = -trace / n;
    if (!(p > 0.0) || !std::isfinite(p)) return Outcome::Failed;
    S = P.M;
    for (int j = 0; j < n; ++j) S[j + (size_t)j * n] -= p;
    std::vector<int> ipiv(n);
    int info = 0;
    lp.dgetrf(&n, &n, S.data(), &n, ipiv.data(), &info);
    if (info != 0) return Outcome::Failed;
    std::fill(Ak.begin(), Ak.end(), 0.0);
    for (int j = 0; j < n; ++j) Ak[j + (size_t)j * n] = 1.0;
    const char N = 'N';
    lp.dgetrs(&N, &n, &n, S.data(), &n, ipiv.data(), Ak.data(), &n, &info); // Ak = S^-1
    if (info != 0) return Outcome::Failed;
    // Y0 = Cd = -2p S^-1 C S^-T
    gemm('N', 'N', n, n, n, Ak.data(), n, P.C.data(), n, T1.data(), n);
    gemm('N', 'T', n, n, n, T1.data(), n, Ak.data(), n, Y.data(), n);
    for (size_t q = 0; q < nn; ++q) Y[q] *= -2.0 * p;
    for (size_t q = 0; q < nn; ++q) Ak[q] *= 2.0 * p; // Ak = Md = I + 2p S^-1
    for (int j = 0; j < n; ++j) Ak[j + (size_t)j * n] += 1.0;
    bool converged = false;
    for (int k = 0; k < 10; ++k) {
        gemm('N', 'N', n, n, n, Ak.data(), n, Y.data(), n, T1.data(), n);
        gemm('N', 'T', n, n, n, T1.data(), n, Ak.data(), n, T2.data(), n);
        const double inc = fro(T2), ny = fro(Y);
        if (!std::isfinite(inc) || inc > 10.0 * ny) return Outcome::Failed; // not a contraction: M is not stable (enough)
        for (size_t q = 0; q < nn; ++q) Y[q] += T2[q];
        if (inc <= 1e-8 * ny) { // the ratio squares from one step to the next: what is left is below 1e-16 (the fence below decides)
            converged = true;
            break;
        }
        if (k >= 5 && inc > 1e-2 * ny) return Outcome::Failed; // the ratio squares per step: would need more squarings than Bartels-Stewart costs
        gemm('N', 'N', n, n, n, Ak.data(), n, Ak.data(), n, T1.data(), n);
        Ak.swap(T1);
    }
    if (!converged) return Outcome::Failed;
    symmetrise(n, Y);
    const Fence fence = residual_fence(P, Y, T1);
    if (!fence.holds(std::sqrt(fence.m2) * std::sqrt(fence.y2))) return Outcome::Failed;
    store(R, n, Y);
    return Outcome::Solved;
}

// ---- factored ADI for a right-hand side of low rank -- the solver's is +-(V'B)(V'B)' with p = 16 columns.  C = sign * F F' (pivoted
// Cholesky, rank r) and, for shifts p_1, p_2, ... > 0 (Li / White's low-rank ADI),
//     Z_1 = sqrt(2 p_1) (M - p_1 I)^-1 F,   Z_j = sqrt(p_j / p_j-1) [I + (p_j + p_j-1) (M - p_j I)^-1] Z_j-1,   X = -sign * sum_j Z_j Z_j'.
// The shifts are Wachspress' L parameters for [a, b], the extent of M's spectrum along the real axis, used cyclically: every mode is
// damped by the shifts near it, so the terms shrink by a roughly constant factor per cycle however far the spectrum is spread (the
// squared Smith iteration above has ONE shift and pays for spread spectra with squarings of n x n matrices).  Cost: L + 1 LU
// factorisations, one solve with r right-hand sides per term, X = Z Z', the residual check -- ~12 n^3 flops at n = 200, r = 16 against
// ~35 n^3.  All terms are positive semi-definite: nothing cancels.  Same fences: verified residual, early exit when the terms do not shrink.

// The laps of one attempt, for the RAILS_SB03MD_TRACE line
struct Stopwatch {
    enum Lap { Factor, Bounds, Operators, Terms, Form, kLaps };
    static double now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    double begin = now(), mark = begin, ms[kLaps] = {0, 0, 0, 0, 0};
    void lap(Lap l)
    {
        const double t = now();
        ms[l] += t - mark;
        mark = t;
    }
};

// The right-hand side as sign * F F' (F: n x rank)
struct LowRankRhs {
    double sign = 1.0;
    int rank = 0;
    std::vector<double> F;
};
// NotApplicable: not (semi-)definite of low rank -- the dense form decides, and nothing is held against this route.  W: n x n scratch.
Outcome factor_rhs(const Problem &P, std::vector<double> &W, LowRankRhs &rhs)
{
    const int n = P.n;
    double trc = 0.0, dmax = 0.0;
    for (int j = 0; j < n; ++j) {
        trc += P.C[j + (size_t)j * n];
        dmax = std::max(dmax, std::fabs(P.C[j + (size_t)j * n]));
    }
    if (!(dmax > 0.0) || !std::isfinite(dmax)) return Outcome::Failed;
    rhs.sign = trc >= 0.0 ? 1.0 : -1.0;
    for (size_t q = 0; q < W.size(); ++q) W[q] = rhs.sign * P.C[q];
    std::vector<int> piv(n);
    int info = 0;
    rails_dpstrf('U', n, W.data(), n, piv.data(), &rhs.rank, 1e-15 * dmax, &info);
    if (info < 0 || rhs.rank <= 0 || rhs.rank > n / 3) return Outcome::NotApplicable;
    rhs.F.assign((size_t)n * rhs.rank, 0.0); // F(piv[j], i) = R(i, j)
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < rhs.rank && i <= j; ++i) rhs.F[piv[j] + (size_t)i * n] = W[i + (size_t)j * n];
    return Outcome::Solved;
}

// LU (LAPACK's packed form, pivots 1-based) of the n x n matrix S whose leading n1 x n1 block has the factors (LU1, ip1): with
// P11 A11 = L11 U11 from before,
//     U12 = L11^-1 P11 A12,   L21 = A21 U11^-1,   P22 (A22 - L21 U12) = L22 U22,   rows of L21 swapped as P22 says,
// which is the factorisation dgetrf would produce if its pivot search in the first n1 columns stopped at row n1: (n - n1) / n of the
// triangular-solve work instead of a factorisation (n = 200, 16 new rows: 0.06 ms for two shifts instead of 0.26 + 0.19 for the bounds).
bool extend_lu(int n1, int n, const std::vector<double> &LU1, const std::vector<int> &ip1, std::vector<double> &S, std::vector<int> &ip)
{
    const HostLapack &lp = host_lapack();
    const int nb = n - n1, one = 1;
    const double d_one = 1.0, d_mone = -1.0;
    for (int j = 0; j < n1; ++j) memcpy(&S[(size_t)j * n], &LU1[(size_t)j * n1], sizeof(double) * n1);
    ip.assign(n, 0);
    for (int j = 0; j < n1; ++j) ip[j] = ip1[j];
    if (nb == 0) return true;
    double *A12 = &S[(size_t)n1 * n], *A21 = &S[n1], *A22 = &S[n1 + (size_t)n1 * n];
    lp.dlaswp(&nb, A12, &n, &one, &n1, ip1.data(), &one);
    lp.dtrsm("L", "L", "N", "U", &n1, &nb, &d_one, S.data(), &n, A12, &n);
    lp.dtrsm("R", "U", "N", "N", &nb, &n1, &d_one, S.data(), &n, A21, &n);
    lp.dgemm("N", "N", &nb, &nb, &n1, &d_mone, A21, &n, A12, &n, &d_one, A22, &n);
    std::vector<int> ip2(nb);
    int info = 0;
    lp.dgetrf(&nb, &nb, A22, &n, ip2.data(), &info);
    if (info != 0) return false;
    lp.dlaswp(&n1, A21, &n, &one, &nb, ip2.data(), &one);
    for (int j = 0; j < nb; ++j) ip[n1 + j] = ip2[j] + n1;
    return true;
}

// In place: S <- S^-1 (n x n), through dgetrf + dgetri (or n solves with the identity)
bool invert_dense(int n, std::vector<double> &S)
{
    const HostLapack &lp = host_lapack();
    std::vector<int> ip(n);
    int info = 0;
    lp.dgetrf(&n, &n, S.data(), &n, ip.data(), &info);
    if (info != 0) return false;
    if (lp.dgetri) {
        double wq = 0.0;
        int lw = -1;
        lp.dgetri(&n, S.data(), &n, ip.data(), &wq, &lw, &info);
        lw = info == 0 ? std::max(n, (int)wq) : 64 * n;
        std::vector<double> work((size_t)lw);
        lp.dgetri(&n, S.data(), &n, ip.data(), work.data(), &lw, &info);
        return info == 0;
    }
    std::vector<double> I((size_t)n * n, 0.0);
    for (int j = 0; j < n; ++j) I[j + (size_t)j * n] = 1.0;
    const char N = 'N';
    lp.dgetrs(&N, &n, &n, S.data(), &n, ip.data(), I.data(), &n, &info);
    S.swap(I);
    return info == 0;
}

// S (n x n, holding the matrix on entry) <- S^-1, given the inverse J1 of its leading n1 x n1 block: with E = J1 A12, F = A21 J1,
// C = (A22 - A21 E)^-1:  S^-1 = [J1 + E C F, -E C; -C F, C].  Four thin products and an (n - n1)-square inverse: (n - n1) / n of an inversion.
bool extend_inverse(int n1, int n, const std::vector<double> &J1, std::vector<double> &S)
{
    const HostLapack &lp = host_lapack();
    const int nb = n - n1;
    if (nb == 0) {
        S = J1;
        return true;
    }
    const double d_one = 1.0, d_mone = -1.0, d_zero = 0.0;
    double *A12 = &S[(size_t)n1 * n], *A21 = &S[n1], *A22 = &S[n1 + (size_t)n1 * n];
    std::vector<double> E((size_t)n1 * nb), F((size_t)nb * n1), Cm((size_t)nb * nb), G((size_t)nb * n1);
    lp.dgemm("N", "N", &n1, &nb, &n1, &d_one, J1.data(), &n1, A12, &n, &d_zero, E.data(), &n1);
    lp.dgemm("N", "N", &nb, &n1, &n1, &d_one, A21, &n, J1.data(), &n1, &d_zero, F.data(), &nb);
    for (int j = 0; j < nb; ++j)
        for (int i = 0; i < nb; ++i) Cm[i + (size_t)j * nb] = A22[i + (size_t)j * n];
    lp.dgemm("N", "N", &nb, &nb, &n1, &d_mone, A21, &n, E.data(), &n1, &d_one, Cm.data(), &nb);
    if (!invert_dense(nb, Cm)) return false;
    lp.dgemm("N", "N", &nb, &n1, &nb, &d_one, Cm.data(), &nb, F.data(), &nb, &d_zero, G.data(), &nb); // G = C F
    // leading block: J1 + E G
    for (int j = 0; j < n1; ++j) memcpy(&S[(size_t)j * n], &J1[(size_t)j * n1], sizeof(double) * n1);
    lp.dgemm("N", "N", &n1, &n1, &nb, &d_one, E.data(), &n1, G.data(), &nb, &d_one, S.data(), &n);
    // -E C, -G, C
    lp.dgemm("N", "N", &n1, &nb, &nb, &d_mone, E.data(), &n1, Cm.data(), &nb, &d_zero, A12, &n);
    for (int j = 0; j < n1; ++j)
        for (int i = 0; i < nb; ++i) A21[i + (size_t)j * n] = -G[i + (size_t)j * nb];
    for (int j = 0; j < nb; ++j)
        for (int i = 0; i < nb; ++i) A22[i + (size_t)j * n] = Cm[i + (size_t)j * nb];
    return true;
}

// The shifted operators (M - p_i I)^-1, i < L, of one call, in one of two forms.  The LU form keeps factors and a term is a pair of
// triangular solves.  From n = 64 on (lyap::explicit_steps_gate) the inverses are formed and with them the step operators
// S_i = sqrt(p_i / p_i-1) [I + (p_i + p_i-1) (M - p_i I)^-1], so that a term is ONE product S_i Z with 16 columns: a pair of triangular
// solves with 16 right-hand sides runs at a third of that rate, and there are 20-odd terms (n = 177: 0.77 -> 0.23 ms).  An inversion
// costs more than a factorisation (0.3-0.4 ms per shift at n = 200), but inside a restart cycle either form is EXTENDED like the matrix.
struct ShiftedOps {
    int n = 0;
    virtual ~ShiftedOps() {}
    // Operator i < L from S = M - p_i I: from scratch, or from the operator i of `kept` -- the same form, the same shift, the leading
    // kept->n rows of M
    virtual void resize(size_t L) = 0;
    virtual bool set(size_t i, std::vector<double> &&S, const ShiftedOps *kept) = 0;
    virtual bool solve_vector(std::vector<double> &v, std::vector<double> &u) const = 0; // v <- (M - p_0 I)^-1 v, u: scratch
    virtual bool first(const std::vector<double> &shift, const std::vector<double> &F, int rank, std::vector<double> &T) = 0; // T = (M - p_0 I)^-1 F
    // T = sqrt(pj / pp) [I + (pj + pp) (M - pj I)^-1] Z, pj = shift[cur], pp the shift of the term before
    virtual bool step(int cur, double pj, double pp, const double *Z, int rank, std::vector<double> &T) const = 0;
    virtual void release_steps() {} // the terms are done: drop what only they needed (the next call extends the operators themselves)

    bool build(int rows, const std::vector<double> &M, const std::vector<double> &shift, const ShiftedOps *kept = nullptr)
    {
        n = rows;
        resize(shift.size());
        for (size_t i = 0; i < shift.size(); ++i) {
            std::vector<double> S = M;
            for (int j = 0; j < n; ++j) S[j + (size_t)j * n] -= shift[i];
            if (!set(i, std::move(S), kept)) return false;
        }
        return true;
    }
    bool extend(const ShiftedOps &kept, int rows, const std::vector<double> &M, const std::vector<double> &shift) { return build(rows, M, shift, &kept); }
};
struct LuOps : ShiftedOps {
    std::vector<std::vector<double>> LU;
    std::vector<std::vector<int>> ip;
    void resize(size_t L) override { LU.resize(L), ip.assign(L, std::vector<int>(n)); }
    bool set(size_t i, std::vector<double> &&S, const ShiftedOps *kept) override
    {
        LU[i] = std::move(S);
        if (const LuOps *k = static_cast<const LuOps *>(kept)) return extend_lu(k->n, n, k->LU[i], k->ip[i], LU[i], ip[i]);
        int info = 0;
        host_lapack().dgetrf(&n, &n, LU[i].data(), &n, ip[i].data(), &info);
        return info == 0;
    }
    bool solve(int i, int cols, double *T) const
    {
        int info = 0;
        host_lapack().dgetrs("N", &n, &cols, LU[i].data(), &n, ip[i].data(), T, &n, &info);
        return info == 0;
    }
    bool solve_vector(std::vector<double> &v, std::vector<double> &) const override { return solve(0, 1, v.data()); }
    bool first(const std::vector<double> &, const std::vector<double> &F, int rank, std::vector<double> &T) override { return T = F, solve(0, rank, T.data()); }
    bool step(int cur, double pj, double pp, const double *Z, int rank, std::vector<double> &T) const override
    {
        std::copy(Z, Z + T.size(), T.begin());
        if (!solve(cur, rank, T.data())) return false;
        const double f = std::sqrt(pj / pp), g = pj + pp;
        for (size_t q = 0; q < T.size(); ++q) T[q] = f * (Z[q] + g * T[q]);
        return true;
    }
};
struct ExplicitOps : ShiftedOps {
    std::vector<std::vector<double>> Inv, Sm; // the inverses are what the next call extends: they are kept as they are beside the step operators
    void resize(size_t L) override { Inv.resize(L); }
    bool set(size_t i, std::vector<double> &&S, const ShiftedOps *kept) override
    {
        Inv[i] = std::move(S);
        if (const ExplicitOps *k = static_cast<const ExplicitOps *>(kept)) return extend_inverse(k->n, n, k->Inv[i], Inv[i]);
        return invert_dense(n, Inv[i]);
    }
    bool solve_vector(std::vector<double> &v, std::vector<double> &u) const override
    {
        gemm('N', 'N', n, 1, n, Inv[0].data(), n, v.data(), n, u.data(), n);
        v = u;
        return true;
    }
    bool first(const std::vector<double> &shift, const std::vector<double> &F, int rank, std::vector<double> &T) override
    {
        const int L = (int)shift.size();
        Sm.resize(L);
        for (int i = 0; i < L; ++i) {
            const double pj = shift[i], pp = shift[(i + L - 1) % L];
            const double f = std::sqrt(pj / pp), fg = f * (pj + pp);
            Sm[i].resize((size_t)n * n);
            for (size_t q = 0; q < Sm[i].size(); ++q) Sm[i][q] = fg * Inv[i][q];
            for (int j = 0; j < n; ++j) Sm[i][j + (size_t)j * n] += f;
        }
        gemm('N', 'N', n, rank, n, Inv[0].data(), n, F.data(), n, T.data(), n);
        return true;
    }
    bool step(int cur, double, double, const double *Z, int rank, std::vector<double> &T) const override
    {
        gemm('N', 'N', n, rank, n, Sm[cur].data(), n, Z, n, T.data(), n);
        return true;
    }
    void release_steps() override { std::vector<std::vector<double>>().swap(Sm); }
};
std::unique_ptr<ShiftedOps> make_ops(bool explicit_form)
{
    if (explicit_form) return std::unique_ptr<ShiftedOps>(new ExplicitOps);
    return std::unique_ptr<ShiftedOps>(new LuOps);
}

// Extent [a, b] of the spectrum along the real axis: b ~ largest modulus (power iteration), a ~ smallest (inverse iteration with
// (M - p I)^-1 = ops' first operator: the eigenvalue nearest p >= 0 is the one of smallest modulus when the spectrum is near the
// negative real axis), six steps each from a fixed start vector
bool spectral_extent(const Problem &P, const ShiftedOps &ops, double pshift, double *a_out, double *b_out)
{
    const int n = P.n;
    std::vector<double> v(n), u(n);
    auto nrm = [&](std::vector<double> const &z) { return std::sqrt(sumsq(z.data(), (size_t)n)); };
    for (int i = 0; i < n; ++i) v[i] = 1.0 + 0.37 * std::sin(1.0 + 2.3 * i);
    double bmax = 0.0, amin = 0.0;
    for (int it = 0; it < 6; ++it) {
        const double nv = nrm(v);
        for (int i = 0; i < n; ++i) v[i] /= nv;
        gemm('N', 'N', n, 1, n, P.M.data(), n, v.data(), n, u.data(), n);
        bmax = std::max(bmax, nrm(u));
        v = u;
    }
    for (int i = 0; i < n; ++i) v[i] = 1.0 + 0.37 * std::sin(1.0 + 2.3 * i);
    for (int it = 0; it < 6; ++it) {
        const double nv = nrm(v);
        for (int i = 0; i < n; ++i) v[i] /= nv;
        if (!ops.solve_vector(v, u)) return false;
        amin = nrm(v); // -> 1 / |lambda - p|min
    }
    if (!(amin > 0.0) || !(bmax > 0.0) || !std::isfinite(amin) || !std::isfinite(bmax)) return false;
    const double lmin = 1.0 / amin - pshift;
    if (!(lmin > 0.0)) return false;
    *a_out = 0.8 * lmin, *b_out = 1.2 * bmax;
    if (!(*a_out < *b_out)) *a_out = 0.5 * *b_out;
    return true;
}

// What the factored ADI route keeps from its last successful call (per thread): inside a restart cycle the solver's projected matrix
// grows by BORDERING -- V gets new orthonormal columns, V'AV keeps its leading block (src/LyapunovSolver.hpp:146-160) -- so the next
// call's matrix has this one as its leading block.  Then the shifts are kept (the extent of the spectrum moves by a few percent per
// trip: the estimate by power / inverse iteration, an LU of M and twelve solves, is skipped) and the shifted operators are EXTENDED
// instead of recomputed.  M - p I with p > 0 and M stable is far from singular, and the result is judged by the residual fence either
// way; a call that does not converge with inherited shifts is repeated from scratch.
struct AdiCache {
    lyap::AdiKept kept;
    std::vector<double> M;
    std::unique_ptr<ShiftedOps> ops;
    // what the next call may build on (the call is answered: what it had is handed over, not copied)
    void keep(lyap::AdiKept &k, std::vector<double> &M_call, std::unique_ptr<ShiftedOps> &ops_call)
    {
        kept = std::move(k);
        M.swap(M_call);
        ops_call->release_steps();
        ops = std::move(ops_call);
    }
};
struct ThreadState {
    lyap::Rests rests;
    AdiCache adi;
};
ThreadState &thread_state()
{
    static thread_local ThreadState s;
    return s;
}
std::atomic<long> g_iterative{0}, g_schur{0}, g_adi_extended{0}, g_adi_fresh{0};

// Shifts and operators of this call, k (k.n, k.tr, k.explicit_form set) and ops: inherited from the cache ...
bool inherited_shifts(const Problem &P, const AdiCache &cache, bool allowed, lyap::AdiKept &k, ShiftedOps &ops, Stopwatch &sw)
{
    const HostLapack &lp = host_lapack();
    const int n = P.n, n1 = cache.kept.n;
    bool inherit = lyap::inherit_shape(cache.kept, allowed, lp.dlaswp && lp.dtrsm, P.tr, n, k.explicit_form);
    for (int j = 0; inherit && j < n1; ++j) inherit = memcmp(&P.M[(size_t)j * n], &cache.M[(size_t)j * n1], sizeof(double) * n1) == 0;
    if (!inherit) return false;
    k.a = cache.kept.a, k.b = cache.kept.b, k.L = cache.kept.L, k.shift = cache.kept.shift;
    inherit = ops.extend(*cache.ops, n, P.M, k.shift);
    sw.lap(Stopwatch::Operators);
    double a_now = 0.0, b_now = 0.0;
    inherit = inherit && spectral_extent(P, ops, k.shift[0], &a_now, &b_now) && lyap::shifts_still_cover(k.a, k.b, a_now, b_now);
    sw.lap(Stopwatch::Bounds);
    return inherit;
}
// ... or fresh: the extent with an LU of M itself, Wachspress' parameters for it, their operators
bool fresh_shifts(const Problem &P, lyap::AdiKept &k, ShiftedOps &ops, Stopwatch &sw)
{
    LuOps lu0;
    if (!lu0.build(P.n, P.M, std::vector<double>(1, 0.0)) || !spectral_extent(P, lu0, 0.0, &k.a, &k.b)) return false;
    sw.lap(Stopwatch::Bounds);
    k.L = lyap::wachspress_count(k.a, k.b);
    if (k.L == 0) return false;
    k.shift = lyap::wachspress_shifts(k.a, k.b, k.L);
    const bool built = ops.build(P.n, P.M, k.shift);
    sw.lap(Stopwatch::Operators);
    return built;
}

// The terms Z_1, Z_2, ... (n x rank each, appended to Z) until one is below 1e-17 of the sum (true), or M shows itself not stable, Z
// grows past its limit or a cycle does not shrink the terms, or the limit of terms is reached (false)
bool adi_terms(int n, const LowRankRhs &rhs, const lyap::AdiKept &k, ShiftedOps &ops, std::vector<double> &Z)
{
    const int L = k.L, rank = rhs.rank, max_terms = lyap::max_terms(L), max_cols = lyap::max_cols(n);
    const size_t blk = (size_t)n * rank;
    std::vector<double> T(blk);
    Z.reserve(blk * 24);
    if (!ops.first(k.shift, rhs.F, rank, T)) return false;
    const double f0 = std::sqrt(2.0 * k.shift[0]);
    for (size_t q = 0; q < blk; ++q) T[q] *= f0;
    Z.insert(Z.end(), T.begin(), T.end());
    double total = sumsq(T.data(), blk), cycle_start = total;
    bool converged = false;
    for (int j = 1; j < max_terms; ++j) {
        const int cur = j % L, prv = (j - 1) % L;
        if (!ops.step(cur, k.shift[cur], k.shift[prv], Z.data() + (size_t)(j - 1) * blk, rank, T)) return false;
        const double n2 = sumsq(T.data(), blk);
        if (!std::isfinite(n2) || n2 > 1e4 * total) return false; // M is not stable
        if ((int)((size_t)(j + 1) * rank) > max_cols) return false;
        Z.insert(Z.end(), T.begin(), T.end());
        total += n2;
        if (n2 <= 1e-17 * total) {
            converged = true;
            break;
        }
        if (cur == L - 1) { // end of a cycle: against the same term of the cycle before it must have shrunk by a clear factor
            if (j >= 2 * L - 1 && n2 > 0.2 * cycle_start) {
                if (switches().trace) fprintf(stderr, "sb03md ADI: n %d, spectrum ~[%.3g, %.3g], %d shifts: term %d is %.2e of the same term one cycle earlier -- giving up\n", n, k.a, k.b, L, j, n2 / cycle_start);
                return false;
            }
            cycle_start = n2;
        }
    }
    if (switches().trace) fprintf(stderr, "sb03md ADI: n %d rank %d, spectrum ~[%.3g, %.3g], %d shifts, %d terms, converged %d\n", n, rank, k.a, k.b, L, (int)(Z.size() / blk), (int)converged);
    return converged;
}

// Y = -sign Z Z' (M Y + Y M' = C), and its fence with the ORIGINAL right-hand side (also covers the truncation of the pivoted Cholesky factor)
Fence adi_solution(const Problem &P, double sign, const std::vector<double> &Z, std::vector<double> &Y, std::vector<double> &W)
{
    const HostLapack &lp = host_lapack();
    const int n = P.n, cols = (int)(Z.size() / n);
    Y.resize((size_t)n * n);
    if (lp.dsyrk) { // the upper triangle at half the flops, mirrored
        const double one_d = 1.0, zero_d = 0.0;
        lp.dsyrk("U", "N", &n, &cols, &one_d, Z.data(), &n, &zero_d, Y.data(), &n);
        for (int j = 0; j < n; ++j)
            for (int i = 0; i < j; ++i) Y[j + (size_t)i * n] = Y[i + (size_t)j * n];
    } else {
        gemm('N', 'T', n, n, cols, Z.data(), n, Z.data(), n, Y.data(), n);
        symmetrise(n, Y);
    }
    for (size_t q = 0; q < Y.size(); ++q) Y[q] *= -sign;
    return residual_fence(P, Y, W);
}

// One attempt.  *inherited: it built on the call before (and may be worth repeating from scratch)
Outcome adi_once(Problem &P, const Result &R, bool from_scratch, bool *inherited)
{
    *inherited = false;
    const HostLapack &lp = host_lapack();
    if (!lp.dgetrf || !lp.dgetrs) return Outcome::Failed;
    Stopwatch sw;
    const int n = P.n;
    std::vector<double> W((size_t)n * n), Y, Z;
    LowRankRhs rhs;
    const Outcome factored = factor_rhs(P, W, rhs);
    if (factored != Outcome::Solved) return factored;
    sw.lap(Stopwatch::Factor);
    AdiCache &cache = thread_state().adi;
    lyap::AdiKept k;
    k.n = n, k.tr = P.tr, k.explicit_form = lyap::explicit_steps_gate(n, switches().explicit_steps);
    std::unique_ptr<ShiftedOps> ops = make_ops(k.explicit_form);
    const bool inherit = inherited_shifts(P, cache, switches().inherit && !from_scratch, k, *ops, sw);
    if (!inherit && !fresh_shifts(P, k, *ops, sw)) return Outcome::Failed;
    (inherit ? g_adi_extended : g_adi_fresh)++;
    *inherited = inherit;
    if (!adi_terms(n, rhs, k, *ops, Z)) return Outcome::Failed;
    sw.lap(Stopwatch::Terms);
    const Fence fence = adi_solution(P, rhs.sign, Z, Y, W);
    sw.lap(Stopwatch::Form);
    const double my = std::sqrt(fence.m2 * fence.y2);
    if (switches().trace)
        fprintf(stderr, "sb03md ADI: residual %.2e of %.2e allowed; ms: factor C %.2f, bounds %.2f, %d LU %.2f, terms %.2f, X = ZZ' + check %.2f, total %.2f\n", fence.residual(),
                fence.allowed(my), sw.ms[Stopwatch::Factor], sw.ms[Stopwatch::Bounds], k.L, sw.ms[Stopwatch::Operators], sw.ms[Stopwatch::Terms], sw.ms[Stopwatch::Form], Stopwatch::now() - sw.begin);
    if (!fence.holds(my)) return Outcome::Failed;
    store(R, n, Y);
    cache.keep(k, P.M, ops);
    return Outcome::Solved;
}

Outcome route_adi(Problem &P, const Result &R)
{
    bool inherited = false;
    const Outcome o = adi_once(P, R, false, &inherited);
    if (o != Outcome::Failed || !inherited) return o;
    // inherited shifts or factors did not do: once more from scratch (X still holds the right-hand side)
    return adi_once(P, R, true, &inherited);
}

// ---- Bartels-Stewart: A = U S U' (dgees; A is overwritten by its real Schur form, as SLICOT does with FACT='N'), the triangular
// Sylvester equation for U' C U, and back
Outcome route_schur(Problem &P, const Result &R)
{
    const HostLapack &lp = host_lapack();
    const bool tr = P.tr;
    int n = P.n, lda = P.lda;
    double *A = P.A, *scale = R.scale;
    std::vector<double> U((size_t)n * n), wr(n), wi(n), F((size_t)n * n), W((size_t)n * n);
    int sdim = 0, lwork = -1, linfo = 0;
    double wq = 0.0;
    lp.dgees("V", "N", nullptr, &n, A, &lda, &sdim, wr.data(), wi.data(), U.data(), &n, &wq, &lwork, nullptr, &linfo);
    lwork = std::max((int)wq, 3 * n);
    std::vector<double> work((size_t)lwork);
    lp.dgees("V", "N", nullptr, &n, A, &lda, &sdim, wr.data(), wi.data(), U.data(), &n, work.data(), &lwork, nullptr, &linfo);
    if (linfo != 0) { // QR iteration failed: SLICOT reports 0 < info <= n
        *R.info = linfo > n ? n : linfo;
        return Outcome::Failed;
    }
    // F = U^T C U
    gemm('T', 'N', n, n, n, U.data(), n, R.X, R.ldx, W.data(), n);
    gemm('N', 'N', n, n, n, W.data(), n, U.data(), n, F.data(), n);
    // S Y + Y S^T = scale F (trans='T')   or   S^T Y + Y S = scale F (trans='N')
    int isgn = 1, tinfo = 0;
    bool done = false;
    if (lp.dtrsyl3 && lyap::blocked_sylvester_gate(n, switches().blocked)) {
        int liwork = -1, ldswork = -1, iq = 0, qinfo = 0;
        double sq[2] = {0.0, 0.0};
        lp.dtrsyl3(tr ? "N" : "T", tr ? "T" : "N", &isgn, &n, &n, A, &lda, A, &lda, F.data(), &n, scale, &iq, &liwork, sq, &ldswork, &qinfo);
        if (qinfo == 0 && iq > 0 && sq[0] > 0 && sq[1] > 0) {
            liwork = iq;
            ldswork = (int)sq[0];
            const int swcols = (int)sq[1];
            std::vector<int> iwork((size_t)liwork);
            std::vector<double> swork((size_t)ldswork * swcols);
            lp.dtrsyl3(tr ? "N" : "T", tr ? "T" : "N", &isgn, &n, &n, A, &lda, A, &lda, F.data(), &n, scale, iwork.data(), &liwork, swork.data(), &ldswork, &tinfo);
            done = tinfo >= 0;
        }
    }
    if (!done) lp.dtrsyl(tr ? "N" : "T", tr ? "T" : "N", &isgn, &n, &n, A, &lda, A, &lda, F.data(), &n, scale, &tinfo);
    // X = U Y U^T
    gemm('N', 'N', n, n, n, U.data(), n, F.data(), n, W.data(), n);
    gemm('N', 'T', n, n, n, W.data(), n, U.data(), n, F.data(), n);
    store(R, n, F);
    if (tinfo == 1) *R.info = n + 1; // perturbed to avoid overflow: A and -A^T have (nearly) common eigenvalues
    return Outcome::Solved;
}

} // namespace

extern "C" void rails_sb03md_set_pause(int calls) { thread_state().rests.set(calls); }
extern "C" void rails_sb03md_counts(long *smith, long *schur)
{
    if (smith) *smith = g_iterative.load();
    if (schur) *schur = g_schur.load();
}
extern "C" void rails_sb03md_adi_counts(long *extended, long *fresh)
{
    if (extended) *extended = g_adi_extended.load();
    if (fresh) *fresh = g_adi_fresh.load();
}

// Continuous-time Lyapunov equation, SB03MD('C','X','N',trans):
//   trans = 'T':  A X + X A^T = scale * C        trans = 'N':  A^T X + X A = scale * C
// C symmetric, X overwrites C.  Where Bartels-Stewart answers, A is overwritten by its real Schur form; the iterative routes leave A
// its values (no caller of this library reads A afterwards).  A solver whose projected matrices are not of an iterative route's kind
// stops asking it for a while (lyap_route.h: the rests).
extern "C" void rails_sb03md(char dico, char job, char fact, char trans, int n, double *A, int lda, double *X, int ldx, double *scale,
                             int *info)
{
    *info = 0;
    if (n < 1) { // the reference prints "n < 1 is not supported" and returns (src/SlicotWrapper.cpp:12-16)
        fprintf(stderr, "rails_sb03md: n < 1 is not supported\n");
        return;
    }
    if ((dico != 'C' && dico != 'c') || (job != 'X' && job != 'x') || (fact != 'N' && fact != 'n')) {
        fprintf(stderr, "rails_sb03md: only DICO='C', JOB='X', FACT='N' is supported\n");
        *info = -1;
        return;
    }
    if (rails_host_lapack_init(nullptr) != RAILS_OK) {
        *info = -100;
        return;
    }
    if (!all_finite(n, n, A, lda) || !all_finite(n, n, X, ldx)) {
        fprintf(stderr, "rails_sb03md: A or C holds NaN or Inf entries\n");
        *info = n + 2;
        return;
    }
    Problem P = {(trans == 'T' || trans == 't' || trans == 'C' || trans == 'c'), n, lda, A, {}, {}};
    const Result R = {X, ldx, info, scale};
    if (lyap::symmetry_is_measured(n, switches().symmetric) && route_symmetric(P, R) == Outcome::Solved) return;
    lyap::Rests &rests = thread_state().rests;
    Route route = lyap::first_route(rests, n, switches().iterative);
    if (route != Route::Schur) load(P, R);
    while (route == Route::Adi || route == Route::Smith) route = lyap::next_route(rests, route, (route == Route::Adi ? route_adi : route_smith)(P, R));
    if (route == Route::Done) {
        g_iterative++;
        *scale = 1.0;
        return;
    }
    g_schur++;
    route_schur(P, R);
}
