// The host arithmetic of the coordinate back end's block orthogonalisation (rails/BlockOrthHost.hpp), checked without a GPU.  Built by
// rails_amd/csrc/Makefile from that header and host_lapack.o alone (no HIP, no library), run by tests/test_block_orth_host.py.
//
// Every expected value is formed here, in long double where that is cheap, never by the header; inputs come from an integer hash.
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "rails/BlockOrthHost.hpp"

void rails_set_error(const char *fmt, ...) // (host_lapack.o reports a missing LAPACK through it)
{
    va_list ap;
    va_start(ap, fmt);
    std::vfprintf(stderr, fmt, ap);
    va_end(ap);
    std::fputc('\n', stderr);
}

namespace bo = rails::block_orth;
typedef long double ld_t;
typedef std::vector<double> vec;
typedef std::vector<ld_t> lvec;

static const double EPS = std::numeric_limits<double>::epsilon();
static int g_fail = 0, g_checks = 0;
static const char *g_case = "";

#define CHECK(cond)                                                                 \
    do {                                                                            \
        ++g_checks;                                                                 \
        if (!(cond)) {                                                              \
            ++g_fail;                                                               \
            std::printf("FAIL [%s] %s:%d: %s\n", g_case, __FILE__, __LINE__, #cond); \
        }                                                                           \
    } while (0)

static uint32_t hash32(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x7feb352dU;
    x ^= x >> 15;
    x *= 0x846ca68bU;
    x ^= x >> 16;
    return x;
}
static double u01(uint32_t seed, uint32_t i) { return (hash32(seed * 0x9E3779B9U + i) + 0.5) / 4294967296.0; } // (0, 1)
static double sym(uint32_t seed, uint32_t i) { return 2.0 * u01(seed, i) - 1.0; }                                // (-1, 1)

// ---- plain reference arithmetic (column-major) ------------------------------------------------------------------------------------
static vec gram(vec const &A, vec const &B, int m, int na, int nb) // A'B
{
    vec G((size_t)na * nb);
    for (int j = 0; j < nb; ++j)
        for (int i = 0; i < na; ++i) {
            ld_t s = 0;
            for (int l = 0; l < m; ++l) s += (ld_t)A[l + (size_t)i * m] * B[l + (size_t)j * m];
            G[i + (size_t)j * na] = (double)s;
        }
    return G;
}
static void subtract_product(vec &X, vec const &P, vec const &C, int m, int k, int n) // X[:, 0:n) -= P C (C is k x n)
{
    for (int j = 0; j < n; ++j)
        for (int l = 0; l < m; ++l) {
            ld_t s = X[l + (size_t)j * m];
            for (int i = 0; i < k; ++i) s -= (ld_t)P[l + (size_t)i * m] * C[i + (size_t)j * k];
            X[l + (size_t)j * m] = (double)s;
        }
}
// upper Cholesky factor of the n x n matrix S in long double
static lvec chol_upper(lvec const &S, int n)
{
    lvec R((size_t)n * n, 0);
    for (int j = 0; j < n; ++j)
        for (int i = 0; i <= j; ++i) {
            ld_t s = S[i + (size_t)j * n];
            for (int l = 0; l < i; ++l) s -= R[l + (size_t)i * n] * R[l + (size_t)j * n];
            R[i + (size_t)j * n] = i == j ? std::sqrt(s) : s / R[i + (size_t)i * n];
        }
    return R;
}
// what the device does with a block in one CholQR pass: X <- X D^-1 R^-1, R'R = D^-1 G D^-1, D = sqrt(diag G)
static void cholqr_pass(vec &X, vec const &G, int m, int w)
{
    lvec S((size_t)w * w);
    for (int b = 0; b < w; ++b)
        for (int a = 0; a < w; ++a) S[a + (size_t)b * w] = (ld_t)G[a + (size_t)b * w] / (std::sqrt((ld_t)G[a + (size_t)a * w]) * std::sqrt((ld_t)G[b + (size_t)b * w]));
    lvec R = chol_upper(S, w);
    for (int l = 0; l < m; ++l) {
        lvec q(w);
        for (int b = 0; b < w; ++b) { // row l of X D^-1, then the triangular solve q R = x
            ld_t s = (ld_t)X[l + (size_t)b * m] / std::sqrt((ld_t)G[b + (size_t)b * w]);
            for (int a = 0; a < b; ++a) s -= q[a] * R[a + (size_t)b * w];
            q[b] = s / R[b + (size_t)b * w];
        }
        for (int b = 0; b < w; ++b) X[l + (size_t)b * m] = (double)q[b];
    }
}

// ---- 1 ---------------------------------------------------------------------------------------------------------------------------
static void check_factor(vec const &G, int ldg, std::vector<int> const &idx, bool all)
{
    const int r = (int)idx.size();
    vec d, R;
    CHECK(bo::scaled_cholesky(G.data(), ldg, all ? nullptr : idx.data(), r, d, R));
    CHECK((int)d.size() == r && (int)R.size() == r * r);
    if ((int)d.size() != r || (int)R.size() != r * r) return;
    double worst = 0.0;
    for (int b = 0; b < r; ++b)
        for (int a = 0; a < r; ++a) {
            const ld_t ga = G[idx[a] + (size_t)idx[a] * ldg], gb = G[idx[b] + (size_t)idx[b] * ldg];
            const ld_t want = (ld_t)G[idx[a] + (size_t)idx[b] * ldg] / (std::sqrt(ga) * std::sqrt(gb));
            ld_t got = 0;
            for (int l = 0; l < r; ++l) got += (ld_t)R[l + (size_t)a * r] * R[l + (size_t)b * r];
            worst = std::max(worst, (double)std::fabs(got - want));
            if (a > b) CHECK(R[a + (size_t)b * r] == 0.0);
            if (a == b) CHECK(std::fabs((ld_t)d[a] - std::sqrt(ga)) <= 2 * EPS * std::sqrt(ga));
        }
    std::printf("  scaled_cholesky r = %d: |R'R - D^-1 G D^-1| = %.3g (allowed %.3g)\n", r, worst, 8.0 * (r + 1) * EPS);
    CHECK(worst <= 8.0 * (r + 1) * EPS);
}
static void scaled_cholesky_cases()
{
    g_case = "scaled_cholesky";
    const int m = 40, n = 7;
    vec X((size_t)m * n);
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < m; ++i) X[i + (size_t)j * m] = sym(11, i + 64 * j) * std::pow(10.0, -6 + 2 * j); // column norms 1e-6 ... 1e6
    const vec G = gram(X, X, m, n, n);
    check_factor(G, n, {0, 1, 2, 3, 4, 5, 6}, true);
    check_factor(G, n, {0, 2, 3, 6}, false);
    check_factor(G, n, {4}, false);
    check_factor(vec{3.5}, 1, {0}, true);
    vec d, R;
    const vec indefinite = {1.0, 2.0, 2.0, 1.0}; // eigenvalues 3 and -1
    CHECK(!bo::scaled_cholesky(indefinite.data(), 2, nullptr, 2, d, R));
}

// ---- 2 ---------------------------------------------------------------------------------------------------------------------------
static vec seeded_upper(int r, uint32_t seed)
{
    vec R((size_t)r * r, 0.0);
    for (int j = 0; j < r; ++j)
        for (int i = 0; i <= j; ++i) R[i + (size_t)j * r] = i == j ? 0.5 + 1.5 * u01(seed, i) : 0.1 * sym(seed + 1, i + 64 * j);
    return R;
}
static void triangular_cases()
{
    g_case = "upper_inverse / upper_product";
    // Measured here, in long double, for r = 1, 2, 17, 48: |R Rinv - I| = 3.2e-17, 7.7e-17, 8.5e-17, 1.0e-16; upper_product(R, Rinv)
    // comes out as the identity to the last bit, so its distance from the long double product is the same figure.  Allowed: 100 times.
    const int sizes[4] = {1, 2, 17, 48};
    const double bound_inverse[4] = {3.2e-15, 7.7e-15, 8.5e-15, 1.0e-14}, *bound_product = bound_inverse;
    for (int k = 0; k < 4; ++k) {
        const int r = sizes[k];
        const vec R = seeded_upper(r, 100 + r);
        vec Rinv, Pr;
        bo::upper_inverse(R, r, Rinv);
        bo::upper_product(R, Rinv, r, Pr);
        CHECK((int)Rinv.size() == r * r && (int)Pr.size() == r * r);
        double e_inv = 0.0, e_prod = 0.0;
        for (int b = 0; b < r; ++b)
            for (int a = 0; a < r; ++a) {
                ld_t s = 0;
                for (int l = 0; l < r; ++l) s += (ld_t)R[a + (size_t)l * r] * Rinv[l + (size_t)b * r];
                e_inv = std::max(e_inv, (double)std::fabs(s - (a == b ? 1 : 0)));
                e_prod = std::max(e_prod, (double)std::fabs(s - Pr[a + (size_t)b * r]));
                if (a > b) CHECK(Rinv[a + (size_t)b * r] == 0.0 && Pr[a + (size_t)b * r] == 0.0);
            }
        std::printf("  r = %d: |R Rinv - I| = %.3g (allowed %.3g), |upper_product - long double product| = %.3g (allowed %.3g)\n", r, e_inv, bound_inverse[k], e_prod, bound_product[k]);
        CHECK(e_inv <= bound_inverse[k]);
        CHECK(e_prod <= bound_product[k]);
    }
    // a product of two different factors, and the column dot product it is built on
    const int r = 17;
    const vec A = seeded_upper(r, 7), B = seeded_upper(r, 9);
    vec C;
    bo::upper_product(A, B, r, C);
    double e = 0.0;
    for (int b = 0; b < r; ++b)
        for (int a = 0; a < r; ++a) {
            ld_t s = 0;
            for (int l = 0; l < r; ++l) s += (ld_t)A[a + (size_t)l * r] * B[l + (size_t)b * r];
            e = std::max(e, (double)std::fabs(s - C[a + (size_t)b * r]));
        }
    CHECK(e <= r * EPS * 4.0); // r terms, |a b| <= 4 each
    ld_t s = 0;
    for (int l = 0; l < r; ++l) s += (ld_t)A[l + (size_t)16 * r] * B[l + (size_t)16 * r];
    CHECK(std::fabs(s - bo::dot(A.data() + (size_t)16 * r, B.data() + (size_t)16 * r, r)) <= r * EPS * 4.0); // |a_l b_l| <= 4 each
}

// ---- 3 ---------------------------------------------------------------------------------------------------------------------------
static void dgks_cases()
{
    g_case = "dgks_rule";
    const int w = 5;
    const double g = 4.0;
    auto run = [&](const double (&surv)[5], int &w2) {
        vec G0((size_t)w * w, 0.25), c2(w);
        for (int j = 0; j < w; ++j) {
            G0[j + (size_t)j * w] = g;
            c2[j] = g * (1.0 - surv[j]);
        }
        return bo::dgks_rule(G0.data(), w, c2.data(), 0.5, w2);
    };
    int w2 = -1;
    const double mixed[5] = {0.9, 0.4, 0.7, 0.5, 0.51}, fine[5] = {0.9, 0.6, 0.7, 0.75, 0.51};
    double worst = run(mixed, w2);
    CHECK(w2 == 4 && std::fabs(worst - 0.4) <= 4 * EPS);
    worst = run(fine, w2);
    CHECK(w2 == 0 && std::fabs(worst - 0.51) <= 4 * EPS);
    // a zero column, a NaN length, a NaN projection: each needs the round
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int kind = 0; kind < 3; ++kind) {
        vec G0((size_t)w * w, 0.0), c2(w, 0.5);
        for (int j = 0; j < w; ++j) G0[j + (size_t)j * w] = g;
        if (kind == 0) G0[2 + 2 * (size_t)w] = c2[2] = 0.0;
        if (kind == 1) G0[2 + 2 * (size_t)w] = nan;
        if (kind == 2) c2[2] = nan;
        w2 = -1;
        worst = bo::dgks_rule(G0.data(), w, c2.data(), 0.5, w2);
        CHECK(w2 == 3);
        if (kind < 2) CHECK(worst == 0.0);
    }
}

// ---- 4 ---------------------------------------------------------------------------------------------------------------------------
static void prediction_and_rebase()
{
    g_case = "prediction and re-base";
    const int m = 64, d0 = 9, w = 5, dw = d0 + w;
    // P: 9 orthonormal columns (Gram-Schmidt, twice, in long double); N: two more orthonormal directions outside span(P)
    vec PN((size_t)m * (d0 + 2));
    for (int j = 0; j < d0 + 2; ++j) {
        lvec v(m);
        for (int i = 0; i < m; ++i) v[i] = sym(21, i + 64 * j);
        for (int pass = 0; pass < 2; ++pass)
            for (int k = 0; k < j; ++k) {
                ld_t s = 0;
                for (int i = 0; i < m; ++i) s += v[i] * PN[i + (size_t)k * m];
                for (int i = 0; i < m; ++i) v[i] -= s * PN[i + (size_t)k * m];
            }
        ld_t n2 = 0;
        for (int i = 0; i < m; ++i) n2 += v[i] * v[i];
        for (int i = 0; i < m; ++i) PN[i + (size_t)j * m] = (double)(v[i] / std::sqrt(n2));
    }
    const vec P(PN.begin(), PN.begin() + (size_t)m * d0);
    // the block: columns 0, 1 keep 30 % of their squared length outside span(P), columns 2 .. 4 are uniform random
    vec X((size_t)m * w);
    for (int j = 0; j < 2; ++j) {
        lvec in(m, 0);
        ld_t n2 = 0;
        for (int k = 0; k < d0; ++k)
            for (int i = 0; i < m; ++i) in[i] += (ld_t)sym(22 + j, k) * P[i + (size_t)k * m];
        for (int i = 0; i < m; ++i) n2 += in[i] * in[i];
        for (int i = 0; i < m; ++i) X[i + (size_t)j * m] = (double)(std::sqrt((ld_t)0.7 / n2) * in[i] + std::sqrt((ld_t)0.3) * PN[i + (size_t)(d0 + j) * m]);
    }
    for (int j = 2; j < w; ++j)
        for (int i = 0; i < m; ++i) X[i + (size_t)j * m] = sym(30, i + 64 * j);
    // the first round's measurement [C1; X'X] and what the host makes of it
    vec CG((size_t)dw * w);
    const vec C1 = gram(P, X, m, d0, w), G0 = gram(X, X, m, w, w);
    vec c2(w), g0diag(w);
    for (int j = 0; j < w; ++j) {
        for (int i = 0; i < d0; ++i) CG[i + (size_t)j * dw] = C1[i + (size_t)j * d0];
        for (int i = 0; i < w; ++i) CG[(d0 + i) + (size_t)j * dw] = G0[i + (size_t)j * w];
        ld_t s = 0;
        for (int i = 0; i < d0; ++i) s += (ld_t)C1[i + (size_t)j * d0] * C1[i + (size_t)j * d0];
        c2[j] = (double)s;
        g0diag[j] = G0[j + (size_t)j * w];
        CHECK(std::fabs(bo::dot(C1.data() + (size_t)j * d0, C1.data() + (size_t)j * d0, d0) - c2[j]) <= d0 * EPS * c2[j]);
    }
    int w2 = -1;
    const double worst = bo::dgks_rule(G0.data(), w, c2.data(), bo::reorth_survival, w2);
    CHECK(w2 == 2 && std::fabs(worst - 0.3) < 1e-12);
    vec Rfp;
    CHECK(bo::predict_block(CG.data(), d0, w, Rfp));
    CHECK((int)Rfp.size() == w * w);
    if ((int)Rfp.size() != w * w) return;
    for (int b = 0; b < w; ++b)
        for (int a = b + 1; a < w; ++a) CHECK(Rfp[a + (size_t)b * w] == 0.0);
    // the device's part: first update, second round on w2 columns, Gram matrix, Q1, Gram matrix again, Q
    vec Q = X;
    subtract_product(Q, P, C1, m, d0, w);
    const vec X1 = Q; // X - P C1 as the device holds it
    vec C2 = gram(P, Q, m, d0, w2);
    subtract_product(Q, P, C2, m, d0, w2);
    const vec G = gram(Q, Q, m, w, w);
    cholqr_pass(Q, G, m, w);
    const vec G2 = gram(Q, Q, m, w, w);
    cholqr_pass(Q, G2, m, w);
    bo::RebaseMaps maps;
    CHECK(bo::rebase_maps(C2.data(), d0, w2, G.data(), G2.data(), w, Rfp, g0diag, maps) == nullptr);
    std::printf("  prediction off by %.3g\n", maps.off);
    CHECK(maps.off <= 1e-12);
    CHECK((int)maps.Tn.size() == w * w && (int)maps.To.size() == d0 * w);
    if ((int)maps.Tn.size() != w * w || (int)maps.To.size() != d0 * w) return;
    // booked coordinates (a_old, a_new): the block's own columns, then 15 random pairs
    double worst_rel = 0.0;
    for (int t = 0; t < w + 15; ++t) {
        vec cj(dw);
        for (int i = 0; i < dw; ++i) cj[i] = t < w ? (i < d0 ? C1[i + (size_t)t * d0] : Rfp[(i - d0) + (size_t)t * w]) : sym(40 + t, i);
        // P a_old + (X - P C1) Rfp^-1 a_new
        lvec y(w), want(m), got(m);
        for (int a = w - 1; a >= 0; --a) {
            ld_t s = cj[d0 + a];
            for (int l = a + 1; l < w; ++l) s -= (ld_t)Rfp[a + (size_t)l * w] * y[l];
            y[a] = s / Rfp[a + (size_t)a * w];
        }
        for (int i = 0; i < m; ++i) {
            ld_t s = 0;
            for (int k = 0; k < d0; ++k) s += (ld_t)P[i + (size_t)k * m] * cj[k];
            for (int b = 0; b < w; ++b) {
                ld_t x1 = X[i + (size_t)b * m];
                for (int k = 0; k < d0; ++k) x1 -= (ld_t)P[i + (size_t)k * m] * C1[k + (size_t)b * d0];
                s += x1 * y[b];
            }
            want[i] = s;
        }
        bo::rebase_column(maps, cj.data());
        ld_t err = 0, nrm = 0;
        for (int i = 0; i < m; ++i) {
            ld_t s = 0;
            for (int k = 0; k < d0; ++k) s += (ld_t)P[i + (size_t)k * m] * cj[k];
            for (int b = 0; b < w; ++b) s += (ld_t)Q[i + (size_t)b * m] * cj[d0 + b];
            err += (s - want[i]) * (s - want[i]);
            nrm += want[i] * want[i];
        }
        worst_rel = std::max(worst_rel, (double)std::sqrt(err / nrm));
    }
    std::printf("  re-based images against the long double reference: %.3g relative (allowed 1e-13)\n", worst_rel);
    CHECK(worst_rel <= 1e-13);
    // the three rejections
    auto says = [](const char *why, const char *what) { return why && std::strstr(why, what); };
    bo::RebaseMaps rej;
    vec spoilt = Rfp;
    spoilt[0] *= 1.01;
    CHECK(says(bo::rebase_maps(C2.data(), d0, w2, G.data(), G2.data(), w, spoilt, g0diag, rej), "did not confirm its prediction"));
    CHECK(rej.off > 9.8e-3 && rej.off < 1.0e-2);
    vec long_before = g0diag;
    long_before[3] = G[3 + 3 * (size_t)w] * 1.01e8; // G[3, 3] just below 1e-8 of it
    CHECK(says(bo::rebase_maps(C2.data(), d0, w2, G.data(), G2.data(), w, Rfp, long_before, rej), "should have treated with care"));
    vec G2nan = G2;
    G2nan[2 + 2 * (size_t)w] = std::numeric_limits<double>::quiet_NaN();
    CHECK(says(bo::rebase_maps(C2.data(), d0, w2, G.data(), G2nan.data(), w, Rfp, g0diag, rej), "not of full rank"));
}

// ---- 5 ---------------------------------------------------------------------------------------------------------------------------
static void coef_store_cases()
{
    g_case = "CoefStore::in_use";
    const int dim = 6;
    rails::CoefStore s(10, 3, true);
    s.col(1)[dim] = 1.0;     // past the basis dimension: not in use
    s.col(2)[dim - 1] = -2.0; // the last row that counts
    CHECK(!s.in_use(0, dim));
    CHECK(!s.in_use(1, dim));
    CHECK(s.in_use(2, dim));
    CHECK(s.in_use(1, dim + 1) && !s.in_use(2, dim - 1) && s.in_use(2, dim, dim - 1) && !s.in_use(2, dim, dim));
}

int main()
{
    scaled_cholesky_cases();
    triangular_cases();
    dgks_cases();
    prediction_and_rebase();
    coef_store_cases();
    std::printf("%d checks, %d failed\n", g_checks, g_fail);
    if (g_fail == 0) std::printf("ALL PASSED\n");
    return g_fail == 0 ? 0 : 1;
}
