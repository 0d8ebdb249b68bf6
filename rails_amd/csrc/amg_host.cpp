// amg_host.cpp -- host set-up of the smoothed-aggregation multigrid preconditioner (amg_host.h has the rules).  No HIP:
// tests/cpp/amg_host.cpp links this object with sprhs_host.o (the stable transpose) and host_lapack.o (the LAPACK pass-throughs).
#include "amg_host.h"

#include <algorithm>
#include <cmath>

#include "cheb_coef.h"
#include "rails_hip.h"

// the library's error message (ctx.hip); absent when this object is linked into a stand-alone program that has none
void rails_set_error(const char *fmt, ...) __attribute__((weak));
#define AMG_FAIL(...)                                      \
    do {                                                   \
        if (rails_set_error) rails_set_error(__VA_ARGS__); \
        return RAILS_EINVAL;                               \
    } while (0)

namespace {

bool is_finite(double v) { return v - v == 0.0; }

// what sprhs_host.cpp's csr_check asks, and on top: square, at least one row, columns of a row strictly increasing, finite values
int check_input(int64_t n, const int64_t *rowptr, const int32_t *col, const double *val)
{
    if (n < 1 || n > 0x7fffffffLL || !rowptr) AMG_FAIL("rails_amg_build_host: bad size %lld or null rowptr", (long long)n);
    if (rowptr[0] != 0) AMG_FAIL("rails_amg_build_host: rowptr[0] != 0");
    for (int64_t i = 0; i < n; ++i)
        if (rowptr[i + 1] < rowptr[i]) AMG_FAIL("rails_amg_build_host: rowptr not monotone at row %lld", (long long)i);
    const int64_t nnz = rowptr[n];
    if (nnz > 0 && (!col || !val)) AMG_FAIL("rails_amg_build_host: null arrays with %lld entries", (long long)nnz);
    for (int64_t i = 0; i < n; ++i)
        for (int64_t q = rowptr[i]; q < rowptr[i + 1]; ++q) {
            if (col[q] < 0 || col[q] >= n) AMG_FAIL("rails_amg_build_host: column %d out of range at entry %lld", col[q], (long long)q);
            if (q > rowptr[i] && col[q] <= col[q - 1]) AMG_FAIL("rails_amg_build_host: the columns of row %lld are not strictly increasing", (long long)i);
            if (!is_finite(val[q])) AMG_FAIL("rails_amg_build_host: entry %lld is not finite", (long long)q);
        }
    return RAILS_OK;
}

// the diagonal and 1 / diagonal; a missing, zero or non-finite diagonal entry is refused.  *negative / *positive: whether every entry is.
int take_diagonal(const rails_amg_csr &A, int level, std::vector<double> &diag, std::vector<double> &dinv, bool *negative, bool *positive)
{
    diag.assign((size_t)A.n_rows, 0.0);
    dinv.assign((size_t)A.n_rows, 0.0);
    *negative = *positive = true;
    for (int64_t i = 0; i < A.n_rows; ++i) {
        double d = 0.0;
        bool found = false;
        for (int64_t q = A.rowptr[i]; q < A.rowptr[i + 1]; ++q)
            if (A.col[q] == i) {
                d = A.val[q];
                found = true;
            }
        if (!found || d == 0.0 || !is_finite(d)) AMG_FAIL("rails_amg_build_host: level %d, diagonal entry %lld is %s", level, (long long)i, found ? "zero or not finite" : "missing");
        *negative = *negative && d < 0.0;
        *positive = *positive && d > 0.0;
        diag[(size_t)i] = d;
        dinv[(size_t)i] = 1.0 / d;
    }
    return RAILS_OK;
}

} // namespace

// the three passes; returns the number of aggregates
int64_t rails_amg_aggregate(const rails_amg_csr &A, const std::vector<double> &diag, double theta_l, std::vector<int32_t> &agg)
{
    const int64_t n = A.n_rows;
    auto strong = [&](int64_t i, int64_t q) {
        const int64_t j = A.col[q];
        return j != i && std::fabs(A.val[q]) >= theta_l * std::sqrt(std::fabs(diag[(size_t)i]) * std::fabs(diag[(size_t)j]));
    };
    agg.assign((size_t)n, -1);
    int32_t count = 0;
    for (int64_t i = 0; i < n; ++i) { // pass 1
        if (agg[(size_t)i] >= 0) continue;
        bool any = false, free_all = true;
        for (int64_t q = A.rowptr[i]; q < A.rowptr[i + 1]; ++q)
            if (strong(i, q)) {
                any = true;
                free_all = free_all && agg[(size_t)A.col[q]] < 0;
            }
        if (!any || !free_all) continue;
        agg[(size_t)i] = count;
        for (int64_t q = A.rowptr[i]; q < A.rowptr[i + 1]; ++q)
            if (strong(i, q)) agg[(size_t)A.col[q]] = count;
        ++count;
    }
    const std::vector<int32_t> after1(agg); // pass 2 decides against the state after pass 1
    for (int64_t i = 0; i < n; ++i) {
        if (after1[(size_t)i] >= 0) continue;
        double best = -1.0;
        for (int64_t q = A.rowptr[i]; q < A.rowptr[i + 1]; ++q)
            if (strong(i, q) && after1[(size_t)A.col[q]] >= 0 && std::fabs(A.val[q]) > best) { // ties: the lower column stays
                best = std::fabs(A.val[q]);
                agg[(size_t)i] = after1[(size_t)A.col[q]];
            }
    }
    for (int64_t i = 0; i < n; ++i) { // pass 3
        if (agg[(size_t)i] >= 0) continue;
        agg[(size_t)i] = count;
        for (int64_t q = A.rowptr[i]; q < A.rowptr[i + 1]; ++q)
            if (strong(i, q) && agg[(size_t)A.col[q]] < 0) agg[(size_t)A.col[q]] = count;
        ++count;
    }
    return count;
}

// C = A B by Gustavson's row-wise product: row i of C gathers a_ik times row k of B in the stored order of both, so every entry is one
// sum of fixed order; the columns of a row are then sorted and every structural entry is kept.
void rails_amg_spgemm(const rails_amg_csr &A, const rails_amg_csr &B, rails_amg_csr &C)
{
    C.n_rows = A.n_rows;
    C.n_cols = B.n_cols;
    C.rowptr.assign((size_t)A.n_rows + 1, 0);
    C.col.clear();
    C.val.clear();
    std::vector<double> w((size_t)B.n_cols, 0.0);
    std::vector<char> seen((size_t)B.n_cols, 0);
    std::vector<int32_t> touched;
    for (int64_t i = 0; i < A.n_rows; ++i) {
        touched.clear();
        for (int64_t a = A.rowptr[i]; a < A.rowptr[i + 1]; ++a) {
            const int64_t k = A.col[a];
            const double v = A.val[a];
            for (int64_t q = B.rowptr[k]; q < B.rowptr[k + 1]; ++q) {
                const int32_t j = B.col[q];
                if (!seen[(size_t)j]) {
                    seen[(size_t)j] = 1;
                    touched.push_back(j);
                }
                const double t = v * B.val[q]; // (a product, then a sum: no contraction into one rounding)
                w[(size_t)j] += t;
            }
        }
        std::sort(touched.begin(), touched.end());
        for (int32_t j : touched) {
            C.col.push_back(j);
            C.val.push_back(w[(size_t)j]);
            w[(size_t)j] = 0.0;
            seen[(size_t)j] = 0;
        }
        C.rowptr[(size_t)i + 1] = (int64_t)C.col.size();
    }
}

namespace {

// P = (I - omega D^-1 A) T: entry (i, a) is [a == agg_i] - (omega / d_i) sum over the j of aggregate a of a_ij, the sum in stored order
void smoothed_prolongation(const rails_amg_csr &A, const std::vector<double> &dinv, const std::vector<int32_t> &agg, int64_t n_agg, double omega,
                           rails_amg_csr &P)
{
    rails_amg_csr T;
    T.n_rows = A.n_rows;
    T.n_cols = n_agg;
    T.rowptr.resize((size_t)A.n_rows + 1);
    T.col.assign(agg.begin(), agg.end());
    T.val.assign((size_t)A.n_rows, 1.0);
    for (int64_t i = 0; i <= A.n_rows; ++i) T.rowptr[(size_t)i] = i;
    rails_amg_spgemm(A, T, P); // A T; the diagonal of A is stored, so the pattern of A T holds the pattern of T
    for (int64_t i = 0; i < A.n_rows; ++i) {
        const double s = omega * dinv[(size_t)i];
        for (int64_t q = P.rowptr[i]; q < P.rowptr[i + 1]; ++q) {
            const double t = s * P.val[(size_t)q];
            P.val[(size_t)q] = (P.col[(size_t)q] == agg[(size_t)i] ? 1.0 : 0.0) - t;
        }
    }
}

} // namespace

// the dense inverse of the last matrix through Cholesky of defsign A_L
int rails_amg_dense_inverse(const rails_amg_csr &A, double defsign, std::vector<double> &inv)
{
    const int n = (int)A.n_rows;
    std::vector<double> M((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i)
        for (int64_t q = A.rowptr[i]; q < A.rowptr[i + 1]; ++q) M[(size_t)i + (size_t)A.col[q] * n] = defsign * A.val[q];
    // the lower triangle is what dpotrf reads; a matrix that is not symmetric is none of this preconditioner's business, but must not pass
    // as one: compare the two triangles loosely, against the largest entry
    double largest = 0.0;
    for (double v : M) largest = std::max(largest, std::fabs(v));
    for (int j = 0; j < n; ++j)
        for (int i = j + 1; i < n; ++i) {
            const double a = M[(size_t)i + (size_t)j * n], b = M[(size_t)j + (size_t)i * n];
            if (std::fabs(a - b) > 1e-8 * largest) AMG_FAIL("rails_amg_build_host: the matrix is not symmetric (coarsest level, entries %d, %d)", i, j);
        }
    int info = 0;
    rails_dpotrf('L', n, M.data(), n, &info);
    if (info == -100) AMG_FAIL("rails_amg_build_host: no host LAPACK for the coarsest level's Cholesky factorisation");
    if (info != 0) AMG_FAIL("rails_amg_build_host: the matrix is not definite (Cholesky of the coarsest level stops at pivot %d of %d)", info, n);
    inv.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) inv[(size_t)i * (n + 1)] = 1.0;
    rails_dtrsm('L', 'L', 'N', 'N', n, n, 1.0, M.data(), n, inv.data(), n);
    rails_dtrsm('L', 'L', 'T', 'N', n, n, defsign, M.data(), n, inv.data(), n);
    for (double v : inv)
        if (!is_finite(v)) AMG_FAIL("rails_amg_build_host: the inverse of the coarsest level is not finite");
    return RAILS_OK;
}

int rails_amg_build_host(int64_t n, const int64_t *rowptr, const int32_t *col, const double *val, double theta, int coarse, rails_amg_hierarchy *out)
{
    if (!out) AMG_FAIL("rails_amg_build_host: null output");
    if (!(theta >= 0.0 && theta < 1.0)) AMG_FAIL("rails_amg_build_host: theta %g is not in [0, 1)", theta);
    if (coarse < 1 || coarse > RAILS_AMG_MAX_COARSE) AMG_FAIL("rails_amg_build_host: coarse %d is not in 1 .. %d", coarse, RAILS_AMG_MAX_COARSE);
    int rc = check_input(n, rowptr, col, val);
    if (rc != RAILS_OK) return rc;
    out->levels.clear();
    out->coarse_inv.clear();
    rails_amg_csr cur;
    cur.n_rows = cur.n_cols = n;
    cur.rowptr.assign(rowptr, rowptr + n + 1);
    cur.col.assign(col, col + rowptr[n]);
    cur.val.assign(val, val + rowptr[n]);
    for (int l = 0;; ++l) {
        std::vector<double> diag, dinv;
        bool negative = false, positive = false;
        rc = take_diagonal(cur, l, diag, dinv, &negative, &positive);
        if (rc != RAILS_OK) return rc;
        if (!negative && !positive) AMG_FAIL("rails_amg_build_host: the matrix is not definite (level %d has diagonal entries of both signs)", l);
        if (l == 0) out->defsign = negative ? -1.0 : 1.0;
        if ((negative ? -1.0 : 1.0) != out->defsign) AMG_FAIL("rails_amg_build_host: the matrix is not definite (the diagonal changes sign at level %d)", l);
        if (cur.n_rows <= coarse || l + 1 >= RAILS_AMG_MAX_LEVELS) break;
        std::vector<int32_t> agg;
        const int64_t n_agg = rails_amg_aggregate(cur, diag, theta * std::pow(0.5, l), agg);
        if (n_agg * 5 > cur.n_rows * 4) break; // the level would keep more than 0.8 of its rows
        rails_amg_level L;
        L.hi = rails_cheb_gershgorin(cur.n_rows, cur.rowptr.data(), cur.val.data(), dinv.data());
        if (!(L.hi > 0.0) || !is_finite(L.hi)) AMG_FAIL("rails_amg_build_host: level %d has no finite bound on its spectrum", l);
        smoothed_prolongation(cur, dinv, agg, n_agg, 4.0 / (3.0 * L.hi), L.P);
        L.R.n_rows = n_agg;
        L.R.n_cols = cur.n_rows;
        L.R.rowptr.resize((size_t)n_agg + 1);
        L.R.col.resize(L.P.col.size());
        L.R.val.resize(L.P.val.size());
        rc = rails_csr_transpose_host(L.P.n_rows, L.P.n_cols, L.P.rowptr.data(), L.P.col.data(), L.P.val.data(), L.R.rowptr.data(), L.R.col.data(), L.R.val.data());
        if (rc != RAILS_OK) return rc;
        rails_amg_csr RA, next;
        rails_amg_spgemm(L.R, cur, RA);
        rails_amg_spgemm(RA, L.P, next);
        L.A = std::move(cur);
        L.dinv = std::move(dinv);
        L.agg = std::move(agg);
        out->levels.push_back(std::move(L));
        cur = std::move(next);
    }
    if (cur.n_rows > RAILS_AMG_MAX_COARSE)
        AMG_FAIL("rails_amg_build_host: the matrix does not coarsen: %lld rows are left after %d level(s), above the %d a dense coarsest block may have",
                 (long long)cur.n_rows, (int)out->levels.size(), RAILS_AMG_MAX_COARSE);
    rc = rails_amg_dense_inverse(cur, out->defsign, out->coarse_inv);
    if (rc != RAILS_OK) return rc;
    out->coarse = std::move(cur);
    return RAILS_OK;
}
