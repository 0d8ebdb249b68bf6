// block_amg_host.cpp -- host set-up of the block multigrid preconditioner (block_amg_host.h has the rules).  No HIP:
// tests/cpp/block_amg_host.cpp links this object with amg_host.o, block_jacobi_host.o, bsr_host.o, sprhs_host.o and host_lapack.o.
#include "block_amg_host.h"

#include <algorithm>
#include <cmath>

#include "block_jacobi_host.h"
#include "rails_hip.h"

// the library's error message (ctx.hip); absent when this object is linked into a stand-alone program that has none
void rails_set_error(const char *fmt, ...) __attribute__((weak));
#define BAMG_FAIL(...)                                     \
    do {                                                   \
        if (rails_set_error) rails_set_error(__VA_ARGS__); \
        return RAILS_EINVAL;                               \
    } while (0)

namespace {

bool is_finite(double v) { return v - v == 0.0; }

int check_input(int64_t mb, int b, const int64_t *browptr, const int32_t *bcol, const double *bval)
{
    if (b < RAILS_BJ_MIN_B || b > RAILS_BJ_MAX_B) BAMG_FAIL("rails_bamg_build_host: block size %d outside %d .. %d", b, RAILS_BJ_MIN_B, RAILS_BJ_MAX_B);
    if (mb < 1 || mb * b > 0x7fffffffLL || !browptr) BAMG_FAIL("rails_bamg_build_host: bad size (%lld block rows of %d) or null browptr", (long long)mb, b);
    if (browptr[0] != 0) BAMG_FAIL("rails_bamg_build_host: browptr[0] != 0");
    for (int64_t i = 0; i < mb; ++i)
        if (browptr[i + 1] < browptr[i]) BAMG_FAIL("rails_bamg_build_host: browptr not monotone at block row %lld", (long long)i);
    const int64_t nnzb = browptr[mb];
    if (nnzb > 0 && (!bcol || !bval)) BAMG_FAIL("rails_bamg_build_host: null arrays with %lld blocks", (long long)nnzb);
    for (int64_t i = 0; i < mb; ++i) {
        bool diagonal = false;
        for (int64_t q = browptr[i]; q < browptr[i + 1]; ++q) {
            if (bcol[q] < 0 || bcol[q] >= mb) BAMG_FAIL("rails_bamg_build_host: block column %d out of range at block %lld", bcol[q], (long long)q);
            if (q > browptr[i] && bcol[q] <= bcol[q - 1])
                BAMG_FAIL("rails_bamg_build_host: the block columns of block row %lld are not strictly increasing", (long long)i);
            diagonal = diagonal || bcol[q] == i;
            for (int e = 0; e < b * b; ++e)
                if (!is_finite(bval[q * b * b + e])) BAMG_FAIL("rails_bamg_build_host: entry %d of block %lld is not finite", e, (long long)q);
        }
        if (!diagonal) BAMG_FAIL("rails_bamg_build_host: block row %lld has no stored diagonal block", (long long)i);
    }
    return RAILS_OK;
}

// the scalar diagonal of the diagonal blocks: nonzero and of one sign
int diagonal_sign(const rails_bamg_bsr &A, int level, const std::vector<double> &dblocks, bool *negative, bool *positive)
{
    const int b = A.b;
    *negative = *positive = true;
    for (int64_t i = 0; i < A.mb; ++i)
        for (int r = 0; r < b; ++r) {
            const double d = dblocks[(size_t)i * b * b + (size_t)r * b + r];
            if (d == 0.0 || !is_finite(d))
                BAMG_FAIL("rails_bamg_build_host: level %d, diagonal entry %d of diagonal block %lld is zero or not finite", level, r, (long long)i);
            *negative = *negative && d < 0.0;
            *positive = *positive && d > 0.0;
        }
    return RAILS_OK;
}

// N: the block pattern with the Frobenius norms; diag: its diagonal
void condense(const rails_bamg_bsr &A, rails_amg_csr &N, std::vector<double> &diag)
{
    const int bb = A.b * A.b;
    N.n_rows = N.n_cols = A.mb;
    N.rowptr = A.browptr;
    N.col = A.bcol;
    N.val.assign((size_t)A.nnzb(), 0.0);
    diag.assign((size_t)A.mb, 0.0);
    for (int64_t i = 0; i < A.mb; ++i)
        for (int64_t q = A.browptr[i]; q < A.browptr[i + 1]; ++q) {
            double s = 0.0;
            for (int e = 0; e < bb; ++e) {
                const double t = A.bval[(size_t)q * bb + e] * A.bval[(size_t)q * bb + e];
                s += t;
            }
            N.val[(size_t)q] = std::sqrt(s);
            if (A.bcol[q] == i) diag[(size_t)i] = N.val[(size_t)q];
        }
}

// the expanded matrix: scalar row I b + r holds row r of each block of block row I in stored order, the zeros inside a block included
void expand(const rails_bamg_bsr &A, const double *vals, rails_amg_csr &E)
{
    const int b = A.b;
    E.n_rows = E.n_cols = A.mb * b;
    E.rowptr.assign((size_t)E.n_rows + 1, 0);
    E.col.resize((size_t)A.nnzb() * b * b);
    E.val.resize((size_t)A.nnzb() * b * b);
    int64_t at = 0;
    for (int64_t i = 0; i < A.mb; ++i)
        for (int r = 0; r < b; ++r) {
            for (int64_t q = A.browptr[i]; q < A.browptr[i + 1]; ++q)
                for (int s = 0; s < b; ++s, ++at) {
                    E.col[(size_t)at] = (int32_t)(A.bcol[q] * b + s);
                    E.val[(size_t)at] = vals[(size_t)q * b * b + (size_t)r * b + s];
                }
            E.rowptr[(size_t)(i * b + r) + 1] = at;
        }
}

// G A block by block (the pattern of A) and the bound hi = max_i sum_j |(G A)_ij|
double scaled_blocks(const rails_bamg_bsr &A, const std::vector<double> &ginv, std::vector<double> &ga)
{
    const int b = A.b, bb = b * b;
    ga.assign((size_t)A.nnzb() * bb, 0.0);
    double hi = 0.0;
    for (int64_t i = 0; i < A.mb; ++i) {
        const double *g = ginv.data() + (size_t)i * bb;
        double rowsum[RAILS_BJ_MAX_B] = {};
        for (int64_t q = A.browptr[i]; q < A.browptr[i + 1]; ++q) {
            const double *a = A.bval.data() + (size_t)q * bb;
            double *o = ga.data() + (size_t)q * bb;
            for (int r = 0; r < b; ++r)
                for (int s = 0; s < b; ++s) {
                    double v = 0.0;
                    for (int k = 0; k < b; ++k) {
                        const double t = g[r * b + k] * a[k * b + s]; // (a product, then a sum: no contraction into one rounding)
                        v += t;
                    }
                    o[r * b + s] = v;
                    rowsum[r] += std::fabs(v);
                }
        }
        for (int r = 0; r < b; ++r)
            if (!(rowsum[r] <= hi)) hi = rowsum[r]; // a NaN shows
    }
    return hi;
}

} // namespace

int rails_bamg_build_host(int64_t mb, int b, const int64_t *browptr, const int32_t *bcol, const double *bval, double theta, int coarse,
                          rails_bamg_hierarchy *out)
{
    if (!out) BAMG_FAIL("rails_bamg_build_host: null output");
    if (!(theta >= 0.0 && theta < 1.0)) BAMG_FAIL("rails_bamg_build_host: theta %g is not in [0, 1)", theta);
    if (coarse < 1 || coarse > RAILS_AMG_MAX_COARSE) BAMG_FAIL("rails_bamg_build_host: coarse %d is not in 1 .. %d", coarse, RAILS_AMG_MAX_COARSE);
    int rc = check_input(mb, b, browptr, bcol, bval);
    if (rc != RAILS_OK) return rc;
    out->b = b;
    out->levels.clear();
    out->coarse_inv.clear();
    rails_bamg_bsr cur;
    cur.b = b;
    cur.mb = mb;
    cur.browptr.assign(browptr, browptr + mb + 1);
    cur.bcol.assign(bcol, bcol + browptr[mb]);
    cur.bval.assign(bval, bval + browptr[mb] * b * b);
    rails_amg_csr E; // the expanded current matrix
    char err[256] = "";
    for (int l = 0;; ++l) {
        std::vector<double> dblocks((size_t)cur.mb * b * b);
        rails_bj_from_bsr(cur.mb, b, cur.browptr.data(), cur.bcol.data(), cur.bval.data(), dblocks.data());
        bool negative = false, positive = false;
        rc = diagonal_sign(cur, l, dblocks, &negative, &positive);
        if (rc != RAILS_OK) return rc;
        if (!negative && !positive) BAMG_FAIL("rails_bamg_build_host: the matrix is not definite (level %d has diagonal entries of both signs)", l);
        if (l == 0) out->defsign = negative ? -1.0 : 1.0;
        if ((negative ? -1.0 : 1.0) != out->defsign) BAMG_FAIL("rails_bamg_build_host: the matrix is not definite (the diagonal changes sign at level %d)", l);
        expand(cur, cur.bval.data(), E);
        if (cur.mb * b <= coarse || l + 1 >= RAILS_AMG_MAX_LEVELS) break;
        rails_amg_csr N;
        std::vector<double> ndiag;
        condense(cur, N, ndiag);
        std::vector<int32_t> agg;
        const int64_t n_agg = rails_amg_aggregate(N, ndiag, theta * std::pow(0.5, l), agg);
        if (n_agg * 5 > cur.mb * 4) break; // the level would keep more than 0.8 of its block rows
        rails_bamg_level L;
        L.ginv.resize(dblocks.size());
        if (rails_bj_invert(cur.mb, b, dblocks.data(), L.ginv.data(), err, sizeof err)) BAMG_FAIL("rails_bamg_build_host: level %d: %s", l, err);
        std::vector<double> ga;
        L.hi = scaled_blocks(cur, L.ginv, ga);
        if (!(L.hi > 0.0) || !is_finite(L.hi)) BAMG_FAIL("rails_bamg_build_host: level %d has no finite bound on its spectrum", l);
        // P = T - omega (G A) T with T = T_nodes (x) I_b
        rails_amg_csr GA, T;
        expand(cur, ga.data(), GA);
        T.n_rows = cur.mb * b;
        T.n_cols = n_agg * b;
        T.rowptr.resize((size_t)T.n_rows + 1);
        T.col.resize((size_t)T.n_rows);
        T.val.assign((size_t)T.n_rows, 1.0);
        for (int64_t i = 0; i <= T.n_rows; ++i) T.rowptr[(size_t)i] = i;
        for (int64_t i = 0; i < T.n_rows; ++i) T.col[(size_t)i] = (int32_t)((int64_t)agg[(size_t)(i / b)] * b + i % b);
        rails_amg_spgemm(GA, T, L.P); // the diagonal blocks are stored, so the pattern of (G A) T holds the pattern of T
        const double omega = 4.0 / (3.0 * L.hi);
        for (int64_t i = 0; i < T.n_rows; ++i)
            for (int64_t q = L.P.rowptr[(size_t)i]; q < L.P.rowptr[(size_t)i + 1]; ++q) {
                const double t = omega * L.P.val[(size_t)q];
                L.P.val[(size_t)q] = (L.P.col[(size_t)q] == T.col[(size_t)i] ? 1.0 : 0.0) - t;
            }
        L.R.n_rows = L.P.n_cols;
        L.R.n_cols = L.P.n_rows;
        L.R.rowptr.resize((size_t)L.R.n_rows + 1);
        L.R.col.resize(L.P.col.size());
        L.R.val.resize(L.P.val.size());
        rc = rails_csr_transpose_host(L.P.n_rows, L.P.n_cols, L.P.rowptr.data(), L.P.col.data(), L.P.val.data(), L.R.rowptr.data(), L.R.col.data(), L.R.val.data());
        if (rc != RAILS_OK) return rc;
        rails_amg_csr RA, next;
        rails_amg_spgemm(L.R, E, RA);
        rails_amg_spgemm(RA, L.P, next);
        rails_bamg_bsr nb;
        nb.b = b;
        nb.mb = n_agg;
        int64_t nnzb = 0;
        rc = rails_bsr_count_host(next.n_rows, next.n_cols, b, next.rowptr.data(), next.col.data(), &nnzb);
        if (rc != RAILS_OK) return rc;
        nb.browptr.resize((size_t)n_agg + 1);
        nb.bcol.resize((size_t)nnzb);
        nb.bval.resize((size_t)nnzb * b * b);
        rc = rails_bsr_fill_host(next.n_rows, next.n_cols, b, next.rowptr.data(), next.col.data(), next.val.data(), nb.browptr.data(), nb.bcol.data(), nb.bval.data());
        if (rc != RAILS_OK) return rc;
        L.A = std::move(cur);
        L.agg = std::move(agg);
        out->levels.push_back(std::move(L));
        cur = std::move(nb);
    }
    if (cur.mb * b > RAILS_AMG_MAX_COARSE)
        BAMG_FAIL("rails_bamg_build_host: the matrix does not coarsen: %lld rows are left after %d level(s), above the %d a dense coarsest block may have",
                  (long long)(cur.mb * b), (int)out->levels.size(), RAILS_AMG_MAX_COARSE);
    rc = rails_amg_dense_inverse(E, out->defsign, out->coarse_inv);
    if (rc != RAILS_OK) return rc;
    out->coarse = std::move(cur);
    return RAILS_OK;
}
