// sprhs_host.cpp -- host part of the sparse right-hand side (include/rails_hip.h: rails_sprhs): the stable transpose of a rectangular
// CSR matrix and ||B'B||_F^2 from the two CSR forms.  No HIP: tests/cpp/sparse_rhs_host.cpp links this object alone.
#include <cstdint>
#include <vector>

#include "rails_hip.h"

// the library's error message (ctx.hip); absent when this object is linked into a stand-alone program
void rails_set_error(const char *fmt, ...) __attribute__((weak));
#define SPRHS_FAIL(...)                                  \
    do {                                                 \
        if (rails_set_error) rails_set_error(__VA_ARGS__); \
        return RAILS_EINVAL;                             \
    } while (0)

namespace {

// monotone rowptr from 0, 0 <= col < n_cols: nothing below reads outside the arrays of a matrix that passes
int csr_check(const char *who, int64_t n_rows, int64_t n_cols, const int64_t *rowptr, const int32_t *col, const double *val)
{
    if (n_rows < 0 || n_cols < 0 || n_cols > 0x7fffffffLL || n_rows > 0x7fffffffLL || !rowptr)
        SPRHS_FAIL("%s: bad shape %lld x %lld or null rowptr", who, (long long)n_rows, (long long)n_cols);
    if (rowptr[0] != 0) SPRHS_FAIL("%s: rowptr[0] != 0", who);
    for (int64_t i = 0; i < n_rows; ++i)
        if (rowptr[i + 1] < rowptr[i]) SPRHS_FAIL("%s: rowptr not monotone at row %lld", who, (long long)i);
    const int64_t nnz = rowptr[n_rows];
    if (nnz > 0 && (!col || !val)) SPRHS_FAIL("%s: null arrays with %lld entries", who, (long long)nnz);
    for (int64_t q = 0; q < nnz; ++q)
        if (col[q] < 0 || col[q] >= n_cols) SPRHS_FAIL("%s: column %d out of range at entry %lld", who, col[q], (long long)q);
    return RAILS_OK;
}

} // namespace

// Counting sort by column: the entries of a transposed row come in increasing original row and duplicates keep their order, so
// every sum over a transposed row has one fixed order.
extern "C" int rails_csr_transpose_host(int64_t n_rows, int64_t n_cols, const int64_t *rowptr, const int32_t *col, const double *val,
                                        int64_t *t_rowptr, int32_t *t_col, double *t_val)
{
    int rc = csr_check("rails_csr_transpose_host", n_rows, n_cols, rowptr, col, val);
    if (rc != RAILS_OK) return rc;
    if (!t_rowptr) SPRHS_FAIL("rails_csr_transpose_host: null output");
    const int64_t nnz = rowptr[n_rows];
    if (nnz > 0 && (!t_col || !t_val)) SPRHS_FAIL("rails_csr_transpose_host: null output arrays");
    for (int64_t j = 0; j <= n_cols; ++j) t_rowptr[j] = 0;
    for (int64_t q = 0; q < nnz; ++q) t_rowptr[col[q] + 1]++;
    for (int64_t j = 0; j < n_cols; ++j) t_rowptr[j + 1] += t_rowptr[j];
    std::vector<int64_t> next(t_rowptr, t_rowptr + n_cols);
    for (int64_t i = 0; i < n_rows; ++i)
        for (int64_t q = rowptr[i]; q < rowptr[i + 1]; ++q) {
            const int64_t d = next[col[q]]++;
            t_col[d] = (int32_t)i;
            t_val[d] = val[q];
        }
    return RAILS_OK;
}

// ||B'B||_F^2 = sum_i sum_j (sum_r B_ri B_rj)^2: row i of B'B is gathered into a sparse accumulator over the columns of B (the rows r of
// column i from the transposed form, their entries from B itself), squared and cleared again.  No p x p array.
extern "C" int rails_csr_gram_norm2_host(int64_t n_rows, int64_t n_cols, const int64_t *rowptr, const int32_t *col, const double *val,
                                         const int64_t *t_rowptr, const int32_t *t_col, const double *t_val, double *out)
{
    int rc = csr_check("rails_csr_gram_norm2_host", n_rows, n_cols, rowptr, col, val);
    if (rc != RAILS_OK) return rc;
    rc = csr_check("rails_csr_gram_norm2_host (transposed form)", n_cols, n_rows, t_rowptr, t_col, t_val);
    if (rc != RAILS_OK) return rc;
    if (!out) SPRHS_FAIL("rails_csr_gram_norm2_host: null output");
    if (t_rowptr[n_cols] != rowptr[n_rows]) SPRHS_FAIL("rails_csr_gram_norm2_host: the two forms differ in their number of entries");
    std::vector<double> w((size_t)n_cols, 0.0);
    std::vector<char> seen((size_t)n_cols, 0);
    std::vector<int32_t> touched;
    long double total = 0.0L;
    for (int64_t i = 0; i < n_cols; ++i) {
        touched.clear();
        for (int64_t a = t_rowptr[i]; a < t_rowptr[i + 1]; ++a) {
            const int64_t r = t_col[a];
            const double v = t_val[a];
            for (int64_t q = rowptr[r]; q < rowptr[r + 1]; ++q) {
                const int32_t j = col[q];
                if (!seen[j]) {
                    seen[j] = 1;
                    touched.push_back(j);
                }
                w[j] += v * val[q];
            }
        }
        long double s = 0.0L;
        for (int32_t j : touched) {
            s += (long double)w[j] * (long double)w[j];
            w[j] = 0.0;
            seen[j] = 0;
        }
        total += s;
    }
    *out = (double)total;
    return RAILS_OK;
}
