// bsr_host.cpp -- host part of the block-CSR operator (include/rails_hip.h: rails_bsr_*): the b x b blocking of a CSR matrix and the
// stable transpose of a block matrix.  No HIP: tests/cpp/bsr_host.cpp links this object alone.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "rails_hip.h"

// the library's error message (ctx.hip); a stand-alone program that links this object alone may leave it out or bring its own
void rails_set_error(const char *fmt, ...) __attribute__((weak));
#define BSR_FAIL(...)                                    \
    do {                                                 \
        if (rails_set_error) rails_set_error(__VA_ARGS__); \
        return RAILS_EINVAL;                             \
    } while (0)

namespace {

int block_size_check(const char *who, int b)
{
    if (b < 2 || b > 8) BSR_FAIL("%s: block size %d outside 2 .. 8", who, b);
    return RAILS_OK;
}

// monotone rowptr from 0, 0 <= col < n_cols: nothing below reads outside the arrays of a matrix that passes
int rows_check(const char *who, int64_t n_rows, int64_t n_cols, const int64_t *rowptr, const int32_t *col)
{
    if (n_rows < 0 || n_cols < 0 || n_cols > 0x7fffffffLL || n_rows > 0x7fffffffLL || !rowptr)
        BSR_FAIL("%s: bad shape %lld x %lld or null rowptr", who, (long long)n_rows, (long long)n_cols);
    if (rowptr[0] != 0) BSR_FAIL("%s: rowptr[0] != 0", who);
    for (int64_t i = 0; i < n_rows; ++i)
        if (rowptr[i + 1] < rowptr[i]) BSR_FAIL("%s: rowptr not monotone at row %lld", who, (long long)i);
    const int64_t nnz = rowptr[n_rows];
    if (nnz > 0 && !col) BSR_FAIL("%s: null column array with %lld entries", who, (long long)nnz);
    for (int64_t q = 0; q < nnz; ++q)
        if (col[q] < 0 || col[q] >= n_cols) BSR_FAIL("%s: column %d out of range at entry %lld", who, col[q], (long long)q);
    return RAILS_OK;
}

int csr_check(const char *who, int64_t m, int64_t n_cols, int b, const int64_t *rowptr, const int32_t *col)
{
    int rc = block_size_check(who, b);
    if (rc != RAILS_OK) return rc;
    if (m < 0 || n_cols < 0 || m % b != 0 || n_cols % b != 0) BSR_FAIL("%s: %lld x %lld is no multiple of the block size %d", who, (long long)m, (long long)n_cols, b);
    return rows_check(who, m, n_cols, rowptr, col);
}

// the block columns that block row I of the blocking touches, ascending, into `out` (`mark` has one slot per block column, all -1 between calls)
void touched_blocks(int64_t I, int b, const int64_t *rowptr, const int32_t *col, std::vector<int64_t> &mark, std::vector<int32_t> &out)
{
    out.clear();
    for (int64_t q = rowptr[I * b]; q < rowptr[(I + 1) * b]; ++q) {
        const int32_t J = col[q] / b;
        if (mark[J] < 0) {
            mark[J] = 0;
            out.push_back(J);
        }
    }
    std::sort(out.begin(), out.end());
}

} // namespace

extern "C" int rails_bsr_count_host(int64_t m, int64_t n_cols, int b, const int64_t *rowptr, const int32_t *col, int64_t *nnzb)
{
    int rc = csr_check("rails_bsr_count_host", m, n_cols, b, rowptr, col);
    if (rc != RAILS_OK) return rc;
    if (!nnzb) BSR_FAIL("rails_bsr_count_host: null output");
    std::vector<int64_t> mark((size_t)(n_cols / b), -1);
    std::vector<int32_t> cols;
    int64_t total = 0;
    for (int64_t I = 0; I < m / b; ++I) {
        touched_blocks(I, b, rowptr, col, mark, cols);
        for (int32_t J : cols) mark[J] = -1;
        total += (int64_t)cols.size();
    }
    *nnzb = total;
    return RAILS_OK;
}

extern "C" int rails_bsr_fill_host(int64_t m, int64_t n_cols, int b, const int64_t *rowptr, const int32_t *col, const double *val,
                                   int64_t *browptr, int32_t *bcol, double *bval)
{
    int rc = csr_check("rails_bsr_fill_host", m, n_cols, b, rowptr, col);
    if (rc != RAILS_OK) return rc;
    if (!browptr) BSR_FAIL("rails_bsr_fill_host: null output");
    const int64_t nnz = rowptr[m];
    if (nnz > 0 && (!val || !bcol || !bval)) BSR_FAIL("rails_bsr_fill_host: null arrays with %lld entries", (long long)nnz);
    std::vector<int64_t> mark((size_t)(n_cols / b), -1);
    std::vector<int32_t> cols;
    const int bb = b * b;
    int64_t at = 0;
    browptr[0] = 0;
    for (int64_t I = 0; I < m / b; ++I) {
        touched_blocks(I, b, rowptr, col, mark, cols);
        for (size_t k = 0; k < cols.size(); ++k) {
            mark[cols[k]] = at + (int64_t)k; // where the block lies
            bcol[at + (int64_t)k] = cols[k];
        }
        std::fill(bval + at * bb, bval + (at + (int64_t)cols.size()) * bb, 0.0);
        for (int r = 0; r < b; ++r)
            for (int64_t q = rowptr[I * b + r]; q < rowptr[I * b + r + 1]; ++q)
                bval[mark[col[q] / b] * bb + r * b + col[q] % b] += val[q];
        for (int32_t J : cols) mark[J] = -1;
        at += (int64_t)cols.size();
        browptr[I + 1] = at;
    }
    return RAILS_OK;
}

extern "C" int rails_bsr_transpose_host(int64_t mb, int64_t nb, int b, const int64_t *browptr, const int32_t *bcol, const double *bval,
                                        int64_t *t_browptr, int32_t *t_bcol, double *t_bval)
{
    int rc = block_size_check("rails_bsr_transpose_host", b);
    if (rc != RAILS_OK) return rc;
    rc = rows_check("rails_bsr_transpose_host", mb, nb, browptr, bcol);
    if (rc != RAILS_OK) return rc;
    if (!t_browptr) BSR_FAIL("rails_bsr_transpose_host: null output");
    const int64_t nnzb = browptr[mb];
    if (nnzb > 0 && (!bval || !t_bcol || !t_bval)) BSR_FAIL("rails_bsr_transpose_host: null arrays with %lld blocks", (long long)nnzb);
    const int bb = b * b;
    for (int64_t j = 0; j <= nb; ++j) t_browptr[j] = 0;
    for (int64_t q = 0; q < nnzb; ++q) t_browptr[bcol[q] + 1]++;
    for (int64_t j = 0; j < nb; ++j) t_browptr[j + 1] += t_browptr[j];
    std::vector<int64_t> next(t_browptr, t_browptr + nb);
    for (int64_t i = 0; i < mb; ++i)
        for (int64_t q = browptr[i]; q < browptr[i + 1]; ++q) {
            const int64_t d = next[bcol[q]]++;
            t_bcol[d] = (int32_t)i;
            for (int r = 0; r < b; ++r)
                for (int s = 0; s < b; ++s) t_bval[d * bb + s * b + r] = bval[q * bb + r * b + s];
        }
    return RAILS_OK;
}
