// sparse_rhs_host.cpp -- the host part of the sparse right-hand side (rails_amd/csrc/sprhs_host.cpp) checked on its own: no HIP, no
// library, linked against sprhs_host.o only, so it can also be built with -fsanitize=address,undefined and run as it is.
//
// Every matrix is generated in here.  rails_csr_transpose_host is compared with a transpose made the slow way (for each column, every
// row in order, every entry in order: the definition of "stable"), ||B'B||_F^2 with the dense p x p product in long double, and the
// two kinds of bad input must come back as RAILS_EINVAL.  The output arrays of every call sit between guard words that must survive.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/rails_hip.h"

namespace {

struct Csr {
    int64_t n_rows = 0, n_cols = 0;
    std::vector<int64_t> rowptr{0};
    std::vector<int32_t> col;
    std::vector<double> val;
    void row(const std::vector<int32_t> &c)
    {
        for (int32_t x : c) {
            col.push_back(x);
            val.push_back(0.5 + 0.125 * (double)((col.size() * 37) % 29) - 1.75); // distinct, both signs
        }
        rowptr.push_back((int64_t)col.size());
        n_rows++;
    }
};

uint32_t mix(uint64_t a, uint64_t b) { return (uint32_t)(((a + 1) * 2654435761ull + (b + 7) * 40503ull + 12345ull) >> 7 & 0xffffffffull); }

// about `per_row` entries per row at hashed columns (unsorted, repeats possible); rows with i % skip_row == 1 and columns with
// j % skip_col == 2 stay empty
Csr scattered(int64_t m, int64_t p, int per_row, int skip_row, int skip_col)
{
    Csr A;
    A.n_cols = p;
    for (int64_t i = 0; i < m; ++i) {
        std::vector<int32_t> c;
        if (!(skip_row && i % skip_row == 1))
            for (int t = 0; t < per_row; ++t) {
                const int32_t j = (int32_t)(mix((uint64_t)i, (uint64_t)t) % (uint32_t)p);
                if (skip_col && j % skip_col == 2) continue;
                c.push_back(j);
            }
        A.row(c);
    }
    return A;
}

int failures = 0;
#define CHECK(cond, ...)                 \
    do {                                 \
        if (!(cond)) {                   \
            printf("  FAILED: " __VA_ARGS__); \
            printf("\n");                \
            failures++;                  \
        }                                \
    } while (0)

constexpr int64_t GI = 0x5a5a5a5a5a5a5a5aLL;
constexpr int32_t GC = 0x5b5b5b5b;
constexpr double GV = -12345.678;

struct Transposed {
    std::vector<int64_t> rowptr;
    std::vector<int32_t> col;
    std::vector<double> val;
    int rc = 0;
};

// the call, its outputs between guards (one word in front, one behind)
Transposed transpose(const Csr &A)
{
    const int64_t nnz = A.rowptr.back();
    std::vector<int64_t> rp((size_t)A.n_cols + 3, GI);
    std::vector<int32_t> ci((size_t)nnz + 2, GC);
    std::vector<double> va((size_t)nnz + 2, GV);
    Transposed T;
    T.rc = rails_csr_transpose_host(A.n_rows, A.n_cols, A.rowptr.data(), A.col.data(), A.val.data(), rp.data() + 1, ci.data() + 1, va.data() + 1);
    CHECK(rp.front() == GI && rp.back() == GI && ci.front() == GC && ci.back() == GC && va.front() == GV && va.back() == GV, "a guard word was overwritten");
    T.rowptr.assign(rp.begin() + 1, rp.end() - 1);
    T.col.assign(ci.begin() + 1, ci.end() - 1);
    T.val.assign(va.begin() + 1, va.end() - 1);
    return T;
}

void check_matrix(const std::string &name, const Csr &A)
{
    printf("CASE %s: %lld x %lld, %lld entries\n", name.c_str(), (long long)A.n_rows, (long long)A.n_cols, (long long)A.rowptr.back());
    const int before = failures;
    Transposed T = transpose(A);
    CHECK(T.rc == RAILS_OK, "transpose returned %d", T.rc);
    if (T.rc != RAILS_OK) return;
    // the slow transpose
    std::vector<int64_t> rp{0};
    std::vector<int32_t> ci;
    std::vector<double> va;
    for (int64_t j = 0; j < A.n_cols; ++j) {
        for (int64_t i = 0; i < A.n_rows; ++i)
            for (int64_t q = A.rowptr[i]; q < A.rowptr[i + 1]; ++q)
                if (A.col[q] == j) {
                    ci.push_back((int32_t)i);
                    va.push_back(A.val[q]);
                }
        rp.push_back((int64_t)ci.size());
    }
    CHECK(T.rowptr == rp, "row pointers differ");
    CHECK(T.col == ci, "row indices differ (order of a transposed row)");
    CHECK(T.val == va, "values differ (duplicates keep their order)");
    // ||B'B||_F^2 against the dense product
    const int64_t p = A.n_cols, m = A.n_rows;
    std::vector<long double> D((size_t)(m * p), 0.0L);
    for (int64_t i = 0; i < m; ++i)
        for (int64_t q = A.rowptr[i]; q < A.rowptr[i + 1]; ++q) D[(size_t)(i * p + A.col[q])] += A.val[q];
    long double ref = 0.0L;
    for (int64_t a = 0; a < p; ++a)
        for (int64_t b = 0; b < p; ++b) {
            long double g = 0.0L;
            for (int64_t i = 0; i < m; ++i) g += D[(size_t)(i * p + a)] * D[(size_t)(i * p + b)];
            ref += g * g;
        }
    double got = -1.0;
    const int rc = rails_csr_gram_norm2_host(m, p, A.rowptr.data(), A.col.data(), A.val.data(), T.rowptr.data(), T.col.data(), T.val.data(), &got);
    CHECK(rc == RAILS_OK, "gram norm returned %d", rc);
    CHECK(fabsl((long double)got - ref) <= 1e-13L * ref, "||B'B||_F^2 = %.17g, dense reference %.17Lg", got, ref);
    if (failures == before) printf("PASS %s\n", name.c_str());
}

void check_refused(const std::string &name, const Csr &A)
{
    printf("CASE %s\n", name.c_str());
    const int before = failures;
    Transposed T = transpose(A);
    CHECK(T.rc == RAILS_EINVAL, "transpose returned %d, expected RAILS_EINVAL", T.rc);
    double got = 0.0;
    Csr Z; // a valid transposed form of the right shape with no entries, so that only A can be what is refused
    Z.rowptr.assign((size_t)A.n_cols + 1, 0);
    const int rc = rails_csr_gram_norm2_host(A.n_rows, A.n_cols, A.rowptr.data(), A.col.data(), A.val.data(), Z.rowptr.data(), nullptr, nullptr, &got);
    CHECK(rc == RAILS_EINVAL, "gram norm returned %d, expected RAILS_EINVAL", rc);
    if (failures == before) printf("PASS %s\n", name.c_str());
}

} // namespace

int main()
{
    check_matrix("tall", scattered(300, 40, 3, 0, 0));
    check_matrix("wide", scattered(40, 300, 5, 0, 0));
    check_matrix("empty_rows_cols", scattered(257, 65, 4, 3, 5));
    {
        Csr A;
        A.n_cols = 7;
        for (int i = 0; i < 20; ++i) A.row({});
        check_matrix("nnz0", A);
    }
    {
        Csr A;
        A.n_cols = 0;
        for (int i = 0; i < 9; ++i) A.row({});
        check_matrix("p0", A);
    }
    {
        Csr A;
        A.n_cols = 4;
        A.row({2, 2, 0, 2});
        A.row({});
        A.row({3, 2, 2, 0, 0});
        A.row({1, 1});
        check_matrix("duplicates", A);
    }
    {
        Csr A; // one dense row and one dense column
        A.n_cols = 90;
        for (int i = 0; i < 130; ++i) {
            std::vector<int32_t> c{0};
            if (i == 77)
                for (int j = 1; j < 90; ++j) c.push_back(j);
            A.row(c);
        }
        check_matrix("dense_row_and_column", A);
    }
    {
        Csr A = scattered(50, 10, 3, 0, 0);
        A.col[17] = 10;
        check_refused("column_out_of_range", A);
        A.col[17] = -1;
        check_refused("column_negative", A);
    }
    {
        Csr A = scattered(50, 10, 3, 0, 0);
        A.rowptr[20] = A.rowptr[19] - 1;
        check_refused("rowptr_not_monotone", A);
        Csr B2 = scattered(50, 10, 3, 0, 0);
        B2.rowptr[0] = 1;
        check_refused("rowptr_not_from_zero", B2);
    }
    if (failures) {
        printf("%d FAILED\n", failures);
        return 1;
    }
    printf("ALL PASSED\n");
    return 0;
}
