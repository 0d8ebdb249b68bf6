// amg_host.cpp -- the host set-up of the smoothed-aggregation multigrid preconditioner (rails_amd/csrc/amg_host.cpp) on its own: no HIP,
// no library, linked against amg_host.o, sprhs_host.o and host_lapack.o only, so it can also be built with -fsanitize=address,undefined
// and run as it is.  Run by tests/test_amg_host.py.
//
//   amg_host dump IN OUT THETA COARSE   builds the hierarchy of the matrix in IN twice, requires the two to be the same bytes, and writes
//                                       it to OUT for the test to compare with tests/amg_reference.py.  IN: int64 n, int64 nnz, rowptr
//                                       (int64), col (int32), val (double).  OUT: see dump() below.  A refusal prints its message and
//                                       exits with 3.
//   amg_host rules                      the stop rules, the 1024 cap and every input refusal on matrices made in here, whose arrays are
//                                       exactly as long as they claim (a read out of range is the sanitizer's to find)
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/rails_hip.h"
#include "../../rails_amd/csrc/amg_host.h"

static char g_message[512] = "";
void rails_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(g_message, sizeof g_message, fmt, ap);
    va_end(ap);
}

namespace {

int failures = 0, checks = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        ++checks;                             \
        if (!(cond)) {                        \
            printf("  FAILED: " __VA_ARGS__); \
            printf("\n");                     \
            failures++;                       \
        }                                     \
    } while (0)

struct Csr {
    int64_t n = 0;
    std::vector<int64_t> rowptr{0};
    std::vector<int32_t> col;
    std::vector<double> val;
    void entry(int64_t j, double v)
    {
        col.push_back((int32_t)j);
        val.push_back(v);
    }
    void end_row()
    {
        rowptr.push_back((int64_t)col.size());
        n++;
    }
};

// 1D chain: -1 2 -1 times `sign`
Csr chain(int64_t n, double sign)
{
    Csr A;
    for (int64_t i = 0; i < n; ++i) {
        if (i > 0) A.entry(i - 1, -sign);
        A.entry(i, 2.0 * sign);
        if (i + 1 < n) A.entry(i + 1, -sign);
        A.end_row();
    }
    return A;
}

Csr diagonal(int64_t n)
{
    Csr A;
    for (int64_t i = 0; i < n; ++i) {
        A.entry(i, 1.0 + (double)(i % 7));
        A.end_row();
    }
    return A;
}

int build(const Csr &A, double theta, int coarse, rails_amg_hierarchy *h)
{
    g_message[0] = 0;
    return rails_amg_build_host(A.n, A.rowptr.data(), A.col.data(), A.val.data(), theta, coarse, h);
}

template <class T>
void put(std::string &s, const std::vector<T> &v)
{
    s.append(reinterpret_cast<const char *>(v.data()), v.size() * sizeof(T));
}
void put64(std::string &s, int64_t v) { s.append(reinterpret_cast<const char *>(&v), sizeof v); }
void putd(std::string &s, double v) { s.append(reinterpret_cast<const char *>(&v), sizeof v); }
void put_csr(std::string &s, const rails_amg_csr &M)
{
    put64(s, M.n_rows);
    put64(s, M.n_cols);
    put64(s, M.nnz());
    put(s, M.rowptr);
    put(s, M.col);
    put(s, M.val);
}

// levels (int64), defsign (double); per level: A, P, R (each: rows, cols, nnz as int64, rowptr int64, col int32, val double), dinv
// (double x rows), hi (double), agg (int32 x rows); then the last matrix and its inverse (double x rows^2, column-major)
std::string dump(const rails_amg_hierarchy &h)
{
    std::string s;
    put64(s, (int64_t)h.levels.size());
    putd(s, h.defsign);
    for (const rails_amg_level &L : h.levels) {
        put_csr(s, L.A);
        put_csr(s, L.P);
        put_csr(s, L.R);
        put(s, L.dinv);
        putd(s, L.hi);
        put(s, L.agg);
    }
    put_csr(s, h.coarse);
    put(s, h.coarse_inv);
    return s;
}

int run_dump(const char *in, const char *out, double theta, int coarse)
{
    FILE *f = fopen(in, "rb");
    if (!f) {
        printf("cannot open %s\n", in);
        return 2;
    }
    int64_t head[2] = {0, 0};
    Csr A;
    bool ok = fread(head, sizeof(int64_t), 2, f) == 2 && head[0] >= 0 && head[1] >= 0 && head[0] < (1 << 28) && head[1] < (1 << 30);
    if (ok) {
        A.n = head[0];
        A.rowptr.resize((size_t)head[0] + 1);
        A.col.resize((size_t)head[1]);
        A.val.resize((size_t)head[1]);
        ok = fread(A.rowptr.data(), sizeof(int64_t), A.rowptr.size(), f) == A.rowptr.size() && fread(A.col.data(), sizeof(int32_t), A.col.size(), f) == A.col.size() &&
             fread(A.val.data(), sizeof(double), A.val.size(), f) == A.val.size();
    }
    fclose(f);
    if (!ok) {
        printf("short or bad input file %s\n", in);
        return 2;
    }
    rails_amg_hierarchy h1, h2;
    const int rc = build(A, theta, coarse, &h1);
    if (rc != RAILS_OK) {
        printf("refused (%d): %s\n", rc, g_message);
        return 3;
    }
    if (build(A, theta, coarse, &h2) != RAILS_OK) {
        printf("the second build failed: %s\n", g_message);
        return 1;
    }
    const std::string s1 = dump(h1), s2 = dump(h2);
    if (s1 != s2) {
        printf("two builds differ\n");
        return 1;
    }
    f = fopen(out, "wb");
    if (!f || fwrite(s1.data(), 1, s1.size(), f) != s1.size()) {
        printf("cannot write %s\n", out);
        return 2;
    }
    fclose(f);
    printf("levels %d, %zu bytes, two builds identical\n", (int)h1.levels.size(), s1.size());
    return 0;
}

bool refused(const Csr &A, double theta, int coarse, const char *word)
{
    rails_amg_hierarchy h;
    const int rc = build(A, theta, coarse, &h);
    return rc == RAILS_EINVAL && std::strstr(g_message, word) != nullptr;
}

int run_rules()
{
    rails_amg_hierarchy h;
    // ---- the stop rules
    printf("stop rules\n");
    {
        Csr one;
        one.entry(0, -3.0);
        one.end_row();
        CHECK(build(one, 0.08, 256, &h) == RAILS_OK && h.levels.empty() && h.coarse.n_rows == 1 && h.coarse_inv.size() == 1 && std::fabs(h.coarse_inv[0] + 1.0 / 3.0) <= 1e-15 && h.defsign == -1.0,
              "a 1-row matrix is the dense inverse alone: %s", g_message);
        const Csr c40 = chain(40, 1.0);
        CHECK(build(c40, 0.08, 40, &h) == RAILS_OK && h.levels.empty() && h.coarse.n_rows == 40, "n <= coarse: no level (%s)", g_message);
        CHECK(build(c40, 0.08, 39, &h) == RAILS_OK && h.levels.size() >= 1 && h.levels[0].A.n_rows == 40 && h.coarse.n_rows <= 39, "n = coarse + 1: a level (%s)", g_message);
        for (size_t l = 0; l < h.levels.size(); ++l) {
            const int64_t next = l + 1 < h.levels.size() ? h.levels[l + 1].A.n_rows : h.coarse.n_rows;
            CHECK(h.levels[l].P.n_cols == next && next * 5 <= h.levels[l].A.n_rows * 4, "level %zu keeps %lld of %lld rows", l, (long long)next, (long long)h.levels[l].A.n_rows);
        }
        // a chain of 1000 with coarse 1 goes down in threes until a level would keep too many rows or one row is left; never past 16
        const Csr c1000 = chain(1000, -1.0);
        CHECK(build(c1000, 0.08, 1, &h) == RAILS_OK && h.levels.size() >= 3 && (int)h.levels.size() + 1 <= RAILS_AMG_MAX_LEVELS && h.defsign == -1.0, "chain of 1000: %s", g_message);
        // the dense inverse is an inverse: A_L Ainv = I
        const int64_t nl = h.coarse.n_rows;
        double worst = 0.0;
        for (int64_t i = 0; i < nl; ++i)
            for (int64_t j = 0; j < nl; ++j) {
                long double s = 0.0L;
                for (int64_t q = h.coarse.rowptr[i]; q < h.coarse.rowptr[i + 1]; ++q) s += (long double)h.coarse.val[q] * h.coarse_inv[(size_t)h.coarse.col[q] + (size_t)j * nl];
                worst = std::fmax(worst, std::fabs((double)(s - (i == j ? 1.0L : 0.0L))));
            }
        CHECK(worst <= 1e-12, "A_L Ainv - I is %g", worst);
        // no strong neighbour anywhere: every row a singleton, the level would keep all its rows, so there is none
        const Csr d300 = diagonal(300);
        CHECK(build(d300, 0.08, 256, &h) == RAILS_OK && h.levels.empty() && h.coarse.n_rows == 300, "a diagonal matrix of 300 rows: one dense block (%s)", g_message);
        // ... and above 1024 rows that is refused: no huge dense block
        CHECK(refused(diagonal(1025), 0.08, 256, "does not coarsen"), "a diagonal matrix of 1025 rows: %s", g_message);
        CHECK(build(diagonal(1024), 0.08, 256, &h) == RAILS_OK && h.coarse.n_rows == 1024, "a diagonal matrix of 1024 rows: %s", g_message);
    }
    // ---- the refusals
    printf("refusals\n");
    const Csr good = chain(30, 1.0);
    CHECK(build(good, 0.08, 8, &h) == RAILS_OK, "the matrix the bad ones are made from: %s", g_message);
    CHECK(rails_amg_build_host(good.n, good.rowptr.data(), good.col.data(), good.val.data(), 0.08, 8, nullptr) == RAILS_EINVAL, "null output");
    CHECK(rails_amg_build_host(good.n, nullptr, good.col.data(), good.val.data(), 0.08, 8, &h) == RAILS_EINVAL, "null rowptr");
    CHECK(rails_amg_build_host(good.n, good.rowptr.data(), nullptr, good.val.data(), 0.08, 8, &h) == RAILS_EINVAL, "null col");
    CHECK(rails_amg_build_host(good.n, good.rowptr.data(), good.col.data(), nullptr, 0.08, 8, &h) == RAILS_EINVAL, "null val");
    CHECK(rails_amg_build_host(0, good.rowptr.data(), good.col.data(), good.val.data(), 0.08, 8, &h) == RAILS_EINVAL, "no rows");
    CHECK(rails_amg_build_host(-4, good.rowptr.data(), good.col.data(), good.val.data(), 0.08, 8, &h) == RAILS_EINVAL, "negative size");
    for (double theta : {-0.1, 1.0, 2.0, std::numeric_limits<double>::quiet_NaN()}) CHECK(refused(good, theta, 8, "theta"), "theta %g", theta);
    for (int coarse : {0, -1, 1025}) CHECK(refused(good, 0.08, coarse, "coarse"), "coarse %d", coarse);
    {
        Csr b = good;
        b.rowptr[0] = 1;
        CHECK(refused(b, 0.08, 8, "rowptr[0]"), "rowptr[0] = 1: %s", g_message);
        b = good;
        b.rowptr[5] = b.rowptr[4] - 1;
        CHECK(refused(b, 0.08, 8, "monotone"), "decreasing rowptr: %s", g_message);
        b = good;
        b.col[7] = 30;
        CHECK(refused(b, 0.08, 8, "out of range"), "column n: %s", g_message);
        b = good;
        b.col[7] = -1;
        CHECK(refused(b, 0.08, 8, "out of range"), "column -1: %s", g_message);
        b = good;
        std::swap(b.col[3], b.col[4]);
        CHECK(refused(b, 0.08, 8, "strictly increasing"), "unsorted columns: %s", g_message);
        b = good;
        b.col[4] = b.col[3];
        CHECK(refused(b, 0.08, 8, "strictly increasing"), "a repeated column: %s", g_message);
        b = good;
        b.val[6] = std::numeric_limits<double>::infinity();
        CHECK(refused(b, 0.08, 8, "not finite"), "an infinite entry: %s", g_message);
        b = good;
        b.val[b.rowptr[10] + 1] = 0.0; // the diagonal of row 10
        CHECK(refused(b, 0.08, 8, "diagonal"), "a zero diagonal entry: %s", g_message);
        b = good;
        b.val[b.rowptr[10] + 1] = std::numeric_limits<double>::quiet_NaN();
        CHECK(refused(b, 0.08, 8, "not finite"), "a NaN diagonal entry: %s", g_message);
        // a missing diagonal entry: row 2 of a chain without its middle
        Csr c;
        for (int64_t i = 0; i < 6; ++i) {
            if (i > 0) c.entry(i - 1, -1.0);
            if (i != 2) c.entry(i, 2.0);
            if (i + 1 < 6) c.entry(i + 1, -1.0);
            c.end_row();
        }
        CHECK(refused(c, 0.08, 2, "missing"), "a missing diagonal entry: %s", g_message);
        b = good;
        b.val[b.rowptr[10] + 1] = -2.0;
        CHECK(refused(b, 0.08, 8, "not definite"), "diagonal entries of both signs: %s", g_message);
        // positive diagonal, indefinite: 1 3; 3 1 (a dense block at once) and inside a chain (found at the coarsest level)
        Csr ind;
        ind.entry(0, 1.0);
        ind.entry(1, 3.0);
        ind.end_row();
        ind.entry(0, 3.0);
        ind.entry(1, 1.0);
        ind.end_row();
        CHECK(refused(ind, 0.08, 8, "not definite"), "an indefinite 2 x 2 matrix: %s", g_message);
        Csr ns = ind;
        ns.val[1] = 0.25;
        ns.val[2] = -0.25;
        CHECK(refused(ns, 0.08, 8, "not symmetric"), "a matrix that is not symmetric: %s", g_message);
    }
    printf("%d checks, %d failed\n", checks, failures);
    return failures ? 1 : 0;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc == 6 && std::string(argv[1]) == "dump") return run_dump(argv[2], argv[3], atof(argv[4]), atoi(argv[5]));
    if (argc == 2 && std::string(argv[1]) == "rules") return run_rules();
    printf("usage: amg_host dump IN OUT THETA COARSE | amg_host rules\n");
    return 2;
}
