// block_amg_host.cpp -- the host set-up of the block multigrid preconditioner (rails_amd/csrc/block_amg_host.cpp) and the launch decision
// of its cycle (block_amg_choice.h) on their own: no HIP, no library, linked against block_amg_host.o, amg_host.o, block_jacobi_host.o,
// bsr_host.o, sprhs_host.o and host_lapack.o only, so it is also built with -fsanitize=address,undefined and run as it is.  Run by
// tests/test_block_amg_host.py.
//
//   block_amg_host dump IN OUT THETA COARSE   builds the hierarchy of the block matrix in IN twice, requires the two to be the same bytes,
//                                             and writes it to OUT for the test to compare with tests/block_amg_reference.py.  IN: int64
//                                             mb, b, nnzb; browptr (int64), bcol (int32), bval (double).  OUT: see dump() below.  A
//                                             refusal prints its message and exits with 3.
//   block_amg_host rules                      every input refusal and the stop rules on matrices made in here, whose arrays are exactly
//                                             as long as they claim (a read out of range is the sanitizer's to find)
//   block_amg_host choice                     the launch decision over its whole range, one line per case, for the Python restatement
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
#include "../../rails_amd/csrc/block_amg_choice.h"
#include "../../rails_amd/csrc/block_amg_host.h"

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

struct Bsr {
    int b = 2;
    int64_t mb = 0;
    std::vector<int64_t> browptr{0};
    std::vector<int32_t> bcol;
    std::vector<double> bval;
    // a block s I + t (ones off the diagonal)
    void block(int64_t j, double s, double t)
    {
        bcol.push_back((int32_t)j);
        for (int r = 0; r < b; ++r)
            for (int c = 0; c < b; ++c) bval.push_back(r == c ? s : t);
    }
    void end_row()
    {
        browptr.push_back((int64_t)bcol.size());
        mb++;
    }
};

// a chain of cells: diagonal blocks sign (4 I + 0.5 offdiag), neighbours -sign I
Bsr chain(int64_t mb, int b, double sign)
{
    Bsr A;
    A.b = b;
    for (int64_t i = 0; i < mb; ++i) {
        if (i > 0) A.block(i - 1, -sign, 0.0);
        A.block(i, 4.0 * sign, 0.5 * sign);
        if (i + 1 < mb) A.block(i + 1, -sign, 0.0);
        A.end_row();
    }
    return A;
}

int build(const Bsr &A, double theta, int coarse, rails_bamg_hierarchy *h)
{
    g_message[0] = 0;
    return rails_bamg_build_host(A.mb, A.b, A.browptr.data(), A.bcol.data(), A.bval.data(), theta, coarse, h);
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
void put_bsr(std::string &s, const rails_bamg_bsr &M)
{
    put64(s, M.mb);
    put64(s, M.nnzb());
    put(s, M.browptr);
    put(s, M.bcol);
    put(s, M.bval);
}

// levels, b (int64), defsign (double); per level: A (mb, nnzb as int64, browptr int64, bcol int32, bval double), P, R (each: rows, cols,
// nnz as int64, rowptr int64, col int32, val double), ginv (double x mb b b), hi (double), agg (int32 x mb); then the last matrix (as A)
// and its inverse (double x rows^2, column-major)
std::string dump(const rails_bamg_hierarchy &h)
{
    std::string s;
    put64(s, (int64_t)h.levels.size());
    put64(s, h.b);
    putd(s, h.defsign);
    for (const rails_bamg_level &L : h.levels) {
        put_bsr(s, L.A);
        put_csr(s, L.P);
        put_csr(s, L.R);
        put(s, L.ginv);
        putd(s, L.hi);
        put(s, L.agg);
    }
    put_bsr(s, h.coarse);
    put(s, h.coarse_inv);
    return s;
}

bool read_file(const char *path, std::string &raw)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) raw.append(buf, n);
    fclose(f);
    return true;
}

bool write_file(const char *path, const std::string &s)
{
    FILE *f = fopen(path, "wb");
    if (!f) return false;
    const bool ok = fwrite(s.data(), 1, s.size(), f) == s.size();
    fclose(f);
    return ok;
}

int run_dump(const char *in, const char *out, double theta, int coarse)
{
    std::string raw;
    if (!read_file(in, raw) || raw.size() < 24) {
        printf("cannot read %s\n", in);
        return 2;
    }
    int64_t head[3];
    memcpy(head, raw.data(), sizeof head);
    Bsr A;
    A.mb = head[0];
    A.b = (int)head[1];
    const int64_t nnzb = head[2];
    const size_t want = 24 + (size_t)(A.mb + 1) * 8 + (size_t)nnzb * 4 + (size_t)nnzb * A.b * A.b * 8;
    if (A.mb < 0 || nnzb < 0 || A.b < 1 || A.b > 64 || raw.size() != want) {
        printf("%s: %zu bytes, %zu expected\n", in, raw.size(), want);
        return 2;
    }
    A.browptr.resize((size_t)A.mb + 1);
    A.bcol.resize((size_t)nnzb);
    A.bval.resize((size_t)nnzb * A.b * A.b);
    const char *p = raw.data() + 24;
    memcpy(A.browptr.data(), p, A.browptr.size() * 8);
    p += A.browptr.size() * 8;
    if (nnzb) memcpy(A.bcol.data(), p, A.bcol.size() * 4);
    p += A.bcol.size() * 4;
    if (nnzb) memcpy(A.bval.data(), p, A.bval.size() * 8);
    rails_bamg_hierarchy h1, h2;
    if (build(A, theta, coarse, &h1) != RAILS_OK) {
        printf("refused: %s\n", g_message);
        return 3;
    }
    if (build(A, theta, coarse, &h2) != RAILS_OK || dump(h1) != dump(h2)) {
        printf("two builds differ\n");
        return 1;
    }
    printf("two builds identical\n");
    return write_file(out, dump(h1)) ? 0 : 2;
}

void refused(const Bsr &A, double theta, int coarse, const char *needle, const char *what)
{
    rails_bamg_hierarchy h;
    const int rc = build(A, theta, coarse, &h);
    CHECK(rc == RAILS_EINVAL && strstr(g_message, needle), "%s: code %d, message '%s' (wanted '%s')", what, rc, g_message, needle);
}

int run_rules()
{
    rails_bamg_hierarchy h;
    // a chain of 40 cells coarsens; every level's rows are a multiple of b; the aggregates cover every cell
    for (int b = 2; b <= 8; ++b) {
        Bsr A = chain(40, b, b % 2 ? 1.0 : -1.0);
        CHECK(build(A, 0.08, 16, &h) == RAILS_OK, "chain, b = %d: %s", b, g_message);
        CHECK(!h.levels.empty() && h.defsign == (b % 2 ? 1.0 : -1.0), "chain, b = %d: %d levels, sign %g", b, (int)h.levels.size(), h.defsign);
        for (const rails_bamg_level &L : h.levels) {
            CHECK(L.P.n_rows == L.A.mb * b && L.P.n_cols % b == 0 && L.R.n_rows == L.P.n_cols, "chain, b = %d: shapes", b);
            CHECK((int64_t)L.agg.size() == L.A.mb && (int64_t)L.ginv.size() == L.A.mb * b * b && L.hi > 0.0, "chain, b = %d: level arrays", b);
        }
        CHECK(h.coarse.mb * b <= 16 && (int64_t)h.coarse_inv.size() == h.coarse.mb * b * h.coarse.mb * b, "chain, b = %d: the last matrix", b);
    }
    // one block row: no level, the dense inverse alone
    {
        Bsr A = chain(1, 3, 1.0);
        CHECK(build(A, 0.08, 256, &h) == RAILS_OK && h.levels.empty() && h.coarse_inv.size() == 9, "one block row: %s", g_message);
    }
    // the stop at RAILS_AMG_MAX_LEVELS and the rule of 0.8 are the scalar set-up's; the cap of 1024 rows
    {
        Bsr A;
        A.b = 2;
        for (int64_t i = 0; i < 600; ++i) {
            A.block(i, 1.0 + (double)(i % 5), 0.0);
            A.end_row();
        }
        refused(A, 0.08, 256, "does not coarsen", "a block-diagonal matrix of 1200 rows");
    }
    const double nan = std::numeric_limits<double>::quiet_NaN();
    {
        Bsr A = chain(6, 2, 1.0);
        refused(A, 1.0, 16, "theta", "theta = 1");
        refused(A, 0.08, 0, "coarse", "coarse = 0");
        refused(A, 0.08, 2000, "coarse", "coarse = 2000");
        rails_bamg_hierarchy *none = nullptr;
        g_message[0] = 0;
        CHECK(rails_bamg_build_host(A.mb, A.b, A.browptr.data(), A.bcol.data(), A.bval.data(), 0.08, 16, none) == RAILS_EINVAL, "null output");
        Bsr B = A;
        B.b = 9;
        refused(B, 0.08, 16, "block size", "b = 9");
        B = A;
        B.browptr[0] = 1;
        refused(B, 0.08, 16, "browptr[0]", "browptr[0] = 1");
        B = A;
        B.browptr[2] = B.browptr[1] - 1;
        refused(B, 0.08, 16, "not monotone", "browptr not monotone");
        B = A;
        B.bcol[1] = 77;
        refused(B, 0.08, 16, "out of range", "a block column out of range");
        B = A;
        std::swap(B.bcol[0], B.bcol[1]);
        refused(B, 0.08, 16, "not strictly increasing", "unsorted block columns");
        B = A;
        B.bcol[1] = B.bcol[0];
        refused(B, 0.08, 16, "not strictly increasing", "a repeated block column");
        B = A;
        B.bval[5] = nan;
        refused(B, 0.08, 16, "not finite", "a NaN entry");
        B = A;
        B.bval[(size_t)B.browptr[1] * 4 + 4 + 1] = std::numeric_limits<double>::infinity();
        refused(B, 0.08, 16, "not finite", "an infinite entry");
    }
    {
        // block row 2 without its diagonal block
        Bsr A;
        A.b = 2;
        for (int64_t i = 0; i < 4; ++i) {
            if (i > 0) A.block(i - 1, -1.0, 0.0);
            if (i != 2) A.block(i, 4.0, 0.5);
            if (i + 1 < 4) A.block(i + 1, -1.0, 0.0);
            A.end_row();
        }
        refused(A, 0.08, 2, "no stored diagonal block", "a missing diagonal block");
    }
    {
        Bsr A = chain(6, 2, 1.0);
        Bsr B = A;
        B.bval[(size_t)B.browptr[2] * 4 + 4] = 0.0; // the (0, 0) entry of the diagonal block of block row 2 (its second block)
        refused(B, 0.08, 2, "zero or not finite", "a zero on the scalar diagonal");
        B = A;
        B.bval[(size_t)B.browptr[2] * 4 + 4] = -4.0;
        refused(B, 0.08, 2, "both signs", "a diagonal block of mixed sign");
        B = A;
        for (int e = 0; e < 4; ++e) B.bval[(size_t)B.browptr[2] * 4 + 4 + e] *= -1.0;
        refused(B, 0.08, 2, "both signs", "signs that differ between blocks");
        B = A;
        for (int e = 0; e < 4; ++e) B.bval[(size_t)B.browptr[2] * 4 + 4 + e] = 1.0; // [[1, 1], [1, 1]]: singular
        refused(B, 0.08, 2, "diagonal block 2", "a singular diagonal block");
    }
    {
        // symmetric, positive diagonal, indefinite: [[1, 3], [3, 1]] blocks on the diagonal of one block row
        Bsr A;
        A.b = 2;
        A.block(0, 1.0, 3.0);
        A.end_row();
        refused(A, 0.08, 16, "not definite", "an indefinite last matrix");
    }
    printf("%d checks, %d failed\n", checks, failures);
    return failures ? 1 : 0;
}

// b nc mb max_brow ld want_fused -> ok fused lpr threads rpg grid lds; and rows_ok over its edges
int run_choice()
{
    const int64_t mbs[] = {1, 7, 31, 32, 33, 48, 255, 256, 1000, 4097, 262144, 1 << 21};
    const int64_t brows[] = {0, 1, 7, 27, 64, 65, 300};
    const int ncs[] = {1, 2, 3, 15, 16, 17, 31, 32, 33};
    for (int b = 1; b <= 9; ++b)
        for (int nc : ncs)
            for (int64_t mb : mbs)
                for (int64_t mx : brows)
                    for (int want = 0; want < 2; ++want)
                        for (int ld : {nc, nc + 1, 34}) {
                            BsrFacts f;
                            f.b = b; f.nc = nc; f.mb = mb; f.max_brow = mx; f.num_cu = 256;
                            f.ldx = f.ldy = ld;
                            const BamgStep s = rails_bamg_step(f, want != 0);
                            printf("step %d %d %lld %lld %d %d -> %d %d %d %d %d %lld %d\n", b, nc, (long long)mb, (long long)mx, ld, want, s.ok ? 1 : 0, s.fused ? 1 : 0,
                                   s.ok ? s.k.lpr : 0, s.ok ? s.k.threads : 0, s.ok ? s.k.rpg : 0, s.ok ? (long long)s.k.grid : 0LL, s.lds_bytes);
                        }
    const int64_t ms[] = {0, 1, 2, 3, 8, 9, 24, (1 << 24) - 8, (1 << 24) - 1, 1 << 24, (int64_t)1 << 31};
    for (int b = 1; b <= 9; ++b)
        for (int64_t m : ms) printf("rows %lld %d -> %d\n", (long long)m, b, rails_bamg_rows_ok(m, b) ? 1 : 0);
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc == 6 && !strcmp(argv[1], "dump")) return run_dump(argv[2], argv[3], atof(argv[4]), atoi(argv[5]));
    if (argc == 2 && !strcmp(argv[1], "rules")) return run_rules();
    if (argc == 2 && !strcmp(argv[1], "choice")) return run_choice();
    printf("usage: block_amg_host dump IN OUT THETA COARSE | rules | choice\n");
    return 2;
}
