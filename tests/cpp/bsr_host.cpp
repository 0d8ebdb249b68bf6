// The host part of the block-CSR operator alone: rails_bsr_count_host / rails_bsr_fill_host / rails_bsr_transpose_host
// (rails_amd/csrc/bsr_host.cpp) against a dense reference, their refusals, and the launch rule of the kernel (rails_amd/csrc/bsr_choice.h).
// No HIP, no library.  `--table` prints, one JSON line per instantiation of RAILS_BSR_TABLE, the smallest shape that reaches it.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "bsr_choice.h"
#include "rails_hip.h"

// the library's error text, kept here: this program links bsr_host.o alone
static char g_error[512] = "";
void rails_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
}

static long n_checks = 0, n_failed = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        ++n_checks;                                       \
        if (!(cond)) {                                    \
            ++n_failed;                                   \
            if (n_failed <= 20) {                         \
                printf("FAILED %s:%d: ", __FILE__, __LINE__); \
                printf(__VA_ARGS__);                      \
                printf("\n");                             \
            }                                             \
        }                                                 \
    } while (0)

struct Csr {
    int64_t m = 0, n = 0;
    std::vector<int64_t> rowptr;
    std::vector<int32_t> col;
    std::vector<double> val;
};
struct Bsr {
    int64_t mb = 0, nb = 0;
    int b = 0;
    std::vector<int64_t> browptr;
    std::vector<int32_t> bcol;
    std::vector<double> bval;
};

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// dense m x n, entries added in stored order; touched[i * n + j]: the b x b block of (i, j) holds an entry
static void dense_of(const Csr &A, int b, std::vector<double> &D, std::vector<char> &touched)
{
    D.assign((size_t)(A.m * A.n), 0.0);
    touched.assign((size_t)((A.m / b) * (A.n / b)), 0);
    for (int64_t i = 0; i < A.m; ++i)
        for (int64_t q = A.rowptr[i]; q < A.rowptr[i + 1]; ++q) {
            D[(size_t)(i * A.n + A.col[q])] += A.val[q];
            touched[(size_t)((i / b) * (A.n / b) + A.col[q] / b)] = 1;
        }
}

static int convert(const Csr &A, int b, Bsr &S)
{
    int64_t nnzb = -1;
    int rc = rails_bsr_count_host(A.m, A.n, b, A.rowptr.data(), A.col.data(), &nnzb);
    if (rc != RAILS_OK) return rc;
    S.mb = A.m / b;
    S.nb = A.n / b;
    S.b = b;
    S.browptr.assign((size_t)S.mb + 1, -7);
    S.bcol.assign((size_t)nnzb, -7);
    S.bval.assign((size_t)nnzb * b * b, -7.0); // (exactly as many as counted: the sanitizers see a write past them)
    rc = rails_bsr_fill_host(A.m, A.n, b, A.rowptr.data(), A.col.data(), A.val.data(), S.browptr.data(), S.bcol.data(), S.bval.data());
    if (rc == RAILS_OK) CHECK(S.browptr[(size_t)S.mb] == nnzb, "fill made %lld blocks, count said %lld", (long long)S.browptr[(size_t)S.mb], (long long)nnzb);
    return rc;
}

// a random matrix of mb x nb blocks: block row 0 has one block, block row 1 all nb of them, block rows 2 and mb - 1 none, the others a
// few; inside a touched block a random subset of entries; columns of a row shuffled (unsorted); duplicates with `dups`
static Csr random_csr(int b, int64_t mb, int64_t nb, bool shuffle, bool dups, unsigned seed)
{
    std::mt19937 g(seed);
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    Csr A;
    A.m = mb * b;
    A.n = nb * b;
    A.rowptr.push_back(0);
    for (int64_t I = 0; I < mb; ++I) {
        std::vector<int32_t> blocks;
        if (I == 0)
            blocks.push_back((int32_t)(g() % nb));
        else if (I == 1)
            for (int64_t J = 0; J < nb; ++J) blocks.push_back((int32_t)J);
        else if (I != 2 && I != mb - 1)
            for (int64_t J = 0; J < nb; ++J)
                if (g() % 4 == 0) blocks.push_back((int32_t)J);
        for (int r = 0; r < b; ++r) {
            std::vector<int32_t> c;
            for (int32_t J : blocks)
                for (int s = 0; s < b; ++s)
                    if (g() % 3 != 0 || (r == 0 && s == 0)) c.push_back(J * b + s); // (entry (0, 0) always: the block is touched)
            if (dups)
                for (size_t k = 0, n0 = c.size(); k < n0; k += 3) c.push_back(c[k]);
            if (shuffle)
                for (size_t k = c.size(); k > 1; --k) std::swap(c[k - 1], c[g() % k]);
            for (int32_t j : c) {
                A.col.push_back(j);
                A.val.push_back(u(g));
            }
            A.rowptr.push_back((int64_t)A.col.size());
        }
    }
    return A;
}

static void test_conversion()
{
    for (int b = 2; b <= 8; ++b)
        for (int variant = 0; variant < 4; ++variant) {
            const bool shuffle = variant & 1, dups = variant & 2;
            const int64_t mb = 7, nb = 7;
            const Csr A = random_csr(b, mb, nb, shuffle, dups, 100u * b + variant);
            Bsr S;
            CHECK(convert(A, b, S) == RAILS_OK, "b %d variant %d: %s", b, variant, g_error);
            std::vector<double> D;
            std::vector<char> touched;
            dense_of(A, b, D, touched);
            // structure: exactly the touched blocks, ascending; block rows 2 and mb - 1 empty, 0 one block, 1 all of them
            CHECK(S.browptr[0] == 0 && S.browptr[1] == 1 && S.browptr[2] - S.browptr[1] == nb && S.browptr[3] == S.browptr[2] && S.browptr[(size_t)mb] == S.browptr[(size_t)mb - 1],
                  "b %d variant %d: block rows of one, all and no blocks", b, variant);
            std::vector<char> have((size_t)(mb * nb), 0);
            for (int64_t I = 0; I < mb; ++I)
                for (int64_t q = S.browptr[(size_t)I]; q < S.browptr[(size_t)I + 1]; ++q) {
                    CHECK(q == S.browptr[(size_t)I] || S.bcol[(size_t)q] > S.bcol[(size_t)q - 1], "b %d: block columns not ascending in block row %lld", b, (long long)I);
                    have[(size_t)(I * nb + S.bcol[(size_t)q])] = 1;
                    for (int r = 0; r < b; ++r)
                        for (int s = 0; s < b; ++s)
                            CHECK(same_bits(S.bval[(size_t)(q * b * b + r * b + s)], D[(size_t)((I * b + r) * A.n + S.bcol[(size_t)q] * b + s)]), "b %d variant %d: entry (%d, %d) of block %lld", b,
                                  variant, r, s, (long long)q);
                }
            CHECK(have == touched, "b %d variant %d: the blocks stored are not the blocks touched", b, variant);
        }
}

// expanding the block matrix and dropping stored zeros gives back a sorted, duplicate-free CSR matrix without zeros, array by array
static void test_round_trip()
{
    for (int b = 2; b <= 8; ++b) {
        Csr A = random_csr(b, 6, 6, false, false, 7u * b);
        Bsr S;
        CHECK(convert(A, b, S) == RAILS_OK, "b %d: %s", b, g_error);
        Csr E;
        E.rowptr.push_back(0);
        for (int64_t i = 0; i < A.m; ++i) {
            const int64_t I = i / b;
            for (int64_t q = S.browptr[(size_t)I]; q < S.browptr[(size_t)I + 1]; ++q)
                for (int s = 0; s < b; ++s) {
                    const double v = S.bval[(size_t)(q * b * b + (i % b) * b + s)];
                    if (v != 0.0) {
                        E.col.push_back(S.bcol[(size_t)q] * b + s);
                        E.val.push_back(v);
                    }
                }
            E.rowptr.push_back((int64_t)E.col.size());
        }
        CHECK(E.rowptr == A.rowptr && E.col == A.col, "b %d: the expanded pattern is not the CSR pattern", b);
        bool same = E.val.size() == A.val.size();
        for (size_t k = 0; same && k < E.val.size(); ++k) same = same_bits(E.val[k], A.val[k]);
        CHECK(same, "b %d: the expanded values are not the CSR values", b);
    }
}

static int transpose(const Bsr &S, Bsr &T)
{
    T.mb = S.nb;
    T.nb = S.mb;
    T.b = S.b;
    T.browptr.assign((size_t)T.mb + 1, -7);
    T.bcol.assign(S.bcol.size(), -7);
    T.bval.assign(S.bval.size(), -7.0);
    return rails_bsr_transpose_host(S.mb, S.nb, S.b, S.browptr.data(), S.bcol.data(), S.bval.data(), T.browptr.data(), T.bcol.data(), T.bval.data());
}

static void test_transpose()
{
    for (int b = 2; b <= 8; ++b) {
        Bsr S, T, TT;
        CHECK(convert(random_csr(b, 7, 7, true, true, 31u * b), b, S) == RAILS_OK, "%s", g_error);
        CHECK(transpose(S, T) == RAILS_OK && transpose(T, TT) == RAILS_OK, "b %d: %s", b, g_error);
        CHECK(TT.browptr == S.browptr && TT.bcol == S.bcol, "b %d: transposing twice changed the pattern", b);
        bool same = TT.bval.size() == S.bval.size();
        for (size_t k = 0; same && k < S.bval.size(); ++k) same = same_bits(TT.bval[k], S.bval[k]);
        CHECK(same, "b %d: transposing twice changed the values", b);
        // every block of the transpose is the transposed block at the transposed place
        for (int64_t J = 0; J < T.mb; ++J)
            for (int64_t q = T.browptr[(size_t)J]; q < T.browptr[(size_t)J + 1]; ++q) {
                const int64_t I = T.bcol[(size_t)q];
                int64_t p = -1;
                for (int64_t k = S.browptr[(size_t)I]; k < S.browptr[(size_t)I + 1]; ++k)
                    if (S.bcol[(size_t)k] == J) p = k;
                CHECK(p >= 0, "b %d: block (%lld, %lld) of the transpose has no origin", b, (long long)J, (long long)I);
                for (int r = 0; p >= 0 && r < b; ++r)
                    for (int s = 0; s < b; ++s) CHECK(same_bits(T.bval[(size_t)(q * b * b + s * b + r)], S.bval[(size_t)(p * b * b + r * b + s)]), "b %d: block not transposed", b);
            }
        // stable: a block matrix with the same block column twice in a block row (and unsorted columns) keeps the stored order of equals,
        // and the rows of a transposed row ascend
        Bsr R;
        R.mb = R.nb = 3;
        R.b = b;
        R.browptr = {0, 3, 5, 6};
        R.bcol = {2, 0, 2, 1, 1, 2};
        R.bval.resize(6 * (size_t)b * b);
        for (size_t k = 0; k < R.bval.size(); ++k) R.bval[k] = (double)k;
        Bsr Rt;
        CHECK(transpose(R, Rt) == RAILS_OK, "%s", g_error);
        CHECK((Rt.browptr == std::vector<int64_t>{0, 1, 3, 6}) && (Rt.bcol == std::vector<int32_t>{0, 1, 1, 0, 0, 2}), "b %d: the transposed pattern of the duplicate case", b);
        // the blocks of transposed row 2 come from blocks 0, 2 (block row 0, in stored order) and 5; of row 1 from 3, 4
        const int origin[6] = {1, 3, 4, 0, 2, 5};
        for (int q = 0; q < 6; ++q) CHECK(Rt.bval[(size_t)q * b * b + 1 * b + 0] == R.bval[(size_t)origin[q] * b * b + 0 * b + 1], "b %d: block %d of the transpose is not block %d", b, q, origin[q]);
    }
}

static void expect_einval(int rc, const char *needle, const char *what)
{
    CHECK(rc == RAILS_EINVAL, "%s: returned %d", what, rc);
    CHECK(std::strstr(g_error, needle) != nullptr, "%s: the text is \"%s\", without \"%s\"", what, g_error, needle);
    g_error[0] = 0;
}

static void test_refusals()
{
    const std::vector<int64_t> rp = {0, 1, 2, 3, 4};
    const std::vector<int32_t> ci = {0, 1, 2, 3};
    const std::vector<double> va = {1, 2, 3, 4};
    int64_t nnzb = 0;
    std::vector<int64_t> brp(8);
    std::vector<int32_t> bci(8);
    std::vector<double> bva(8 * 64);
    auto count = [&](int64_t m, int64_t n, int b, const std::vector<int64_t> &r, const std::vector<int32_t> &c) { return rails_bsr_count_host(m, n, b, r.data(), c.data(), &nnzb); };
    auto fill = [&](int64_t m, int64_t n, int b, const std::vector<int64_t> &r, const std::vector<int32_t> &c) {
        return rails_bsr_fill_host(m, n, b, r.data(), c.data(), va.data(), brp.data(), bci.data(), bva.data());
    };
    auto trans = [&](int64_t mb, int64_t nb, int b, const std::vector<int64_t> &r, const std::vector<int32_t> &c) {
        return rails_bsr_transpose_host(mb, nb, b, r.data(), c.data(), bva.data(), brp.data(), bci.data(), bva.data() + 4 * 64);
    };
    CHECK(count(4, 4, 2, rp, ci) == RAILS_OK && nnzb == 2, "the plain case: %s", g_error);
    CHECK(fill(4, 4, 2, rp, ci) == RAILS_OK, "the plain case: %s", g_error);
    for (int b : {-1, 0, 1, 9, 16}) {
        expect_einval(count(4 * 9 * 16, 4 * 9 * 16, b, rp, ci), "outside 2 .. 8", "count, block size");
        expect_einval(fill(4 * 9 * 16, 4 * 9 * 16, b, rp, ci), "outside 2 .. 8", "fill, block size");
        expect_einval(trans(4, 4, b, rp, ci), "outside 2 .. 8", "transpose, block size");
    }
    expect_einval(count(4, 4, 3, rp, ci), "no multiple of the block size", "count, rows no multiple");
    expect_einval(fill(4, 6, 4, rp, ci), "no multiple of the block size", "fill, columns no multiple");
    const std::vector<int64_t> down = {0, 2, 1, 3, 4}, late = {1, 1, 2, 3, 4};
    expect_einval(count(4, 4, 2, down, ci), "not monotone at row 1", "count, decreasing rowptr");
    expect_einval(fill(4, 4, 2, down, ci), "not monotone at row 1", "fill, decreasing rowptr");
    expect_einval(trans(4, 4, 2, down, ci), "not monotone at row 1", "transpose, decreasing browptr");
    expect_einval(count(4, 4, 2, late, ci), "rowptr[0] != 0", "count, rowptr[0]");
    const std::vector<int32_t> high = {0, 1, 4, 3}, low = {0, -1, 2, 3};
    expect_einval(count(4, 4, 2, rp, high), "column 4 out of range at entry 2", "count, column too large");
    expect_einval(fill(4, 4, 2, rp, low), "column -1 out of range at entry 1", "fill, negative column");
    expect_einval(trans(4, 4, 2, rp, high), "column 4 out of range at entry 2", "transpose, block column too large");
    expect_einval(rails_bsr_count_host(4, 4, 2, nullptr, ci.data(), &nnzb), "null rowptr", "count, null rowptr");
    expect_einval(rails_bsr_count_host(4, 4, 2, rp.data(), ci.data(), nullptr), "null output", "count, null output");
}

// ------------------------------------------------------------------------------------------------------------ the launch rule ---
struct Reach {
    bool seen = false;
    BsrFacts f;
};

static void test_choice(bool table)
{
    std::vector<Reach> reach(sizeof kBsrTable / sizeof kBsrTable[0]);
    std::set<int> listed;
    for (const BsrInst &t : kBsrTable) listed.insert(rails_bsr_inst(t.b, t.lpr));
    CHECK(listed.size() == reach.size(), "RAILS_BSR_TABLE names an instantiation twice");
    const int64_t mbs[] = {1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1000, 4097, 175616, 1000000, 268435455};
    const int64_t longest[] = {0, 1, 2, 7, 27, 63, 64, 65, 300, 5000};
    // (mb ascending inside nc ascending: the first shape that reaches an instantiation is its smallest)
    for (int b = 2; b <= 8; ++b)
        for (int nc = 1; nc <= 140; ++nc)
            for (int64_t mb : mbs)
                for (int64_t lg : longest)
                    for (int cu : {1, 64, 256})
                        for (int yv = 0; yv < 2; ++yv) {
                            BsrFacts f;
                            f.b = b; f.nc = nc; f.mb = mb; f.max_brow = lg; f.num_cu = cu; f.y_vec2 = yv != 0; f.ldx = f.ldy = 144;
                            const BsrChoice c = rails_bsr_choice(f);
                            CHECK(c.ok, "no choice for b %d nc %d mb %lld", b, nc, (long long)mb);
                            if (!c.ok) continue;
                            CHECK(listed.count(c.key()) == 1, "k_spmm_bsr<%d, %d> is not in the table", c.b, c.lpr);
                            CHECK(c.b == b && c.threads == rails_bsr_threads(b) && c.threads % c.lpr == 0 && c.threads % 64 == 0, "instantiation of b %d nc %d", b, nc);
                            CHECK(c.rpg >= 1 && c.rpg <= 4 && c.rows == c.threads / c.lpr * c.rpg, "block rows per workgroup, b %d nc %d", b, nc);
                            CHECK(c.grid == 8 * c.bpx && c.grid >= 8 && c.grid * c.rows >= mb && (c.bpx - 1) * 8 * c.rows < mb, "the grid covers %lld block rows, b %d nc %d", (long long)mb, b, nc);
                            CHECK(2 * c.lpr >= (nc < 64 ? nc : 64), "b %d: %d lanes for %d columns", b, c.lpr, nc);
                            CHECK(c.all_staged == ((int64_t)c.rows * lg <= rails_bsr_lds_blocks(b)), "all_staged, b %d", b);
                            CHECK(c.rpg == 1 || (int64_t)c.rows * (lg ? lg : 1) <= rails_bsr_lds_blocks(b), "b %d: more than one round although the runs do not fit", b);
                            CHECK(c.y_vec == f.y_vec2, "y_vec");
                            size_t at = 0;
                            while (at < reach.size() && rails_bsr_inst(kBsrTable[at].b, kBsrTable[at].lpr) != c.key()) ++at;
                            if (at < reach.size() && !reach[at].seen) reach[at] = {true, f};
                        }
    for (size_t k = 0; k < reach.size(); ++k) CHECK(reach[k].seen, "k_spmm_bsr<%d, %d> is listed and never chosen", kBsrTable[k].b, kBsrTable[k].lpr);
    // what the rule refuses
    for (int b : {0, 1, 9}) {
        BsrFacts f;
        f.b = b; f.nc = 4; f.mb = 10;
        CHECK(!rails_bsr_choice(f).ok, "a choice for b = %d", b);
    }
    BsrFacts z;
    z.b = 4; z.nc = 0; z.mb = 10;
    CHECK(!rails_bsr_choice(z).ok, "a choice for no columns");
    z.nc = 4; z.mb = 0;
    CHECK(!rails_bsr_choice(z).ok, "a choice for no rows");
    if (table)
        for (size_t k = 0; k < reach.size(); ++k) {
            const BsrChoice c = rails_bsr_choice(reach[k].f);
            printf("{\"kernel\": \"k_spmm_bsr\", \"inst\": [%d, %d], \"b\": %d, \"nc\": %d, \"mb\": %lld, \"threads\": %d, \"rows\": %d}\n", kBsrTable[k].b, kBsrTable[k].lpr, reach[k].f.b,
                   reach[k].f.nc, (long long)reach[k].f.mb, c.threads, c.rows);
        }
}

int main(int argc, char **argv)
{
    const bool table = argc > 1 && std::string(argv[1]) == "--table";
    if (table) {
        test_choice(true);
        return n_failed ? 1 : 0;
    }
    test_conversion();
    test_round_trip();
    test_transpose();
    test_refusals();
    test_choice(false);
    printf("%ld checks, %ld failed\n", n_checks, n_failed);
    if (n_failed == 0) printf("ALL PASSED\n");
    return n_failed ? 1 : 0;
}
