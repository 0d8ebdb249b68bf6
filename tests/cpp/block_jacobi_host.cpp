// The host part of the block-Jacobi preconditioner (rails_amd/csrc/block_jacobi_host.h) and the block geometry of the passes
// (rails_amd/csrc/iter_geom.h: rails_iter_pass_geom_block) alone, on the host: no HIP, no library.  Built by rails_amd/csrc/Makefile into
// rails_amd/lib/block_jacobi_host, run by tests/test_block_jacobi_host.py (which also builds it once more, as host code, under the address
// and undefined-behaviour sanitizers).
//   block_jacobi_host                  the checks below; prints ALL PASSED at the end
//   block_jacobi_host geom NBMAX       one line "nb w b TY slabs rows_per_slab" per (nb <= NBMAX and a few large values, w <= 32, b in 2 .. 8)
//   block_jacobi_host invert IN OUT    IN: int64 nblocks, int64 b, nblocks * b * b doubles; OUT: the inverses (or the refusal on stdout, exit 2)
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "block_jacobi_host.h"
#include "iter_geom.h"

static int failed = 0, checks = 0;
#define CHECK(cond)                                                                                                                            \
    do {                                                                                                                                       \
        ++checks;                                                                                                                              \
        if (!(cond)) {                                                                                                                         \
            ++failed;                                                                                                                          \
            if (failed <= 20) std::printf("line %d: %s\n", __LINE__, #cond);                                                                  \
        }                                                                                                                                      \
    } while (0)

static const int64_t LARGE[] = {8191, 8192, 8193, 1024 * 2048 - 1, 1024 * 2048 + 7, (int64_t)268435455};

static void check_geometry()
{
    for (int b = 2; b <= 8; ++b)
        for (int w = 1; w <= 32; ++w) {
            int tx_want = 0;
            while ((2 << tx_want) < w) ++tx_want;
            const int64_t TY = 256 >> tx_want;
            std::vector<int64_t> sizes;
            for (int64_t nb = 1; nb <= 600; ++nb) sizes.push_back(nb);
            for (int64_t nb : LARGE) sizes.push_back(nb);
            for (int64_t nb : {8 * TY - 1, 8 * TY, 8 * TY + 1, 17 * 8 * TY, 17 * 8 * TY + 5}) sizes.push_back(nb);
            for (int64_t nb : sizes) {
                const int64_t n = nb * b;
                int64_t slabs = -1;
                const rails_pass_geom g = rails_iter_pass_geom_block(n, w, 32, b, &slabs);
                CHECK(g.ncw == w && g.ld == 32 && g.m == n && g.tx_bits == tx_want);
                CHECK(slabs >= 1 && slabs <= 1024);
                CHECK(g.rows_per_slab >= b && g.rows_per_slab % b == 0); // whole block rows
                const int64_t bps = g.rows_per_slab / b;
                // the slabs tile the block rows as iter_pass_block cuts them, and the rows as the point passes of the same solve do
                int64_t covered = 0;
                bool bad = false;
                for (int64_t s = 0; s < slabs; ++s) {
                    const int64_t b0 = s * bps, b1 = std::min(b0 + bps, nb);
                    bad = bad || b1 <= b0 || b0 != covered;
                    covered = b1;
                    const int64_t r0 = s * g.rows_per_slab, r1 = std::min(r0 + g.rows_per_slab, n);
                    bad = bad || r0 != b0 * b || r1 != b1 * b;
                }
                CHECK(!bad && covered == nb);
                // at least 8 block rows per thread where there are that many (the last slab may be shorter), and no more slabs than that allows
                if (nb >= 8 * TY) CHECK(bps >= 8 * TY);
                if (nb < 8 * TY) CHECK(slabs == 1);
            }
        }
}

static bool refused(int op, int hb, bool reduces, int64_t m, int b, bool given, const char *needle)
{
    int source = -1, be = -1;
    char err[256] = "";
    const int rc = rails_bj_plan(op, hb, reduces, m, b, given, &source, &be, err, sizeof err);
    return rc != 0 && std::strstr(err, needle) != nullptr && std::strstr(err, "rails_iter_block_jacobi") != nullptr;
}

static void check_plan()
{
    int source = -1, be = -1;
    char err[256] = "";
    // accepted: blocks given on every kind; none given on a block-CSR handle (b 0 or its own) and on a CSR handle with host arrays
    for (int op : {RAILS_BJ_OP_CSR, RAILS_BJ_OP_CSR_NO_HOST, RAILS_BJ_OP_CALLBACK, RAILS_BJ_OP_LU, RAILS_BJ_OP_ITER})
        CHECK(rails_bj_plan(op, 0, false, 24, 4, true, &source, &be, err, sizeof err) == 0 && source == RAILS_BJ_FROM_ARGUMENT && be == 4);
    CHECK(rails_bj_plan(RAILS_BJ_OP_BSR, 4, false, 24, 4, true, &source, &be, err, sizeof err) == 0 && source == RAILS_BJ_FROM_ARGUMENT && be == 4);
    CHECK(rails_bj_plan(RAILS_BJ_OP_BSR, 4, false, 24, 0, false, &source, &be, err, sizeof err) == 0 && source == RAILS_BJ_FROM_BSR && be == 4);
    CHECK(rails_bj_plan(RAILS_BJ_OP_BSR, 4, false, 24, 4, false, &source, &be, err, sizeof err) == 0 && source == RAILS_BJ_FROM_BSR && be == 4);
    CHECK(rails_bj_plan(RAILS_BJ_OP_CSR, 0, false, 24, 3, false, &source, &be, err, sizeof err) == 0 && source == RAILS_BJ_FROM_CSR && be == 3);
    for (int b = 2; b <= 8; ++b) CHECK(rails_bj_plan(RAILS_BJ_OP_CSR, 0, false, 840, b, false, &source, &be, err, sizeof err) == 0 && be == b);
    // b == 0 without blocks on anything but a block-CSR handle clears, on a context that reduces too
    for (int op : {RAILS_BJ_OP_CSR, RAILS_BJ_OP_CSR_NO_HOST, RAILS_BJ_OP_CALLBACK, RAILS_BJ_OP_LU, RAILS_BJ_OP_ITER})
        for (bool reduces : {false, true}) CHECK(rails_bj_plan(op, 0, reduces, 24, 0, false, &source, &be, err, sizeof err) == 0 && source == RAILS_BJ_CLEAR && be == 0);
    // refused, each with its reason
    CHECK(refused(RAILS_BJ_OP_CSR, 0, false, 24, 1, true, "not in 2 .. 8"));
    CHECK(refused(RAILS_BJ_OP_CSR, 0, false, 24, 9, true, "not in 2 .. 8"));
    CHECK(refused(RAILS_BJ_OP_CSR, 0, false, 24, -3, false, "not in 2 .. 8"));
    CHECK(refused(RAILS_BJ_OP_CSR, 0, false, 24, 0, true, "not in 2 .. 8"));
    CHECK(refused(RAILS_BJ_OP_CSR, 0, false, 25, 4, true, "does not divide"));
    CHECK(refused(RAILS_BJ_OP_CSR, 0, false, 25, 4, false, "does not divide"));
    CHECK(refused(RAILS_BJ_OP_CALLBACK, 0, false, 24, 4, false, "callback"));
    CHECK(refused(RAILS_BJ_OP_LU, 0, false, 24, 4, false, "LU"));
    CHECK(refused(RAILS_BJ_OP_ITER, 0, false, 24, 4, false, "iterative solve"));
    CHECK(refused(RAILS_BJ_OP_CSR_NO_HOST, 0, false, 24, 4, false, "no CSR arrays on the host"));
    CHECK(refused(RAILS_BJ_OP_BSR, 4, false, 24, 2, false, "block size 4"));
    CHECK(refused(RAILS_BJ_OP_BSR, 4, false, 24, 2, true, "block size 4"));
    CHECK(refused(RAILS_BJ_OP_CSR, 0, true, 24, 4, true, "reduces"));
    CHECK(refused(RAILS_BJ_OP_BSR, 4, true, 24, 0, false, "reduces"));
}

static void check_extraction()
{
    // 2 block rows of 2 x 2 blocks; block row 0 stores its diagonal block twice around an off-diagonal one, block row 1 has none
    {
        const int64_t browptr[] = {0, 3, 4};
        const int32_t bcol[] = {0, 1, 0, 0};
        const double bval[] = {1, 2, 3, 4, 9, 9, 9, 9, 10, 20, 30, 40, 7, 7, 7, 7};
        double blocks[8];
        std::fill(blocks, blocks + 8, -1.0);
        rails_bj_from_bsr(2, 2, browptr, bcol, bval, blocks);
        const double want[8] = {11, 22, 33, 44, 0, 0, 0, 0};
        for (int k = 0; k < 8; ++k) CHECK(blocks[k] == want[k]);
    }
    // stored order of a repeated diagonal block: (1e16 + 1) - 1e16 is 0 in that order and 1 in the other
    {
        const int64_t browptr[] = {0, 3};
        const int32_t bcol[] = {0, 0, 0};
        double bval[12] = {};
        bval[0] = 1e16;
        bval[4] = 1.0;
        bval[8] = -1e16;
        double blocks[4];
        rails_bj_from_bsr(1, 2, browptr, bcol, bval, blocks);
        CHECK(blocks[0] == (1e16 + 1.0) - 1e16 && blocks[1] == 0.0 && blocks[2] == 0.0 && blocks[3] == 0.0);
    }
    // CSR, m = 6, b = 3: unsorted columns, a duplicate, entries outside the block range, a missing entry, an empty row
    {
        const int64_t rowptr[] = {0, 4, 6, 6, 9, 10, 13};
        const int32_t col[] = {2, 5, 0, 2, /* row 1 */ 1, 3, /* row 2: empty; row 3 */ 5, 0, 3, /* row 4 */ 2, /* row 5 */ 4, 5, 4};
        const double val[] = {1.5, 100, 2.5, 0.25, 4, 100, 6, 100, 7, 100, 1e16, 3, -1e16};
        double blocks[18];
        std::fill(blocks, blocks + 18, -1.0);
        rails_bj_from_csr(2, 3, rowptr, col, val, blocks);
        const double want[18] = {2.5, 0, 1.75, 0, 4, 0, 0, 0, 0, /* block 1 */ 7, 0, 6, 0, 0, 0, 0, 1e16 + -1e16, 3};
        for (int k = 0; k < 18; ++k) CHECK(blocks[k] == want[k]);
    }
}

static void check_inverse()
{
    char err[256] = "";
    // a permutation-like block: partial pivoting is needed (the leading entry is 0)
    {
        const double blk[4] = {0, 2, 4, 0};
        double inv[4];
        CHECK(rails_bj_invert(1, 2, blk, inv, err, sizeof err) == 0);
        CHECK(inv[0] == 0.0 && inv[1] == 0.25 && inv[2] == 0.5 && inv[3] == 0.0);
    }
    // A X = I on diagonally dominant blocks of every size, a plain sanity check: |A| |X| has row sums below 4 there, so one rounding of X
    // leaves at most 4 * eps / 2 in an entry of A X; 64 eps is far above that (the sharp, componentwise bound is the Python test's)
    for (int b = 2; b <= 8; ++b) {
        std::vector<double> blk((size_t)3 * b * b), inv(blk.size());
        uint64_t s = 88172645463325252ull + (uint64_t)b;
        for (size_t k = 0; k < blk.size(); ++k) {
            s ^= s << 13, s ^= s >> 7, s ^= s << 17;
            blk[k] = (double)(s % 2001) / 1000.0 - 1.0;
        }
        for (int k = 0; k < 3; ++k)
            for (int i = 0; i < b; ++i) blk[(size_t)k * b * b + i * b + i] += b;
        CHECK(rails_bj_invert(3, b, blk.data(), inv.data(), err, sizeof err) == 0);
        for (int k = 0; k < 3; ++k)
            for (int i = 0; i < b; ++i)
                for (int j = 0; j < b; ++j) {
                    long double acc = 0;
                    for (int l = 0; l < b; ++l) acc += (long double)blk[(size_t)k * b * b + i * b + l] * inv[(size_t)k * b * b + l * b + j];
                    CHECK(std::fabs((double)(acc - (i == j ? 1.0L : 0.0L))) <= 64 * std::numeric_limits<double>::epsilon());
                }
    }
    // refusals name the block: a singular block, a NaN, an infinity, an inverse that overflows
    {
        double blk[12] = {1, 0, 0, 1, /* block 1: singular */ 1, 2, 2, 4, /* block 2 */ 2, 0, 0, 2};
        double inv[12];
        CHECK(rails_bj_invert(3, 2, blk, inv, err, sizeof err) != 0 && std::strstr(err, "block 1 ") && std::strstr(err, "pivot"));
        blk[4] = std::numeric_limits<double>::quiet_NaN();
        CHECK(rails_bj_invert(3, 2, blk, inv, err, sizeof err) != 0 && std::strstr(err, "block 1 "));
        blk[4] = 1;
        blk[7] = 5;
        blk[9] = std::numeric_limits<double>::infinity();
        CHECK(rails_bj_invert(3, 2, blk, inv, err, sizeof err) != 0 && std::strstr(err, "block 2 "));
        blk[9] = 0;
        CHECK(rails_bj_invert(3, 2, blk, inv, err, sizeof err) == 0);
        blk[0] = 1e-320; // the pivot is not zero, its reciprocal overflows double
        CHECK(rails_bj_invert(3, 2, blk, inv, err, sizeof err) != 0 && std::strstr(err, "block 0 ") && std::strstr(err, "not finite"));
        const double zero[9] = {};
        double inv3[9];
        CHECK(rails_bj_invert(1, 3, zero, inv3, err, sizeof err) != 0 && std::strstr(err, "block 0 "));
    }
}

int main(int argc, char **argv)
{
    if (argc >= 3 && std::string(argv[1]) == "geom") {
        const int64_t nbmax = std::atoll(argv[2]);
        std::vector<int64_t> sizes;
        for (int64_t nb = 1; nb <= nbmax; ++nb) sizes.push_back(nb);
        for (int64_t nb : LARGE) sizes.push_back(nb);
        for (int64_t nb : sizes)
            for (int w = 1; w <= 32; ++w)
                for (int b = 2; b <= 8; ++b) {
                    int64_t slabs = 0;
                    const rails_pass_geom g = rails_iter_pass_geom_block(nb * b, w, 32, b, &slabs);
                    std::printf("%lld %d %d %d %lld %lld\n", (long long)nb, w, b, 256 >> g.tx_bits, (long long)slabs, (long long)g.rows_per_slab);
                }
        return 0;
    }
    if (argc >= 4 && std::string(argv[1]) == "invert") {
        FILE *f = std::fopen(argv[2], "rb");
        int64_t head[2] = {0, 0};
        if (!f || std::fread(head, sizeof(int64_t), 2, f) != 2 || head[0] < 0 || head[1] < 2 || head[1] > 8) return 3;
        std::vector<double> blk((size_t)(head[0] * head[1] * head[1])), inv(blk.size());
        if (std::fread(blk.data(), sizeof(double), blk.size(), f) != blk.size()) return 3;
        std::fclose(f);
        char err[256] = "";
        if (rails_bj_invert(head[0], (int)head[1], blk.data(), inv.data(), err, sizeof err)) {
            std::printf("%s\n", err);
            return 2;
        }
        f = std::fopen(argv[3], "wb");
        if (!f || std::fwrite(inv.data(), sizeof(double), inv.size(), f) != inv.size()) return 3;
        std::fclose(f);
        return 0;
    }
    check_geometry();
    check_plan();
    check_extraction();
    check_inverse();
    std::printf("%d checks, %d failed\n", checks, failed);
    if (!failed) std::printf("ALL PASSED\n");
    return failed ? 1 : 0;
}
