// The geometry of the iterative solve's passes (rails_amd/csrc/iter_geom.h) alone, on the host: no HIP, no library.  Built by
// rails_amd/csrc/Makefile into rails_amd/lib/iter_geom_host, run by tests/test_iter_geom_host.py (which also builds it once more, as host
// code, under the address and undefined-behaviour sanitizers).  Prints ALL PASSED at the end.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "iter_geom.h"

static int failed = 0, checks = 0;
#define CHECK(cond)                                                                                                                            \
    do {                                                                                                                                       \
        ++checks;                                                                                                                              \
        if (!(cond)) {                                                                                                                         \
            ++failed;                                                                                                                          \
            if (failed <= 20) std::printf("line %d (w %d, n %lld): %s\n", __LINE__, w, (long long)n, #cond);                                   \
        }                                                                                                                                      \
    } while (0)

// The two functions the header replaced, written out as they stood: the group's geometry from the operator's rows, a multigrid level's
// from the group's tx_bits.
static void group_rule(int64_t m, int w, int *tx_bits_out, int64_t *rps_out, int64_t *nslab_out)
{
    const int pairs = (w + 1) / 2;
    int tx_bits = 0;
    while ((1 << tx_bits) < pairs) ++tx_bits;
    const int TY = 256 >> tx_bits;
    int64_t nslab = std::max<int64_t>(1, std::min<int64_t>(1024, m / ((int64_t)TY * 8)));
    const int64_t rps = (m + nslab - 1) / nslab;
    nslab = (m + rps - 1) / rps;
    *tx_bits_out = tx_bits;
    *rps_out = rps;
    *nslab_out = nslab;
}
static void level_rule(int tx_bits, int64_t n, int64_t *rps_out, int64_t *slabs_out)
{
    const int TY = 256 >> tx_bits;
    int64_t ns = std::max<int64_t>(1, std::min<int64_t>(1024, n / ((int64_t)TY * 8)));
    const int64_t rps = (n + ns - 1) / ns;
    *slabs_out = (n + rps - 1) / rps;
    *rps_out = rps;
}

int main()
{
    for (int w = 1; w <= 32; ++w) {
        int64_t n = 0;
        // tx_bits: the smallest, at most 4, with a pair of columns per thread along x
        int tx_want = 0;
        while ((2 << tx_want) < w) ++tx_want;
        CHECK(tx_want <= 4 && (2 << tx_want) >= w && (tx_want == 0 || (2 << (tx_want - 1)) < w));
        const int64_t TY = 256 >> tx_want;
        const std::vector<int64_t> sizes = {1, 2, 8 * TY - 1, 8 * TY, 8 * TY + 1, 576, 102, 14, 1024 * 8 * TY - 1, 1024 * 8 * TY + 1, ((int64_t)1 << 24) - 1};
        for (int64_t rows : sizes) {
            n = rows;
            const int ld = (w + 15) / 16 * 16;
            int64_t slabs = -1;
            const rails_pass_geom g = rails_iter_pass_geom(n, w, ld, &slabs);
            CHECK(g.ncw == w && g.ld == ld && g.m == n);
            CHECK(g.tx_bits == tx_want);
            CHECK(slabs >= 1 && slabs <= 1024);
            // the slabs tile [0, n) exactly as the kernels cut them (iter_pass: block b owns [b rps, min((b + 1) rps, m))), none empty
            CHECK(g.rows_per_slab >= 1);
            CHECK((slabs - 1) * g.rows_per_slab < n && slabs * g.rows_per_slab >= n);
            int64_t covered = 0;
            bool empty = false;
            for (int64_t b = 0; b < slabs; ++b) {
                const int64_t r0 = b * g.rows_per_slab, r1 = std::min(r0 + g.rows_per_slab, n);
                empty = empty || r1 <= r0 || r0 != covered;
                covered = r1;
            }
            CHECK(!empty && covered == n);
            // the values of the two functions as they stood
            int tx_old;
            int64_t rps_old, nslab_old, rps_lvl, slabs_lvl;
            group_rule(n, w, &tx_old, &rps_old, &nslab_old);
            level_rule(tx_old, n, &rps_lvl, &slabs_lvl);
            CHECK(g.tx_bits == tx_old && g.rows_per_slab == rps_old && slabs == nslab_old);
            CHECK(g.rows_per_slab == rps_lvl && slabs == slabs_lvl);
        }
    }
    std::printf("%d checks, %d failed\n", checks, failed);
    if (!failed) std::printf("ALL PASSED\n");
    return failed ? 1 : 0;
}
