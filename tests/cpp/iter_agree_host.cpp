// What the ranks of a row partition agree on when an iterative A^-1 object is made (rails_amd/csrc/iter_agree.h), and the rule for the
// ghost-row form of the fused Chebyshev step (rails_amd/csrc/cheb_coef.h), alone on the host: no HIP, no library.  Built by
// rails_amd/csrc/Makefile into rails_amd/lib/iter_agree_host, run by tests/test_iter_agree_host.py (which also builds it once more, as host
// code, under the address and undefined-behaviour sanitizers).  Prints ALL PASSED at the end.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "cheb_coef.h"
#include "iter_agree.h"

static int failed = 0, checks = 0;
#define CHECK(cond)                                                                                                                            \
    do {                                                                                                                                       \
        ++checks;                                                                                                                              \
        if (!(cond)) {                                                                                                                         \
            ++failed;                                                                                                                          \
            std::printf("line %d: %s\n", __LINE__, #cond);                                                                                     \
        }                                                                                                                                      \
    } while (0)

struct Rank {
    double state;
    bool negative;
    double hi_plain, hi_jacobi;
};

// the gather as the library makes it: every rank's slot in a zeroed vector of its own, the vectors added entry by entry in rank order
static rails_iter_agreed agree(const std::vector<Rank> &ranks)
{
    const int n = (int)ranks.size();
    std::vector<double> sum((size_t)n * RAILS_AGREE_SLOT, 0.0);
    for (int r = 0; r < n; ++r) {
        std::vector<double> mine((size_t)n * RAILS_AGREE_SLOT, 0.0);
        rails_iter_agree_fill(mine.data() + (size_t)r * RAILS_AGREE_SLOT, ranks[r].state, ranks[r].negative, ranks[r].hi_plain, ranks[r].hi_jacobi);
        for (size_t i = 0; i < sum.size(); ++i) sum[i] += mine[i];
    }
    return rails_iter_agree(sum.data(), n);
}

int main()
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const double D = RAILS_AGREE_DIAG, N = RAILS_AGREE_NO_DIAG, X = RAILS_AGREE_REFUSED;
    {   // three ranks that agree: Jacobi on, positive, the bounds are the largest
        const rails_iter_agreed a = agree({{D, false, 4.0, 1.5}, {D, false, 7.5, 1.25}, {D, false, 6.0, 1.9}});
        CHECK(!a.refused && a.jacobi && a.defsign == 1.0 && a.hi_plain == 7.5 && a.hi_jacobi == 1.9);
    }
    {   // the diagonal missing on one rank of three turns Jacobi off for all; its bound goes with it, the plain bound stays
        for (int miss = 0; miss < 3; ++miss) {
            std::vector<Rank> r = {{D, false, 4.0, 1.5}, {D, false, 7.5, 1.25}, {D, false, 6.0, 1.9}};
            r[miss] = {N, false, 5.0, 0.0};
            const rails_iter_agreed a = agree(r);
            CHECK(!a.refused && !a.jacobi && a.defsign == 1.0 && a.hi_jacobi == 0.0 && a.hi_plain >= 6.0);
        }
    }
    {   // defsign -1 only when every rank's diagonal is all negative: one positive entry on one rank gives +1
        CHECK(agree({{D, true, 4.0, 1.5}, {D, true, 7.5, 1.25}, {D, true, 6.0, 1.9}}).defsign == -1.0);
        for (int pos = 0; pos < 3; ++pos) {
            std::vector<Rank> r = {{D, true, 4.0, 1.5}, {D, true, 7.5, 1.25}, {D, true, 6.0, 1.9}};
            r[pos].negative = false;
            const rails_iter_agreed a = agree(r);
            CHECK(a.jacobi && a.defsign == 1.0);
        }
        // all negative but no diagonal on one rank: the single-rank rule (no diagonal: +1)
        CHECK(agree({{D, true, 4.0, 1.5}, {N, false, 7.5, 0.0}}).defsign == 1.0);
        CHECK(agree({{D, true, 4.0, 1.5}}).defsign == -1.0 && agree({{D, false, 4.0, 1.5}}).defsign == 1.0);
    }
    {   // hi is the maximum, wherever it sits
        for (int big = 0; big < 3; ++big) {
            std::vector<Rank> r = {{D, false, 4.0, 1.5}, {D, false, 4.0, 1.5}, {D, false, 4.0, 1.5}};
            r[big].hi_plain = 9.0;
            r[(big + 1) % 3].hi_jacobi = 1.75;
            const rails_iter_agreed a = agree(r);
            CHECK(a.hi_plain == 9.0 && a.hi_jacobi == 1.75);
        }
    }
    {   // a NaN bound shows, first, in the middle or last; a rank without host arrays (0) leaves no bound at all
        for (int bad = 0; bad < 3; ++bad) {
            std::vector<Rank> r = {{D, false, 4.0, 1.5}, {D, false, 7.5, 1.25}, {D, false, 6.0, 1.9}};
            r[bad].hi_plain = nan;
            rails_iter_agreed a = agree(r);
            CHECK(a.hi_plain != a.hi_plain && a.hi_jacobi == 1.9);
            r[bad].hi_plain = 7.5;
            r[bad].hi_jacobi = nan;
            a = agree(r);
            CHECK(a.hi_jacobi != a.hi_jacobi && a.hi_plain == 7.5);
        }
        const rails_iter_agreed none = agree({{D, false, 4.0, 1.5}, {D, false, 0.0, 0.0}, {D, false, 6.0, 1.9}});
        CHECK(none.hi_plain == 0.0 && none.hi_jacobi == 0.0 && none.jacobi);
        const rails_iter_agreed inf = agree({{D, false, 4.0, 1.5}, {D, false, std::numeric_limits<double>::infinity(), 1.0}});
        CHECK(std::isinf(inf.hi_plain)); // (the solve's own test for a finite bound refuses it)
    }
    {   // a rank that refuses its arguments makes every rank refuse; anything that is none of the three states counts as a refusal
        CHECK(agree({{D, false, 4.0, 1.5}, {X, false, 0.0, 0.0}, {D, false, 6.0, 1.9}}).refused);
        CHECK(agree({{D, false, 4.0, 1.5}, {nan, false, 0.0, 0.0}}).refused);
        CHECK(agree({{D, false, 4.0, 1.5}, {2.0, false, 0.0, 0.0}}).refused); // two ranks in one slot
        CHECK(!agree({{N, false, 0.0, 0.0}}).refused && !agree({{N, false, 0.0, 0.0}}).jacobi);
    }

    // ---- the rule for the ghost-row form of the fused step, at the edges of each limit
    const int64_t two24 = (int64_t)1 << 24;
    CHECK(rails_cheb_fused_ghost_eligible(true, 1000, 2, 16, 4));
    CHECK(!rails_cheb_fused_ghost_eligible(false, 1000, 2, 16, 4)); // not a stored CSR operator
    CHECK(rails_cheb_fused_ghost_eligible(true, 1, 0, 16, 2) && !rails_cheb_fused_ghost_eligible(true, 0, 0, 16, 2));
    CHECK(rails_cheb_fused_ghost_eligible(true, 1000, 0, 16, 2) && !rails_cheb_fused_ghost_eligible(true, 1000, -1, 16, 2));
    CHECK(rails_cheb_fused_ghost_eligible(true, two24 - 1, 2, 16, 2) && !rails_cheb_fused_ghost_eligible(true, two24, 2, 16, 2));
    CHECK(rails_cheb_fused_ghost_eligible(true, 1000, two24 - 1, 16, 2) && !rails_cheb_fused_ghost_eligible(true, 1000, two24, 16, 2));
    // row strides: times 8 below 2^24
    CHECK(rails_cheb_fused_ghost_eligible(true, 16, 2, two24 / 8 - 1, 2) && !rails_cheb_fused_ghost_eligible(true, 16, 2, two24 / 8, 2));
    CHECK(rails_cheb_fused_ghost_eligible(true, 16, 2, 16, two24 / 8 - 1) && !rails_cheb_fused_ghost_eligible(true, 16, 2, 16, two24 / 8));
    CHECK(!rails_cheb_fused_ghost_eligible(true, 16, 2, 0, 2) && !rails_cheb_fused_ghost_eligible(true, 16, 2, 16, 0));
    {   // both buffers below 0xffffff00 bytes: m * ld * 8 and n_ghost * ldg * 8
        const int64_t ld = 32, limit = 0xffffff00ll, rows_ok = (limit - 1) / (ld * 8), rows_bad = rows_ok + 1;
        CHECK(rows_ok < two24 && rows_ok * ld * 8 < limit && rows_bad * ld * 8 >= limit);
        CHECK(rails_cheb_fused_ghost_eligible(true, rows_ok, 2, ld, 2) && !rails_cheb_fused_ghost_eligible(true, rows_bad, 2, ld, 2));
        CHECK(rails_cheb_fused_ghost_eligible(true, 16, rows_ok, 16, ld) && !rails_cheb_fused_ghost_eligible(true, 16, rows_bad, 16, ld));
    }
    // the form without ghost rows keeps refusing them
    CHECK(rails_cheb_fused_eligible(true, 0, 1000, 16) && !rails_cheb_fused_eligible(true, 1, 1000, 16));

    std::printf("%d checks, %d failed\n", checks, failed);
    if (failed == 0) std::printf("ALL PASSED\n");
    return failed ? 1 : 0;
}
