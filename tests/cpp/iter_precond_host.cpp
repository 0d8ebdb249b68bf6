// The rule of the iterative solve's preconditioners (rails_amd/csrc/iter_precond.h) alone, on the host: no HIP, no library.  Built by
// rails_amd/csrc/Makefile into rails_amd/lib/iter_precond_host, run by tests/test_iter_precond_host.py (which also builds it once more,
// as host code, under the address and undefined-behaviour sanitizers).
//   iter_precond_host --table [m b]
//                               one line per combination of facts and request (R: granted, or the refusal's text) and per combination
//                               of facts (E: the effect record), for the comparison with tests/iter_precond_reference.py line by line;
//                               with m and b: the same table for that one row count and block size (tests/test_gpu_iter_precond.py)
//   iter_precond_host           what must hold over the same product whatever the texts are; prints ALL PASSED at the end
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "iter_precond.h"

static int failed = 0, checks = 0;
#define CHECK(cond)                                                                                                                            \
    do {                                                                                                                                       \
        ++checks;                                                                                                                              \
        if (!(cond)) {                                                                                                                         \
            ++failed;                                                                                                                          \
            if (failed <= 20) std::printf("line %d (%s): %s\n", __LINE__, key, #cond);                                                        \
        }                                                                                                                                      \
    } while (0)

// the operator as the product runs over it: a stored one with and without its host arrays, a block-CSR one (b = 3) with and without its
// host copy, a callback, an LU, an iterative solve
static const char *const OPS[] = {"stored", "stored_nohost", "bsr", "bsr_nohost", "callback", "lu", "iter"};
static int BLOCK = 3;
// rows on both sides of 2^24, divisible by the block size and not
static std::vector<int64_t> ROWS = {3000, 3001, 16777218, 16777217};
static const char *const REQUESTS[] = {"poly_degree", "amg", "block_amg", "block_jacobi", "install_blocks", "amg_setup", "block_amg_setup"};
static const char *const WHO[] = {"rails_iter_set", "rails_iter_set", "rails_iter_set", "rails_iter_set", "rails_iter_block_jacobi", "rails_iter_amg_setup", "rails_iter_block_amg_setup"};
static const int POLY = 5; // the degree where "poly_degree" is on or asked for

static void set_op(rails_precond_facts &f, int op)
{
    static const int kind[] = {RAILS_PC_OP_STORED, RAILS_PC_OP_STORED, RAILS_PC_OP_BSR, RAILS_PC_OP_BSR, RAILS_PC_OP_CALLBACK, RAILS_PC_OP_LU, RAILS_PC_OP_ITER};
    f.op = kind[op];
    f.host_csr = op == 0;
    f.host_b = op == 2 ? BLOCK : 0;
}

static void key_of(const rails_precond_facts &f, int op, char *key, size_t cap)
{
    std::snprintf(key, cap, "cg=%d op=%s reduces=%d exchanges=%d m=%lld diag=%d blocks=%d defsign=%d jacobi=%d poly_degree=%d amg=%d block_amg=%d block_jacobi=%d", (int)f.cg, OPS[op],
                  (int)f.reduces, (int)f.exchanges, (long long)f.m, (int)f.diag, f.blocks_b, f.defsign, (int)f.jacobi, f.poly_degree, (int)f.amg, (int)f.block_amg, (int)f.block_jacobi);
}

static void one(const rails_precond_facts &f, int op, bool table)
{
    char key[320], err[320], again[320];
    key_of(f, op, key, sizeof key);
    const rails_precond_effect e = rails_precond_effect_of(f);
    if (table)
        std::printf("E %s | pass=%d b=%d beyond=%d K=%d sign=%d panels=%u\n", key, e.pass, e.b, e.beyond, e.K, e.sign, e.panels);
    else {
        CHECK((e.b > 0) == (e.pass == RAILS_PC_PASS_BLOCKS) && (e.K > 0) == (e.beyond == RAILS_PC_BEYOND_POLY));
        CHECK(e.sign == 1 || (e.sign == f.defsign && e.pass == RAILS_PC_PASS_NONE && e.beyond == RAILS_PC_BEYOND_NONE));
        CHECK(e.panels < (1u << W_COUNT) && (e.panels & 15u) == 15u);
        // what a call reads is among the panels: z where anything is applied, s^ for BiCGStab's second application, d and the second z beyond
        if (e.pass != RAILS_PC_PASS_NONE || e.beyond != RAILS_PC_BEYOND_NONE) CHECK(e.panels >> W_Z & 1);
        if (e.pass != RAILS_PC_PASS_NONE && !f.cg) CHECK(e.panels >> W_SH & 1);
        if (e.beyond != RAILS_PC_BEYOND_NONE) CHECK((e.panels >> W_D & 1) && (e.panels >> W_Z2 & 1));
        if (!f.cg) CHECK((e.panels >> W_RH & 1) && (e.panels >> W_T & 1));
    }
    if (f.defsign < 0) return; // (no request looks at the sign)
    for (int r = 0; r < RAILS_PC_REQUESTS; ++r)
        for (int v = (r == RAILS_PC_POLY ? 0 : 1); v <= 1; ++v) {
            const int value = r == RAILS_PC_POLY ? v * POLY : r == RAILS_PC_INSTALL_BLOCKS ? BLOCK : 1;
            std::memset(err, 0, sizeof err);
            const bool ok = rails_precond_grant(f, r, value, WHO[r], err, sizeof err);
            if (table) {
                std::printf("R %s | %s %d | %s\n", key, REQUESTS[r], value, ok ? "granted" : err);
                continue;
            }
            CHECK(ok == (err[0] == 0));
            if (!ok) CHECK(std::strncmp(err, WHO[r], std::strlen(WHO[r])) == 0 && std::strlen(err) + 1 < sizeof err);
            // a short buffer truncates and terminates, and the answer does not depend on it
            std::memset(again, 'x', sizeof again);
            CHECK(rails_precond_grant(f, r, value, WHO[r], again, 8) == ok && (ok || (std::strlen(again) == 7 && std::strncmp(again, err, 7) == 0)));
            // one at a time: with another preconditioner on, turning one on is refused
            const int others = (f.poly_degree > 0) + f.amg + f.block_amg + f.block_jacobi;
            const bool self = (r == RAILS_PC_POLY && f.poly_degree > 0) || ((r == RAILS_PC_AMG || r == RAILS_PC_SETUP_AMG) && f.amg) ||
                              ((r == RAILS_PC_BLOCK_AMG || r == RAILS_PC_SETUP_BLOCK_AMG) && f.block_amg) || ((r == RAILS_PC_BLOCK_JACOBI || r == RAILS_PC_INSTALL_BLOCKS) && f.block_jacobi);
            if (value != 0 && others - (int)self > 0) CHECK(!ok);
            if (r == RAILS_PC_POLY && value == 0) CHECK(ok);
        }
}

int main(int argc, char **argv)
{
    const bool table = argc > 1 && std::strcmp(argv[1], "--table") == 0;
    if (table && argc > 3) {
        ROWS = {std::atoll(argv[2])};
        BLOCK = std::atoi(argv[3]);
    }
    rails_precond_facts f;
    for (int cg = 0; cg < 2; ++cg)
        for (int op = 0; op < 7; ++op)
            for (int net = 0; net < 4; ++net)
                for (int64_t m : ROWS)
                    for (int have = 0; have < 8; ++have)
                        for (int on = 0; on < 32; ++on) {
                            f.cg = cg != 0;
                            set_op(f, op);
                            f.reduces = (net & 1) != 0;
                            f.exchanges = (net & 2) != 0;
                            f.m = m;
                            f.diag = (have & 1) != 0;
                            f.blocks_b = (have & 2) ? BLOCK : 0;
                            f.defsign = (have & 4) ? -1 : 1;
                            f.jacobi = (on & 1) != 0;
                            f.poly_degree = (on & 2) ? POLY : 0;
                            f.amg = (on & 4) != 0;
                            f.block_amg = (on & 8) != 0;
                            f.block_jacobi = (on & 16) != 0;
                            one(f, op, table);
                        }
    if (table) return 0;
    std::printf("%d checks, %d failed\n", checks, failed);
    if (!failed) std::printf("ALL PASSED\n");
    return failed ? 1 : 0;
}
