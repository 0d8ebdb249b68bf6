// What the 32-bit guards decide for facts read from standard input, one question per line, one answer per line: no HIP, no library.  Built
// by rails_amd/csrc/Makefile into rails_amd/lib/tall_stride_guard_host, run by tests/test_tall_stride_cases_host.py, which asks it every
// case of tests/tall_stride_cases.py and compares with that module's restatement of the rules.
//
//   row <variant> <nc> <xoff> <yoff> <ldx> <m> <ncols_ext> <max_row_nnz> <rect>   -> PLAIN | CC | NARROW    (row_choice.h, serial product,
//                                                                                    no ghost rows; rect: the extra rows follow X)
//   cheb <m> <ld>                                                                 -> 0 | 1                  (cheb_coef.h, the fused step)
#include <cstdio>
#include <cstring>

#include "cheb_coef.h"
#include "row_choice.h"

int main()
{
    char what[16];
    while (std::scanf("%15s", what) == 1) {
        if (!std::strcmp(what, "row")) {
            long long variant, nc, xoff, yoff, ldx, m, ncols_ext, max_row_nnz, rect;
            if (std::scanf("%lld %lld %lld %lld %lld %lld %lld %lld %lld", &variant, &nc, &xoff, &yoff, &ldx, &m, &ncols_ext, &max_row_nnz, &rect) != 9) return 2;
            RowFacts f; // the way the serial tail of rails_spmm states it (spmm.hip: local_product, row_facts)
            f.variant = (int)variant, f.max_row_nnz = (int)max_row_nnz, f.m = m, f.ncols_ext = ncols_ext, f.rect = rect != 0;
            f.nc = (int)nc, f.ldx = f.ldg = (int)ldx;
            f.x_vec2 = (xoff & 1) == 0 && ldx % 2 == 0;
            f.y_vec2 = (yoff & 1) == 0;
            f.vec2 = ((xoff | yoff) & 1) == 0 && ldx % 2 == 0;
            f.xg_is_tail = rect != 0;
            const RowChoice ch = rails_row_choice(f);
            std::printf("%s\n", ch.kind == RowChoice::PLAIN ? "PLAIN" : ch.kind == RowChoice::CC ? "CC" : "NARROW");
        } else if (!std::strcmp(what, "cheb")) {
            long long m, ld;
            if (std::scanf("%lld %lld", &m, &ld) != 2) return 2;
            std::printf("%d\n", rails_cheb_fused_eligible(true, 0, m, ld) ? 1 : 0);
        } else
            return 2;
    }
    return 0;
}
