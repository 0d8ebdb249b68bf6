// Which kernel takes a product (rails_amd/csrc/op_choice.h: the whole-operator rule, serial and overlapped; rails_amd/csrc/row_choice.h: the
// row-kernel rule) alone, on the host: no HIP, no library.  Built by rails_amd/csrc/Makefile into rails_amd/lib/op_choice_host, run by
// tests/test_op_choice_host.py.  Prints ALL PASSED at the end.
#include <cstdio>
#include <initializer_list>

#include "op_choice.h"
#include "row_choice.h"

static int failed = 0, checks = 0;
#define CHECK(cond)                                                                                                                            \
    do {                                                                                                                                       \
        ++checks;                                                                                                                              \
        if (!(cond)) {                                                                                                                         \
            ++failed;                                                                                                                          \
            std::printf("line %d: %s\n", __LINE__, #cond);                                                                                     \
        }                                                                                                                                      \
    } while (0)

// ---- the whole-operator rule -----------------------------------------------------------------------------------------------------------
// the full-size banded operator of tests/test_gpu_sweep.py (banded_random(1000000, 27, 4096, seed=1): the mean window of a row is 7571
// X rows) and its smaller one (banded_random(140000, 27, 1000, seed=5): 1847) on a 256-CU device, all switches at their defaults
static OpFacts banded(int nc, int variant = 0)
{
    OpFacts f;
    f.variant = variant;
    f.max_row_nnz = 27;
    f.m = f.ncols_ext = 1000000;
    f.window_rows = 7571;
    f.int_hi = f.m;
    f.nc = nc;
    f.x_vec2 = f.y_vec2 = true;
    f.num_cu = 256;
    return f;
}
// the middle block of three of such an operator: 4096 ghost rows on either side, the rows within 4096 of an end are boundary rows
static OpFacts banded_block(int nc, int variant = 0)
{
    OpFacts f = banded(nc, variant);
    f.n_ghost = 8192;
    f.ncols_ext = f.m + f.n_ghost;
    f.int_lo = 4096;
    f.int_hi = f.m - 4096;
    f.window_rows = 9000; // (the boundary rows' ghost columns sit behind the local ones)
    f.window_rows_int = 7571;
    return f;
}

struct Grid {
    bool answer;
    int calls = 0;
    bool operator()()
    {
        ++calls;
        return answer;
    }
};

// the order as a string: S / P / T, upper case where forced
static const char *order_text(const OpOrder &o)
{
    static char buf[8];
    int n = 0;
    for (int i = 0; i < o.n; ++i) buf[n++] = (char)("spt"[o.step[i].kernel] - (o.step[i].forced ? 32 : 0));
    buf[n] = 0;
    return buf;
}
static bool order_is(const OpFacts &f, bool grid, const char *want, int want_calls = -1)
{
    Grid g{grid};
    const OpOrder o = rails_op_order(f, g);
    const char *got = order_text(o);
    bool same = true;
    int i = 0;
    for (; want[i] && got[i]; ++i) same = same && want[i] == got[i];
    same = same && want[i] == got[i] && (want_calls < 0 || g.calls == want_calls);
    if (!same) std::printf("  order '%s' after %d grid scans, expected '%s' after %d\n", got, g.calls, want, want_calls);
    return same;
}

static void sweep_shape()
{
    // the automatic choice at the three widths whose chunks of 16 columns divide an XCD's 32 workgroups.  128 columns (4 phases): the
    // full-size operator qualifies
    CHECK(rails_sweep_shape_worthwhile(1000000, 7571, 128));
    // 256 columns (2 phases): the window has to fit ONE row block, so the full-size operator does not qualify and the narrow band does
    CHECK(!rails_sweep_shape_worthwhile(1000000, 7571, 256));
    CHECK(rails_sweep_shape_worthwhile(140000, 1847, 256));
    CHECK(rails_sweep_shape_worthwhile(140000, 1847, 128));
    // 64 columns (8 phases): every X row would be staged by 8 workgroups per part before the window is counted -- the staging bound
    // phases x (part + window + 1024) <= 8 x part cannot hold, whatever the operator
    CHECK(!rails_sweep_shape_worthwhile(1000000, 7571, 64));
    CHECK(!rails_sweep_shape_worthwhile(1000000000, 1, 64));
    // widths outside the rule, and an operator without a window (no entries)
    CHECK(!rails_sweep_shape_worthwhile(1000000, 7571, 48));
    CHECK(!rails_sweep_shape_worthwhile(1000000, 7571, 512));
    CHECK(!rails_sweep_shape_worthwhile(1000000, 7571, 96)); // 6 chunks do not divide 32
    CHECK(!rails_sweep_shape_worthwhile(1000000, 7571, 136));
    for (int nc : {64, 128, 256}) CHECK(!rails_sweep_shape_worthwhile(1000000, 0, nc));
    // one row either side of each bound.  The window: window + 256 <= (phases - 1) row blocks
    CHECK(RAILS_SWEEP_BLOCK_ROWS == 22 * 8 * 16);
    CHECK(rails_sweep_shape_worthwhile(1000000, 3 * RAILS_SWEEP_BLOCK_ROWS - 256, 128));
    CHECK(!rails_sweep_shape_worthwhile(1000000, 3 * RAILS_SWEEP_BLOCK_ROWS - 255, 128));
    CHECK(rails_sweep_shape_worthwhile(1000000, RAILS_SWEEP_BLOCK_ROWS - 256, 256));
    CHECK(!rails_sweep_shape_worthwhile(1000000, RAILS_SWEEP_BLOCK_ROWS - 255, 256));
    // the rows: every XCD's part holds `phases` row blocks
    CHECK(rails_sweep_shape_worthwhile(8 * 4 * RAILS_SWEEP_BLOCK_ROWS, 1000, 128));
    CHECK(!rails_sweep_shape_worthwhile(8 * 4 * RAILS_SWEEP_BLOCK_ROWS - 1, 1000, 128));
    CHECK(rails_sweep_shape_worthwhile(8 * 2 * RAILS_SWEEP_BLOCK_ROWS, 1000, 256));
    CHECK(!rails_sweep_shape_worthwhile(8 * 2 * RAILS_SWEEP_BLOCK_ROWS - 1, 1000, 256));
    // the staging bound: at 128 and 256 columns the two bounds above imply it (the largest window against the smallest part:
    // 4 x (4 x 2816 + 3 x 2816 - 256 + 1024) <= 8 x 4 x 2816), so it never decides there ...
    CHECK(rails_sweep_shape_worthwhile(8 * 4 * RAILS_SWEEP_BLOCK_ROWS, 3 * RAILS_SWEEP_BLOCK_ROWS - 256, 128));
    CHECK(rails_sweep_shape_worthwhile(8 * 2 * RAILS_SWEEP_BLOCK_ROWS, RAILS_SWEEP_BLOCK_ROWS - 256, 256));
    // ... and at 64 columns it is the one that says no where the other two hold
    CHECK(8 * 8 * RAILS_SWEEP_BLOCK_ROWS <= 1000000 && 7571 + 256 <= 7 * RAILS_SWEEP_BLOCK_ROWS && !rails_sweep_shape_worthwhile(1000000, 7571, 64));

    // the plan of a built schedule
    CHECK(rails_sweep_plan_fits(true, 0.52, 3.7));
    CHECK(rails_sweep_plan_fits(true, 0.4, 8.0));
    CHECK(!rails_sweep_plan_fits(false, 0.52, 3.7));
    CHECK(!rails_sweep_plan_fits(true, 0.39, 3.7));
    CHECK(!rails_sweep_plan_fits(true, 0.52, 8.1));
}

static void serial_order()
{
    OpFacts f;
    // SWEEP, forced: variant 7 whatever the shape, nothing else, no grid scan
    CHECK(order_is(banded(128, 7), false, "S", 0));
    CHECK(order_is(banded(48, 7), false, "S", 0));
    CHECK(order_is(banded_block(128, 7), false, "S", 0)); // (the launcher refuses ghost rows itself)
    // SWEEP, automatic: variant 0, no ghost rows, a worthwhile shape, not a grid stencil; the box kernel stays behind it (the sweep
    // declines until its schedule exists).  One scan serves the sweep's and the planes' question
    CHECK(order_is(banded(128), false, "st", 1));
    CHECK(order_is(banded(128), true, "pt", 1)); // a grid stencil of that shape: the planes
    CHECK(order_is(banded(256), false, "t", 1)); // the window does not fit: no sweep (the scan is the planes' question)
    f = banded(128);
    f.window_rows = 0;
    CHECK(order_is(f, false, "t", 1));
    // PLANES, forced: variant 9
    CHECK(order_is(banded(128, 9), true, "P", 0));
    CHECK(order_is(banded(1, 9), false, "P", 0));
    // PLANES, automatic: variant 0, at least two columns, no ghost rows, not rectangular, RAILS_SPMM_PLANES, a grid stencil
    CHECK(order_is(banded(48), true, "pt", 1));
    CHECK(order_is(banded(48), false, "t", 1));
    CHECK(order_is(banded(2), true, "pt", 1));
    CHECK(order_is(banded(1), true, "t", 0));
    f = banded(48);
    f.planes = false;
    CHECK(order_is(f, true, "t", 0));
    f = banded(48);
    f.rect = true;
    CHECK(order_is(f, true, "t", 0));
    CHECK(order_is(banded_block(48), true, "t", 0));  // ghost rows: neither the planes nor a scan
    CHECK(order_is(banded_block(128), true, "t", 0)); // ... nor the sweep
    // TILED, forced: variants 2 and 6
    CHECK(order_is(banded(128, 2), true, "T", 0));
    CHECK(order_is(banded(16, 6), false, "T", 0));
    // TILED, automatic: variant 0 unless the lean row kernel is to have the product (8 < nc <= 16, rows of at most 64 entries, fewer than
    // 2^24 columns, both switches on)
    CHECK(order_is(banded(8), false, "t"));
    CHECK(order_is(banded(9), false, ""));
    CHECK(order_is(banded(16), false, ""));
    CHECK(order_is(banded(16), true, "p", 1)); // (the planes come before that question)
    CHECK(order_is(banded(17), false, "t"));
    f = banded(16);
    f.max_row_nnz = 65;
    CHECK(order_is(f, false, "t"));
    f = banded(16);
    f.ncols_ext = 1 << 24;
    CHECK(order_is(f, false, "t"));
    f = banded(16);
    f.narrow_cc = false;
    CHECK(order_is(f, false, "t"));
    f = banded(16);
    f.narrow_fast = false;
    CHECK(order_is(f, false, "t"));
    // the other variants go to the row kernels at once, without a scan
    for (int variant : {1, 3, 4, 5, 8}) {
        CHECK(order_is(banded(128, variant), true, "", 0));
        CHECK(order_is(banded(16, variant), true, "", 0));
    }
}

static void overlapped_order()
{
    // overlapped: the switch, ghost rows, not rectangular, variant 0 / 1 / 3, an interior of at least half the block and 1024 rows
    HaloOrder h = rails_halo_order(banded_block(128));
    CHECK(h.overlap);
    OpFacts f = banded_block(128);
    f.halo_overlap = false;
    CHECK(!rails_halo_order(f).overlap && rails_halo_order(f).interior.n == 0);
    CHECK(!rails_halo_order(banded(128)).overlap); // no ghost rows
    f = banded_block(128);
    f.rect = true;
    CHECK(!rails_halo_order(f).overlap);
    for (int variant = 0; variant <= 9; ++variant)
        CHECK(rails_halo_order(banded_block(128, variant)).overlap == (variant == 0 || variant == 1 || variant == 3));
    f = banded_block(16);
    f.m = 4000, f.int_lo = 1000, f.int_hi = 3000; // exactly half
    CHECK(rails_halo_order(f).overlap);
    f.int_hi = 2999;
    CHECK(!rails_halo_order(f).overlap);
    f.m = 1500, f.int_lo = 100, f.int_hi = 1124; // exactly 1024 rows
    CHECK(rails_halo_order(f).overlap);
    f.int_hi = 1123;
    CHECK(!rails_halo_order(f).overlap);
    // the interior rows: the planes, then the sweep, in automatic mode only
    CHECK(order_text(h.interior)[0] == 'p' && order_text(h.interior)[1] == 's' && h.interior.n == 2);
    CHECK(rails_halo_order(banded_block(128, 1)).interior.n == 0 && rails_halo_order(banded_block(128, 3)).interior.n == 0);
    f = banded_block(128);
    f.planes = false;
    CHECK(rails_halo_order(f).interior.n == 1 && rails_halo_order(f).interior.has(OpStep::SWEEP));
    // the interior sweep: aligned windows, a 256-CU device, 32-bit rows, and the shape test on the interior rows and their own window
    CHECK(!rails_halo_order(banded_block(48)).interior.has(OpStep::SWEEP) && rails_halo_order(banded_block(48)).interior.has(OpStep::PLANES));
    CHECK(!rails_halo_order(banded_block(256)).interior.has(OpStep::SWEEP));
    f = banded_block(128);
    f.x_vec2 = false;
    CHECK(!rails_halo_order(f).interior.has(OpStep::SWEEP));
    f = banded_block(128);
    f.y_vec2 = false;
    CHECK(!rails_halo_order(f).interior.has(OpStep::SWEEP));
    f = banded_block(128);
    f.num_cu = 128;
    CHECK(!rails_halo_order(f).interior.has(OpStep::SWEEP));
    f = banded_block(128);
    f.window_rows_int = 3 * RAILS_SWEEP_BLOCK_ROWS - 255; // (the whole block's window does not count)
    CHECK(!rails_halo_order(f).interior.has(OpStep::SWEEP));
    f.window_rows_int = 3 * RAILS_SWEEP_BLOCK_ROWS - 256, f.window_rows = 100000;
    CHECK(rails_halo_order(f).interior.has(OpStep::SWEEP));
    f = banded_block(128);
    f.m = 100000, f.int_lo = 4096, f.int_hi = 4096 + 8 * 4 * RAILS_SWEEP_BLOCK_ROWS - 1; // one interior row short
    CHECK(rails_halo_order(f).overlap && !rails_halo_order(f).interior.has(OpStep::SWEEP));
    f.int_hi += 1;
    CHECK(rails_halo_order(f).interior.has(OpStep::SWEEP));
}

static void prepare_choice()
{
    auto choice = [](const OpFacts &f, bool grid, int want_calls) {
        Grid g{grid};
        const PrepareChoice c = rails_prepare_choice(f, g);
        if (g.calls != want_calls) {
            std::printf("  %d grid scans, expected %d\n", g.calls, want_calls);
            return (PrepareChoice)-1;
        }
        return c;
    };
    // the sweep schedule where the sweep leads the serial order
    CHECK(choice(banded(128), false, 1) == PrepareChoice::SWEEP);
    CHECK(choice(banded(128, 7), false, 0) == PrepareChoice::SWEEP);
    CHECK(choice(banded_block(128, 7), false, 0) == PrepareChoice::SWEEP); // (rails_sweep_prepare reports that it does not fit)
    CHECK(choice(banded(128), true, 1) == PrepareChoice::NONE);
    CHECK(choice(banded(48), false, 0) == PrepareChoice::NONE);
    CHECK(choice(banded(128, 1), false, 0) == PrepareChoice::NONE);
    // the interior schedule where the product overlaps and its interior rows try the sweep, unless the planes take them
    CHECK(choice(banded_block(128), false, 1) == PrepareChoice::SWEEP_INTERIOR);
    CHECK(choice(banded_block(128), true, 1) == PrepareChoice::NONE);
    CHECK(choice(banded_block(48), false, 0) == PrepareChoice::NONE);
    CHECK(choice(banded_block(128, 1), false, 0) == PrepareChoice::NONE);
    // ... and not where the product would not overlap: the switch off, or an interior below half the block
    OpFacts f = banded_block(128);
    f.halo_overlap = false;
    CHECK(choice(f, false, 0) == PrepareChoice::NONE);
    f = banded_block(128);
    f.int_lo = f.m / 2 + 1;
    CHECK(choice(f, false, 0) == PrepareChoice::NONE);
}

// ---- the row-kernel rule --------------------------------------------------------------------------------------------------
// the flat operator of ROW_KERNEL_CASES in tests/test_gpu_kernels.py (3000 rows, 12 entries per row) the way the serial tail of rails_spmm
// states it: windows at column xoff / yoff of panels whose leading dimension is padded to a multiple of 16
static RowFacts flat(int variant, int nc, int xoff, int yoff)
{
    RowFacts f;
    f.variant = variant;
    f.max_row_nnz = 12;
    f.m = f.ncols_ext = 3000;
    f.nc = nc;
    f.ldx = f.ldg = (nc + xoff + 15) / 16 * 16;
    f.x_vec2 = (xoff & 1) == 0;
    f.y_vec2 = (yoff & 1) == 0;
    f.vec2 = ((xoff | yoff) & 1) == 0;
    return f;
}
static const RowChoice::Kind PLAIN = RowChoice::PLAIN, CC = RowChoice::CC, NARROW = RowChoice::NARROW;

static void row_kernels()
{
    // the outcomes test_row_kernel_choice asserts on the GPU, case by case
    for (int nc : {1, 2, 8}) CHECK(rails_row_choice(flat(1, nc, 0, 0)).kind == PLAIN);
    for (int nc : {9, 16, 17, 32}) CHECK(rails_row_choice(flat(1, nc, 0, 0)).kind == NARROW);
    CHECK(rails_row_choice(flat(1, 16, 0, 1)).kind == NARROW && !rails_row_choice(flat(1, 16, 0, 1)).y_vec);
    CHECK(rails_row_choice(flat(1, 16, 1, 0)).kind == NARROW);
    CHECK(rails_row_choice(flat(1, 17, 1, 0)).kind == PLAIN);
    CHECK(rails_row_choice(flat(1, 33, 0, 0)).kind == PLAIN);
    CHECK(rails_row_choice(flat(3, 16, 0, 0)).kind == PLAIN);
    CHECK(rails_row_choice(flat(4, 32, 0, 0)).kind == NARROW);
    CHECK(rails_row_choice(flat(4, 48, 0, 0)).kind == CC && rails_row_choice(flat(4, 48, 0, 0)).lpr == 16);
    CHECK(rails_row_choice(flat(4, 48, 0, 1)).kind == PLAIN);
    CHECK(rails_row_choice(flat(5, 64, 0, 0)).kind == PLAIN);
    CHECK(rails_row_choice(flat(5, 80, 0, 0)).kind == CC && rails_row_choice(flat(5, 80, 0, 0)).lpr == 32);
    RowFacts f = flat(1, 16, 0, 0); // test_row_kernel_choice_long_row: one row of 70 entries
    f.max_row_nnz = 70;
    CHECK(rails_row_choice(f).kind == PLAIN);

    // row 1 of the table: column chunks by variant or RAILS_SPMM_CHUNK (not on variant 3), serial, both windows aligned, wider than a chunk
    f = flat(1, 48, 0, 0);
    f.chunk_env = 32;
    CHECK(rails_row_choice(f).kind == CC && rails_row_choice(f).lpr == 16);
    f.chunk_env = 64;
    CHECK(rails_row_choice(f).kind == PLAIN);
    f = flat(3, 48, 0, 0);
    f.chunk_env = 32;
    CHECK(rails_row_choice(f).kind == PLAIN);
    f = flat(4, 48, 0, 0);
    f.span_ghost = 0; // a span never chunks a wide panel
    CHECK(rails_row_choice(f).kind == PLAIN);
    // row 2: the lean kernel, 8 lanes per row up to 16 columns, else 16; serial and spans, the ghost form where a span's rows may have
    // ghost columns
    CHECK(rails_row_choice(flat(1, 16, 0, 0)).lpr == 8 && rails_row_choice(flat(1, 17, 0, 0)).lpr == 16 && !rails_row_choice(flat(1, 16, 0, 0)).ghost);
    f = flat(0, 16, 0, 0);
    f.n_ghost = 100, f.ncols_ext = 3100, f.ldg = 16;
    f.span_ghost = 0;
    CHECK(rails_row_choice(f).kind == NARROW && !rails_row_choice(f).ghost);
    f.span_ghost = 1;
    CHECK(rails_row_choice(f).kind == NARROW && rails_row_choice(f).ghost);
    f.span_ghost = -1; // the serial product of a row block
    CHECK(rails_row_choice(f).kind == NARROW && rails_row_choice(f).ghost);
    f = flat(1, 16, 0, 0);
    f.rect = true, f.ncols_ext = 4000, f.xg_is_tail = true; // a rectangular operator whose extra rows follow X in the same panel: flat
    CHECK(rails_row_choice(f).kind == NARROW && !rails_row_choice(f).ghost);
    // row 3: the same where the lean kernel does not fit -- switched off, 2^24 columns, a panel of 4 GiB: one chunk of 16 / 32 columns
    f = flat(1, 16, 0, 0);
    f.narrow_fast = false;
    CHECK(rails_row_choice(f).kind == CC && rails_row_choice(f).lpr == 8);
    f = flat(1, 32, 0, 0);
    f.m = f.ncols_ext = 1 << 24;
    CHECK(rails_row_choice(f).kind == CC && rails_row_choice(f).lpr == 16);
    f = flat(1, 16, 0, 0);
    f.m = f.ncols_ext = 9000000, f.ldx = f.ldg = 64; // 9e6 x 64 x 8 bytes > 4 GiB
    CHECK(rails_row_choice(f).kind == CC);
    f.span_ghost = 0;
    CHECK(rails_row_choice(f).kind == CC);
    // row 4: X not aligned, 8 < c <= 16, serial only; where the lean kernel does not fit the plain one (the chunked one needs aligned X)
    f = flat(1, 16, 1, 0);
    f.span_ghost = 0;
    CHECK(rails_row_choice(f).kind == PLAIN);
    f = flat(1, 16, 1, 0);
    f.narrow_fast = false;
    CHECK(rails_row_choice(f).kind == PLAIN);
    CHECK(rails_row_choice(flat(1, 9, 1, 0)).kind == NARROW && rails_row_choice(flat(1, 8, 1, 0)).kind == PLAIN);
    // row 5: everything else -- RAILS_SPMM_NARROW_CC off, variant 3, wide panels: two columns per lane from two columns on, 1 to 64
    // lanes per row by the width
    f = flat(1, 16, 0, 0);
    f.narrow_cc = false;
    CHECK(rails_row_choice(f).kind == PLAIN && rails_row_choice(f).lpr == 8 && rails_row_choice(f).vec == 2);
    CHECK(rails_row_choice(flat(1, 1, 0, 0)).lpr == 1 && rails_row_choice(flat(1, 1, 0, 0)).vec == 2); // (aligned windows: the serial path's two)
    CHECK(rails_row_choice(flat(1, 1, 1, 0)).vec == 1);
    CHECK(rails_row_choice(flat(1, 2, 1, 1)).vec == 2 && rails_row_choice(flat(1, 2, 1, 1)).lpr == 1);
    CHECK(rails_row_choice(flat(3, 128, 0, 0)).lpr == 64 && rails_row_choice(flat(3, 64, 0, 0)).lpr == 32 && rails_row_choice(flat(3, 33, 0, 0)).lpr == 32 &&
          rails_row_choice(flat(3, 32, 0, 0)).lpr == 16 && rails_row_choice(flat(3, 8, 0, 0)).lpr == 4 && rails_row_choice(flat(3, 4, 0, 0)).lpr == 2);
}

int main()
{
    sweep_shape();
    serial_order();
    overlapped_order();
    prepare_choice();
    row_kernels();
    std::printf("%d checks, %d failed\n", checks, failed);
    std::printf(failed ? "FAILED\n" : "ALL PASSED\n");
    return failed ? 1 : 0;
}
