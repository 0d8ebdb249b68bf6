// bsr_choice.h -- how a block-CSR product is launched (spmm_bsr.hip: k_spmm_bsr<B, LPR>), from plain facts: the instantiation, the lanes
// that own a block row, the block rows a workgroup owns, the grid, and whether every workgroup's run of blocks is staged in LDS.  The rule
// and nothing else: plain arithmetic, no HIP, no I/O, no environment.  Checked on the host alone by tests/cpp/bsr_host.cpp, which also
// proves that every instantiation listed here is reached and none that is not listed.
//
// RAILS_BSR_TABLE is the list of instantiations spmm_bsr.hip compiles: it expands once into the constexpr table below and once into the
// switch of the launching function.  A choice outside the list is an error return there, never another kernel.
#ifndef RAILS_BSR_CHOICE_H
#define RAILS_BSR_CHOICE_H

#include <cstdint>

// X(B, LPR): k_spmm_bsr<B, LPR> -- B x B blocks, LPR lanes per block row (two columns each: chunks of 16 / 32 / 64 columns)
#define RAILS_BSR_TABLE(X)                                                                                                          \
    X(2, 8) X(2, 16) X(2, 32) X(3, 8) X(3, 16) X(3, 32) X(4, 8) X(4, 16) X(4, 32) X(5, 8) X(5, 16) X(5, 32) X(6, 8) X(6, 16) X(6, 32) \
    X(7, 8) X(7, 16) X(7, 32) X(8, 8) X(8, 16) X(8, 32)

constexpr int RAILS_BSR_LDS_DOUBLES = 4096; // values of the blocks a workgroup stages: 32 KiB, 1024 blocks at b = 2, 64 at b = 8

// threads of a workgroup: fewer for larger blocks, so that the block rows in flight (threads / LPR) keep their blocks within the buffer
constexpr int rails_bsr_threads(int b) { return b <= 4 ? 256 : b <= 6 ? 128 : 64; }
// blocks the LDS buffer holds
constexpr int rails_bsr_lds_blocks(int b) { return RAILS_BSR_LDS_DOUBLES / (b * b); }
// blocks whose X rows a lane loads before it multiplies: 8 to 5 rows of 16 bytes in flight
constexpr int rails_bsr_unroll(int b) { return b <= 2 ? 4 : b <= 4 ? 2 : 1; }
constexpr int rails_bsr_inst(int b, int lpr) { return (b << 8) | lpr; }

struct BsrFacts {
    int b = 0, nc = 0;
    bool y_vec2 = false;     // Y rows 16-byte aligned: a window on an even column of a panel with an even leading dimension
    int ldx = 0, ldy = 0;
    int64_t mb = 0;
    int64_t max_brow = 0;    // blocks of the longest block row
    int num_cu = 256;
};

struct BsrChoice {
    bool ok;         // false: no kernel for these facts (b outside 2 .. 8, no columns, no rows, a grid beyond 2^31)
    int b, lpr;      // the instantiation
    int threads;     // of a workgroup
    int rpg;         // block rows per lane group, one after the other
    int rows;        // block rows a workgroup owns: threads / lpr * rpg
    int64_t bpx;     // workgroups per XCD (the XCD-aware map of the row kernels); grid = 8 * bpx
    int64_t grid;
    bool y_vec;      // 16-byte stores
    bool all_staged; // every workgroup's run of blocks fits the buffer (a longer run takes the unstaged form, decided per workgroup)
    int key() const { return rails_bsr_inst(b, lpr); }
};

inline BsrChoice rails_bsr_choice(const BsrFacts &f)
{
    BsrChoice c{};
    if (f.b < 2 || f.b > 8 || f.nc < 1 || f.mb < 1 || f.max_brow < 0) return c;
    c.b = f.b;
    c.lpr = f.nc <= 16 ? 8 : f.nc <= 32 ? 16 : 32; // wider panels: the lanes loop over chunks of 64 columns
    c.threads = rails_bsr_threads(f.b);
    const int groups = c.threads / c.lpr, cap = rails_bsr_lds_blocks(f.b);
    // as many block rows per group as keep the longest possible run within the buffer and leave two workgroups per CU, at most four
    c.rpg = 1;
    while (c.rpg < 4 && (int64_t)groups * (2 * c.rpg) * (f.max_brow > 0 ? f.max_brow : 1) <= cap &&
           (f.mb + (int64_t)groups * 2 * c.rpg - 1) / ((int64_t)groups * 2 * c.rpg) >= 2 * (int64_t)(f.num_cu > 0 ? f.num_cu : 1))
        c.rpg *= 2;
    c.rows = groups * c.rpg;
    c.bpx = ((f.mb + c.rows - 1) / c.rows + 7) / 8;
    c.grid = c.bpx * 8;
    if (c.grid > 0x7fffffffLL) return c;
    c.y_vec = f.y_vec2;
    c.all_staged = (int64_t)c.rows * f.max_brow <= cap;
    c.ok = true;
    return c;
}

// ------------------------------------------------------------------------------------------- the table, for the host program ---
struct BsrInst {
    int b, lpr;
};
#define RAILS_BSR_INST(B, LPR) {B, LPR},
constexpr BsrInst kBsrTable[] = {RAILS_BSR_TABLE(RAILS_BSR_INST)};
#undef RAILS_BSR_INST

#endif
