// dense_choice.h -- which dense kernel takes a call (dense_gram.hip, dense_gemm.hip, dense_deferred.hip): from the shape of a call and
// the switches, the kernel family, its template integers and its launch geometry.  The rule and nothing else: plain arithmetic, no HIP,
// no I/O, no environment, no globals.  Checked on the host alone by tests/cpp/dense_choice_host.cpp, which also proves that every
// instantiation listed here is reached and none that is not listed.
//
// The RAILS_DENSE_*_TABLE lists are the instantiations the .hip files compile: each expands once into a constexpr table below (what the
// host program checks against) and once into the switch of the launching function.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace dense {

// What the rule depends on beside the shape.  The .hip side fills in what a primitive's rule reads (dense_common.h).
struct DenseSwitches {
    bool tile_fit = true;             // rails_dense_set_tile_fit / RAILS_DENSE_TILE_FIT
    bool update_gram_pipeline = true; // rails_dense_set_update_gram_pipeline / RAILS_UPDATE_GRAM_PIPELINE
    int gram_cols = 1;                // RAILS_GRAM_COLS
    int gram_extra_column = 1;        // RAILS_GRAM_EXTRA_COLUMN
    int fused_update_gram = 1;        // RAILS_FUSED_UPDATE_GRAM
    int panel_gemm_wide = 1;          // RAILS_PANEL_GEMM_WIDE
    int num_cu = 256;
};

// one number per instantiation: the case labels of the launching switches
constexpr int inst(int a, int b = 0, int c = 0) { return (a << 16) | (b << 8) | c; }

// rows that may be read 16 bytes at a time: an aligned first row and an even leading dimension
inline bool rows_vec_ok(const void *ptr, int ld) { return (((uintptr_t)ptr) & 15) == 0 && (ld % 2) == 0; }

// --------------------------------------------------------------------------------------------------------------------------- Gram ---
// X(TI, TJ): k_gram<TI, TJ>; k_gram2<TI, TJ>
#define RAILS_DENSE_GRAM_TABLE(X) X(1, 1) X(8, 1) X(1, 8) X(2, 2) X(4, 2) X(2, 4)
#define RAILS_DENSE_GRAM2_TABLE(X) X(1, 1) X(8, 1) X(4, 2)
// X(TI, TJ, NE): k_gram_cols<TI, TJ, NE> and k_gram_cols2<TI, TJ, NE>
#define RAILS_DENSE_GRAM_COLS_TABLE(X) X(4, 1, 0) X(5, 1, 0) X(6, 1, 0) X(4, 1, 1) X(5, 1, 1) X(6, 1, 1) X(3, 2, 0) X(4, 2, 0) X(5, 2, 0)

enum class GramForm { RowSplit, WideX };
struct GramChoice {
    GramForm form;
    int ti, tj, ne;      // k_gram[2]<ti, tj> (ne = 0) or k_gram_cols[2]<ti, tj, ne>
    int64_t nslab, rps;  // grid.x, rows per slab
    int ngj;             // row-split form: tile groups along Y (a kernel argument)
    unsigned grid_y;
    int key() const { return form == GramForm::WideX ? inst(ti, tj, ne) : inst(ti, tj); }
};

// row slabs of a Gram product (a x b): enough blocks to fill the chip, partial-tile traffic bounded to ~4% of the input
inline void gram_slabs(int64_t m, int a, int b, int64_t *nslab_out, int64_t *rps_out)
{
    double bound = 0.02 * (double)m * (double)(a + b) / ((double)a * (double)b);
    int64_t nslab = (int64_t)std::min<double>(1024.0, std::max<double>(1.0, bound));
    int64_t maxslab = (m + 15) / 16;
    if (nslab > maxslab) nslab = std::max<int64_t>(1, maxslab);
    int64_t rps = (m + nslab - 1) / nslab;
    rps = (rps + 15) / 16 * 16;
    if (rps < 16) rps = 16;
    *nslab_out = std::max<int64_t>(1, (m + rps - 1) / rps);
    *rps_out = rps;
}

// wide-X form: tiles of 16 X-columns per wave, the choice that leaves the fewest idle tile slots in blocks of four waves
// (one_tile: Y is one MFMA column tile, b <= 16 or the 17th column on the vector unit).  With the tile fit a one-tile form of six
// tiles per wave becomes one of five where five cover the columns with the same number of waves (19 and 20 tiles, 289 to 320
// columns: 20 slots instead of 24).  Not where five need a wave more: at 17 and 18 tiles six tiles keep three waves busy, the fourth
// leaves at once and costs nothing, and four waves of five measured 16 us slower (profiles/r11_tile_fit_kernels.md).
// (Eight tiles per wave cost 32 ceil(ntiles / 32) slots, never fewer than the 16 ceil(ntiles / 16) of four: that candidate is never taken.)
inline int gram_cols_tiles(int ntiles, bool one_tile, bool tile_fit)
{
    const int cand2[3] = {3, 4, 5}, cand1[3] = {4, 6, 8};
    const int *cand = one_tile ? cand1 : cand2;
    int best = cand[1], best_cost = 1 << 30;
    for (int q = 0; q < 3; ++q) {
        int ti = cand[q], strips = (ntiles + ti - 1) / ti, cost = (strips + 3) / 4 * 4 * ti;
        if (cost < best_cost) best = ti, best_cost = cost;
    }
    if (one_tile && best == 6 && (ntiles + 4) / 5 == (ntiles + 5) / 6 && tile_fit) best = 5;
    return best;
}

// the shapes of the wide-X form (the projections [P | X]' X of the coordinate-space back end); only for these does the rule read
// gram_cols, gram_extra_column and tile_fit
inline bool gram_wide_shape(int a, int b) { return b <= 32 && a >= 128; }

inline GramChoice gram_choice(int64_t m, int a, int b, bool two_segment, const DenseSwitches &sw)
{
    GramChoice g{};
    gram_slabs(m, a, b, &g.nslab, &g.rps);
    // (the two-segment operand has always ignored RAILS_GRAM_COLS and RAILS_GRAM_EXTRA_COLUMN)
    if (gram_wide_shape(a, b) && (two_segment || sw.gram_cols)) {
        // b = 17: one MFMA column tile and the 17th column on the vector unit (dense_gram_cols.inc)
        const bool extra = b == 17 && (two_segment || sw.gram_extra_column), one_tile = b <= 16 || extra;
        const int ntiles = (a + 15) / 16;
        g.form = GramForm::WideX;
        g.ti = gram_cols_tiles(ntiles, one_tile, sw.tile_fit);
        g.tj = one_tile ? 1 : 2;
        g.ne = extra ? 1 : 0;
        g.grid_y = (unsigned)(((ntiles + g.ti - 1) / g.ti + 3) / 4);
        return g;
    }
    g.form = GramForm::RowSplit;
    if (b <= 16)
        g.ti = a <= 16 ? 1 : 8, g.tj = 1;
    else if (two_segment)
        g.ti = 4, g.tj = 2;
    else if (a <= 16)
        g.ti = 1, g.tj = 8;
    else if (a <= 32 && b <= 32) // the block's own 17 x 17 Gram matrices of CholQR2
        g.ti = 2, g.tj = 2;
    else if (b <= 32)
        g.ti = 4, g.tj = 2;
    else
        g.ti = 2, g.tj = 4;
    g.ngj = (b + 16 * g.tj - 1) / (16 * g.tj);
    g.grid_y = (unsigned)((a + 16 * g.ti - 1) / (16 * g.ti) * g.ngj);
    return g;
}

// --------------------------------------------------------------------------------- the fused update + second projection ---
// X(NBW, NE): k_update_gram<NBW, NE> and k_update_gram_p<NBW, NE>
#define RAILS_DENSE_UPDATE_GRAM_TABLE(X) X(4, 0) X(4, 1) X(5, 0) X(5, 1) X(6, 0) X(6, 1) X(8, 0) X(8, 1)

struct UpdateGramChoice {
    bool fused;     // false: rails_panel_gemm_dev, then rails_gram_dev
    bool pipelined; // k_update_gram_p, or k_update_gram
    int nbw, ne;
    unsigned grid;
    int64_t ntiles;
    int key() const { return inst(nbw, ne); }
};

// rows_ok: X's rows may be read 16 bytes at a time and the columns between k and k rounded up to 4 are Y's own.
// One pass over X where the shapes allow (r <= 17, r2 <= 16, 32 <= k <= 512, at least 4096 rows), the two separate kernels otherwise.
inline UpdateGramChoice update_gram_choice(int64_t m, int k, int r, int r2, bool rows_ok, const DenseSwitches &sw)
{
    UpdateGramChoice u{};
    u.fused = sw.fused_update_gram && rows_ok && r <= 17 && r2 <= 16 && k >= 32 && k <= 512 && m >= 4096;
    if (!u.fused) return u;
    u.pipelined = sw.update_gram_pipeline;
    u.ntiles = (m + 15) / 16;
    u.grid = (unsigned)std::min<int64_t>(u.ntiles, 2 * (int64_t)std::max(sw.num_cu, 1));
    u.ne = r > 16 ? 1 : 0;
    if (k <= 256)
        u.nbw = 4;
    else if (k <= 320 && sw.tile_fit) // (the waves' interleaved blocks of 16 columns: 20 of them instead of 24)
        u.nbw = 5;
    else if (k <= 384)
        u.nbw = 6;
    else
        u.nbw = 8;
    return u;
}

// ------------------------------------------------------------------------------------------------------------------ panel GEMM ---
// X(TR, KC): k_panel_gemm<TR, KC>; k_panel_gemm2<TR, KC>
#define RAILS_DENSE_PANEL_GEMM_TABLE(X) X(1, 32) X(2, 32) X(4, 32) X(8, 32) X(16, 16)
#define RAILS_DENSE_PANEL_GEMM2_TABLE(X) X(1, 32) X(2, 32)

struct PanelGemmChoice {
    int tr, kc;
    int key() const { return inst(tr, kc); }
};

// r output columns (r <= 256: sixteen tiles)
inline PanelGemmChoice panel_gemm_choice(int r)
{
    const int tiles = (r + 15) / 16;
    if (tiles <= 1) return {1, 32};
    if (tiles <= 2) return {2, 32};
    if (tiles <= 4) return {4, 32};
    if (tiles <= 8) return {8, 32};
    return {16, 16};
}
// the two-segment operand: r <= 32
inline PanelGemmChoice panel_gemm2_choice(int r) { return {r <= 16 ? 1 : 2, 32}; }

// ------------------------------------------------------------------------------------------------------------- one-pass wide GEMM ---
// X(TR): k_panel_gemm_wide<TR>
#define RAILS_DENSE_GEMM_WIDE_TABLE(X) X(6) X(8) X(10) X(12) X(13) X(14) X(15) X(16) X(17) X(18)

struct GemmWideSlice {
    int j0, nc, tr; // output columns [j0, j0 + nc) by k_panel_gemm_wide<tr>
};
struct GemmWidePlan {
    bool own_kernel;   // false: rails_panel_gemm_dev in slices of 128 output columns
    bool tile_fit;
    int r, nslices, width;
    size_t ct_doubles; // the packed C of one slice (workspace: nslices of them)
    int count() const { return own_kernel ? (r + width - 1) / width : 0; }
    // Tiles of 16 output columns per wave: an even count, or with the tile fit the exact count where that is 13, 15 or 17 (a rank of
    // 257 to 272 after compress() is 17 tiles: as 18, one tile in eighteen of every k-step multiplied zeros).  Fewer than six tiles run
    // in the six-tile kernel.
    GemmWideSlice slice(int j) const
    {
        const int j0 = j * width, nc = std::min(width, r - j0), exact = (nc + 15) / 16;
        const int tr = (tile_fit && (exact == 13 || exact == 15 || exact == 17)) ? exact : (nc + 31) / 32 * 2;
        return {j0, nc, tr < 6 ? 6 : tr > 18 ? 18 : tr};
    }
};

// slices of equal width, at most 288 columns (18 tiles of 16: what a wave's registers hold), X read once per slice
inline GemmWidePlan gemm_wide_plan(int k, int r, const DenseSwitches &sw)
{
    GemmWidePlan p{};
    p.own_kernel = sw.panel_gemm_wide && r > 64 && k >= 32;
    p.tile_fit = sw.tile_fit;
    p.r = r;
    if (!p.own_kernel) return p;
    p.nslices = (r + 287) / 288;
    p.width = ((r + p.nslices - 1) / p.nslices + 15) / 16 * 16;
    p.ct_doubles = (size_t)((k + 31) / 32 * 32) * (16 * 18 + 4);
    return p;
}

// --------------------------------------------------------------------------------------------------- the tables, for the host program ---
struct Inst {
    int a, b, c;
};
#define RAILS_DENSE_INST2(A, B) {A, B, 0},
#define RAILS_DENSE_INST3(A, B, C) {A, B, C},
#define RAILS_DENSE_INST1(A) {A, 0, 0},
constexpr Inst kGram[] = {RAILS_DENSE_GRAM_TABLE(RAILS_DENSE_INST2)};
constexpr Inst kGram2[] = {RAILS_DENSE_GRAM2_TABLE(RAILS_DENSE_INST2)};
constexpr Inst kGramCols[] = {RAILS_DENSE_GRAM_COLS_TABLE(RAILS_DENSE_INST3)}; // one- and two-segment alike
constexpr Inst kUpdateGram[] = {RAILS_DENSE_UPDATE_GRAM_TABLE(RAILS_DENSE_INST2)}; // both schedules of each
constexpr Inst kPanelGemm[] = {RAILS_DENSE_PANEL_GEMM_TABLE(RAILS_DENSE_INST2)};
constexpr Inst kPanelGemm2[] = {RAILS_DENSE_PANEL_GEMM2_TABLE(RAILS_DENSE_INST2)};
constexpr Inst kGemmWide[] = {RAILS_DENSE_GEMM_WIDE_TABLE(RAILS_DENSE_INST1)};
#undef RAILS_DENSE_INST1
#undef RAILS_DENSE_INST2
#undef RAILS_DENSE_INST3

} // namespace dense
