// Which dense kernel takes a call (rails_amd/csrc/dense_choice.h) alone, on the host: no HIP, no library.  Built by rails_amd/csrc/Makefile
// into rails_amd/lib/dense_choice_host, run by tests/test_dense_choice_host.py (which also builds it once more, as host code, under the
// address and undefined-behaviour sanitizers).  Prints ALL PASSED at the end.
//
// The launch chains the header replaced are written out below as they stood (old_*), and the header's answer is compared with them over
// every shape and switch setting of the ranges in main().  Beside that: every answer is an instantiation of the header's tables, every
// grid covers its tiles, the tile fit changes tile counts and nothing else, and the instantiations reached are exactly the tables'.
// With --table: one JSON line per instantiation, the smallest shape that reaches it, under the default switches where there is one
// (tests/test_gpu_dense_choice.py and scripts/dense_identity.py run these on the device).
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "dense_choice.h"

using namespace dense;

static long failed = 0, checks = 0;
// where a check failed: a format and the loop variables (formatted only when it is printed)
static const char *where_f = "";
static long long where_v[10];
template <typename... T>
static void at(const char *f, T... v)
{
    const long long vals[] = {(long long)v..., 0};
    where_f = f;
    for (size_t i = 0; i < sizeof...(T) && i < 10; ++i) where_v[i] = vals[i];
}
static void print_where(int line, const char *cond)
{
    char buf[512];
    const long long *w = where_v;
    std::snprintf(buf, sizeof buf, where_f, w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8], w[9]);
    std::printf("line %d (%s): %s\n", line, buf, cond);
}
#define CHECK(cond)                                                                                                                            \
    do {                                                                                                                                       \
        ++checks;                                                                                                                              \
        if (!(cond)) {                                                                                                                         \
            ++failed;                                                                                                                          \
            if (failed <= 20) print_where(__LINE__, #cond);                                                                                    \
        }                                                                                                                                      \
    } while (0)

// --------------------------------------------------------------------------------------------- the chains as they stood ---
struct OldLaunch {
    const char *kernel = "";
    int t[3] = {0, 0, 0};
    int64_t nslab = 0, rps = 0;
    unsigned grid_x = 0, grid_y = 0;
    int ngj = 0;
};

static void old_gram_slabs(int64_t m, int a, int b, int64_t *nslab_out, int64_t *rps_out)
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

static int old_gram_cols_tiles(int ntiles, bool one_tile, bool tile_fit)
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

static void old_launch_gram(OldLaunch &o, const char *kernel, int TI, int TJ, int a, int b)
{
    int ngi = (a + 16 * TI - 1) / (16 * TI), ngj = (b + 16 * TJ - 1) / (16 * TJ);
    o.kernel = kernel, o.t[0] = TI, o.t[1] = TJ, o.t[2] = 0;
    o.grid_x = (unsigned)o.nslab, o.grid_y = (unsigned)(ngi * ngj), o.ngj = ngj;
}

// the macro RAILS_GRAM_COLS
static void old_gram_cols(OldLaunch &o, const char *kernel, int a, int b, bool extra, bool tile_fit)
{
    const int ntiles = (a + 15) / 16, best = old_gram_cols_tiles(ntiles, b <= 16 || extra, tile_fit);
    o.kernel = kernel;
    o.grid_x = (unsigned)o.nslab, o.grid_y = (unsigned)(((ntiles + best - 1) / best + 3) / 4);
    if (extra)
        o.t[0] = best == 4 ? 4 : best == 5 ? 5 : best == 6 ? 6 : 8, o.t[1] = 1, o.t[2] = 1;
    else if (b <= 16)
        o.t[0] = best == 4 ? 4 : best == 5 ? 5 : best == 6 ? 6 : 8, o.t[1] = 1, o.t[2] = 0;
    else if (best == 3)
        o.t[0] = 3, o.t[1] = 2, o.t[2] = 0;
    else if (best == 4)
        o.t[0] = 4, o.t[1] = 2, o.t[2] = 0;
    else
        o.t[0] = 5, o.t[1] = 2, o.t[2] = 0;
}

static OldLaunch old_gram(int64_t m, int a, int b, const DenseSwitches &sw)
{
    OldLaunch o;
    old_gram_slabs(m, a, b, &o.nslab, &o.rps);
    if (b <= 16 && a <= 16)
        old_launch_gram(o, "k_gram", 1, 1, a, b);
    else if (b <= 32 && a >= 128) {
        if (sw.gram_cols) {
            const bool extra = sw.gram_extra_column && b == 17;
            old_gram_cols(o, "k_gram_cols", a, b, extra, sw.tile_fit);
        } else if (b <= 16)
            old_launch_gram(o, "k_gram", 8, 1, a, b);
        else
            old_launch_gram(o, "k_gram", 4, 2, a, b);
    } else if (b <= 16)
        old_launch_gram(o, "k_gram", 8, 1, a, b);
    else if (a <= 16)
        old_launch_gram(o, "k_gram", 1, 8, a, b);
    else if (a <= 32 && b <= 32)
        old_launch_gram(o, "k_gram", 2, 2, a, b);
    else if (b <= 32)
        old_launch_gram(o, "k_gram", 4, 2, a, b);
    else if (a <= 32)
        old_launch_gram(o, "k_gram", 2, 4, a, b);
    else
        old_launch_gram(o, "k_gram", 2, 4, a, b);
    return o;
}

static OldLaunch old_gram2(int64_t m, int a, int b, const DenseSwitches &sw)
{
    OldLaunch o;
    old_gram_slabs(m, a, b, &o.nslab, &o.rps);
    if (a >= 128 && b <= 32) {
        const bool extra = b == 17;
        old_gram_cols(o, "k_gram_cols2", a, b, extra, sw.tile_fit);
    } else if (a <= 16 && b <= 16)
        old_launch_gram(o, "k_gram2", 1, 1, a, b);
    else if (b <= 16)
        old_launch_gram(o, "k_gram2", 8, 1, a, b);
    else
        old_launch_gram(o, "k_gram2", 4, 2, a, b);
    return o;
}

struct OldUpdateGram {
    bool fused = false;
    int nbw = 0, ne = 0, form = 0;
    unsigned grid = 0;
    int64_t ntiles = 0;
};
static OldUpdateGram old_update_gram(int64_t m, int k, int r, int r2, bool rows_ok, const DenseSwitches &sw)
{
    OldUpdateGram o;
    if (sw.fused_update_gram && rows_ok && r <= 17 && r2 <= 16 && k >= 32 && k <= 512 && m >= 4096) {
        o.fused = true;
        o.ntiles = (m + 15) / 16;
        o.grid = (unsigned)std::min<int64_t>(o.ntiles, 2 * (int64_t)std::max(sw.num_cu, 1));
        const int ne = r > 16 ? r - 16 : 0;
        if (k <= 256)
            o.nbw = 4;
        else if (k <= 320 && sw.tile_fit)
            o.nbw = 5;
        else if (k <= 384)
            o.nbw = 6;
        else
            o.nbw = 8;
        // launch_update_gram<NBW>
        const bool pipeline = sw.update_gram_pipeline;
        o.ne = ne == 0 ? 0 : 1;
        o.form = pipeline ? 2 : 1;
    }
    return o;
}

static void old_panel_gemm(int r, int *TR, int *KC)
{
    int tr = (r + 15) / 16;
    if (tr <= 1)
        *TR = 1, *KC = 32;
    else if (tr <= 2)
        *TR = 2, *KC = 32;
    else if (tr <= 4)
        *TR = 4, *KC = 32;
    else if (tr <= 8)
        *TR = 8, *KC = 32;
    else
        *TR = 16, *KC = 16;
}
static void old_panel_gemm2(int r, int *TR, int *KC)
{
    if (r <= 16)
        *TR = 1, *KC = 32;
    else
        *TR = 2, *KC = 32;
}

struct OldWide {
    bool own = false;
    int nslices = 0, width = 0, n = 0;
    size_t ct_doubles = 0;
    int j0[8], nc[8], tr[8]; // (r <= 1200: at most five slices)
};
static OldWide old_gemm_wide(int k, int r, const DenseSwitches &sw)
{
    OldWide o;
    if (sw.panel_gemm_wide && r > 64 && k >= 32) {
        o.own = true;
        const int nslices = (r + 287) / 288, width = ((r + nslices - 1) / nslices + 15) / 16 * 16;
        o.nslices = nslices, o.width = width;
        o.ct_doubles = (size_t)((k + 31) / 32 * 32) * (16 * 18 + 4);
        int slice = 0;
        for (int j0 = 0; j0 < r; j0 += width, ++slice) {
            const int nc = std::min(width, r - j0), exact = (nc + 15) / 16;
            const int tr = (sw.tile_fit && (exact == 13 || exact == 15 || exact == 17)) ? exact : (nc + 31) / 32 * 2;
            int inst;
            switch (tr) {
            case 13: inst = 13; break;
            case 15: inst = 15; break;
            case 17: inst = 17; break;
            case 2: case 4: case 6: inst = 6; break;
            case 8: inst = 8; break;
            case 10: inst = 10; break;
            case 12: inst = 12; break;
            case 14: inst = 14; break;
            case 16: inst = 16; break;
            default: inst = 18; break;
            }
            if (slice < 8) o.j0[slice] = j0, o.nc[slice] = nc, o.tr[slice] = inst;
        }
        o.n = slice;
    }
    return o;
}

// ----------------------------------------------------------------------------------------------------- tables and reach ---
typedef std::vector<int> Key; // template integers
template <size_t N>
static std::set<Key> table_of(const Inst (&t)[N], int n)
{
    std::set<Key> s;
    for (const Inst &i : t) {
        Key k = {i.a, i.b, i.c};
        k.resize(n);
        s.insert(k);
    }
    return s;
}

// the first shape that reached an instantiation, per switch setting (the loops below go from small to large)
struct Reached {
    std::string line; // the JSON of the shape
    int rank;         // of the switch setting: 0 the defaults
};
static std::map<std::string, std::map<Key, Reached>> reached; // kernel -> instantiation -> first and best
static bool reach_is_news(const char *kernel, const Key &key, int rank)
{
    auto &m = reached[kernel];
    auto it = m.find(key);
    return it == m.end() || rank < it->second.rank;
}
static void reach(const char *kernel, const Key &key, int rank, const std::string &line) { reached[kernel][key] = Reached{line, rank}; }
static std::string fmt(const char *f, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, f);
    std::vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}
static void reach_equals_table(const char *kernel, const std::set<Key> &table)
{
    at(kernel);
    std::set<Key> got;
    for (const auto &kv : reached[kernel]) got.insert(kv.first);
    CHECK(got == table);
    for (const Key &k : table)
        if (!got.count(k)) std::printf("%s<%d, %d, %d> is never reached\n", kernel, k[0], k.size() > 1 ? k[1] : 0, k.size() > 2 ? k[2] : 0);
    for (const Key &k : got)
        if (!table.count(k)) std::printf("%s<%d, %d, %d> is reached and not in the table\n", kernel, k[0], k.size() > 1 ? k[1] : 0, k.size() > 2 ? k[2] : 0);
}

// ------------------------------------------------------------------------------------------------------------------ Gram ---
static void check_gram()
{
    const int64_t rows[] = {1, 15, 16, 17, 1003, 4099, 20011, 1000003};
    const std::set<Key> t_gram = table_of(kGram, 2), t_gram2 = table_of(kGram2, 2), t_cols = table_of(kGramCols, 3);
    for (int setting = 0; setting < 8; ++setting) {
        // 0: the defaults; then one switch off, two, three
        static const int off[8] = {0, 1, 2, 4, 3, 5, 6, 7};
        DenseSwitches sw, fit_on;
        sw.tile_fit = !(off[setting] & 1);
        sw.gram_cols = !(off[setting] & 2);
        sw.gram_extra_column = !(off[setting] & 4);
        fit_on = sw;
        fit_on.tile_fit = true;
        for (int a = 1; a <= 640; ++a)
            for (int b = 1; b <= 64; ++b)
                for (int two = 0; two < 2; ++two)
                    for (int64_t m : rows) {
                        at("gram two-segment %lld m %lld a %lld b %lld fit %lld cols %lld extra %lld", two, m, a, b, sw.tile_fit, sw.gram_cols, sw.gram_extra_column);
                        const GramChoice g = gram_choice(m, a, b, two != 0, sw);
                        const OldLaunch o = two ? old_gram2(m, a, b, sw) : old_gram(m, a, b, sw);
                        const bool wide = g.form == GramForm::WideX;
                        const char *kernel = wide ? (two ? "k_gram_cols2" : "k_gram_cols") : (two ? "k_gram2" : "k_gram");
                        CHECK(!std::strcmp(kernel, o.kernel));
                        CHECK(g.ti == o.t[0] && g.tj == o.t[1] && g.ne == o.t[2]);
                        CHECK(g.nslab == o.nslab && g.rps == o.rps);
                        CHECK((unsigned)g.nslab == o.grid_x && g.grid_y == o.grid_y);
                        if (!wide) CHECK(g.ngj == o.ngj);
                        // an instantiation of the table
                        const Key key = wide ? Key{g.ti, g.tj, g.ne} : Key{g.ti, g.tj};
                        CHECK((wide ? t_cols : two ? t_gram2 : t_gram).count(key) == 1);
                        CHECK(g.key() == (wide ? inst(g.ti, g.tj, g.ne) : inst(g.ti, g.tj)));
                        // the grid covers the rows and the tiles
                        CHECK(g.nslab >= 1 && g.rps % 16 == 0 && g.nslab * g.rps >= m && (g.nslab - 1) * g.rps < m);
                        if (wide) {
                            CHECK((int64_t)g.grid_y * 4 * g.ti * 16 >= a && 16 * g.tj + g.ne >= b);
                        } else {
                            const int ngi = (int)(g.grid_y / (unsigned)g.ngj);
                            CHECK(g.grid_y == (unsigned)(ngi * g.ngj) && ngi * 16 * g.ti >= a && g.ngj * 16 * g.tj >= b);
                        }
                        // the tile fit changes tile counts and nothing else
                        const GramChoice f = gram_choice(m, a, b, two != 0, fit_on);
                        CHECK(f.form == g.form && f.tj == g.tj && f.ne == g.ne && f.nslab == g.nslab && f.rps == g.rps && f.ngj == g.ngj);
                        if (m == 1003 && reach_is_news(kernel, key, setting))
                            reach(kernel, key, setting,
                                  fmt("{\"primitive\": \"%s\", \"kernel\": \"%s\", \"inst\": [%d, %d%s], \"m\": 1003, \"a\": %d, \"b\": %d, \"switches\": {\"tile_fit\": %d, "
                                      "\"gram_cols\": %d, \"gram_extra_column\": %d}}",
                                      two ? "gram2" : "gram", kernel, g.ti, g.tj, wide ? fmt(", %d", g.ne).c_str() : "", a, b, (int)sw.tile_fit, sw.gram_cols,
                                      sw.gram_extra_column));
                    }
    }
    reach_equals_table("k_gram", t_gram);
    reach_equals_table("k_gram2", t_gram2);
    reach_equals_table("k_gram_cols", t_cols);
    reach_equals_table("k_gram_cols2", t_cols);
}

// ----------------------------------------------------------------------------------------------------------- update-gram ---
static void check_update_gram()
{
    const int64_t rows[] = {4095, 4096, 4099, 1000003};
    const std::set<Key> table = table_of(kUpdateGram, 2);
    for (int setting = 0; setting < 8; ++setting) {
        static const int off[8] = {0, 1, 2, 4, 3, 5, 6, 7};
        DenseSwitches sw, fit_on;
        sw.tile_fit = !(off[setting] & 1);
        sw.update_gram_pipeline = !(off[setting] & 2);
        sw.fused_update_gram = !(off[setting] & 4);
        for (int num_cu : {256, 1}) {
            sw.num_cu = num_cu;
            fit_on = sw;
            fit_on.tile_fit = true;
            for (int k = 1; k <= 600; ++k)
                for (int r = 1; r <= 40; ++r)
                    for (int r2 = 1; r2 <= r; ++r2)
                        for (int64_t m : rows)
                            for (int rows_ok = 0; rows_ok < 2; ++rows_ok) {
                                const UpdateGramChoice u = update_gram_choice(m, k, r, r2, rows_ok != 0, sw);
                                const OldUpdateGram o = old_update_gram(m, k, r, r2, rows_ok != 0, sw);
                                at("update_gram m %lld k %lld r %lld r2 %lld rows_ok %lld fit %lld pipeline %lld fused %lld cu %lld", m, k, r, r2, rows_ok, sw.tile_fit,
                                   sw.update_gram_pipeline, sw.fused_update_gram, num_cu);
                                CHECK(u.fused == o.fused);
                                const UpdateGramChoice f = update_gram_choice(m, k, r, r2, rows_ok != 0, fit_on);
                                CHECK(f.fused == u.fused);
                                if (!u.fused) continue;
                                CHECK(u.nbw == o.nbw && u.ne == o.ne && u.grid == o.grid && u.ntiles == o.ntiles && (u.pipelined ? 2 : 1) == o.form);
                                CHECK(table.count(Key{u.nbw, u.ne}) == 1 && u.key() == inst(u.nbw, u.ne));
                                // the waves' blocks cover X's columns, the tile Y's; the workgroups stride over all tiles of 16 rows
                                CHECK(64 * u.nbw >= k && 16 + u.ne >= r && r2 <= 16);
                                CHECK(u.ntiles * 16 >= m && (u.ntiles - 1) * 16 < m && u.grid >= 1 && (int64_t)u.grid <= u.ntiles);
                                CHECK(f.ne == u.ne && f.grid == u.grid && f.ntiles == u.ntiles && f.pipelined == u.pipelined);
                                // (a shape a caller can make: where k is no multiple of 4, rows_ok needs the block to be at least that much wider)
                                if (m == 4099 && num_cu == 256 && r >= ((k + 3) & ~3) - k && reach_is_news(u.pipelined ? "k_update_gram_p" : "k_update_gram", Key{u.nbw, u.ne}, setting))
                                    reach(u.pipelined ? "k_update_gram_p" : "k_update_gram", Key{u.nbw, u.ne}, setting,
                                          fmt("{\"primitive\": \"update_gram\", \"kernel\": \"%s\", \"inst\": [%d, %d], \"m\": 4099, \"k\": %d, \"r\": %d, \"r2\": %d, \"switches\": "
                                              "{\"tile_fit\": %d, \"update_gram_pipeline\": %d}}",
                                              u.pipelined ? "k_update_gram_p" : "k_update_gram", u.nbw, u.ne, k, r, r2, (int)sw.tile_fit, (int)sw.update_gram_pipeline));
                            }
        }
    }
    reach_equals_table("k_update_gram", table);
    reach_equals_table("k_update_gram_p", table);
}

// ------------------------------------------------------------------------------------------------------------ panel GEMM ---
static void check_panel_gemm()
{
    const std::set<Key> table = table_of(kPanelGemm, 2), table2 = table_of(kPanelGemm2, 2);
    for (int r = 1; r <= 256; ++r) {
        at("panel_gemm r %lld", r);
        int TR, KC;
        old_panel_gemm(r, &TR, &KC);
        const PanelGemmChoice p = panel_gemm_choice(r);
        CHECK(p.tr == TR && p.kc == KC && table.count(Key{p.tr, p.kc}) == 1 && p.key() == inst(p.tr, p.kc));
        CHECK(16 * p.tr >= r);
        if (reach_is_news("k_panel_gemm", Key{p.tr, p.kc}, 0))
            reach("k_panel_gemm", Key{p.tr, p.kc}, 0, fmt("{\"primitive\": \"panel_gemm\", \"kernel\": \"k_panel_gemm\", \"inst\": [%d, %d], \"m\": 1003, \"r\": %d}", p.tr, p.kc, r));
    }
    for (int r = 1; r <= 32; ++r) {
        at("panel_gemm2 r %lld", r);
        int TR, KC;
        old_panel_gemm2(r, &TR, &KC);
        const PanelGemmChoice p = panel_gemm2_choice(r);
        CHECK(p.tr == TR && p.kc == KC && table2.count(Key{p.tr, p.kc}) == 1 && p.key() == inst(p.tr, p.kc));
        CHECK(16 * p.tr >= r);
        if (reach_is_news("k_panel_gemm2", Key{p.tr, p.kc}, 0))
            reach("k_panel_gemm2", Key{p.tr, p.kc}, 0, fmt("{\"primitive\": \"panel_gemm2\", \"kernel\": \"k_panel_gemm2\", \"inst\": [%d, %d], \"m\": 1003, \"r\": %d}", p.tr, p.kc, r));
    }
    reach_equals_table("k_panel_gemm", table);
    reach_equals_table("k_panel_gemm2", table2);
}

// ------------------------------------------------------------------------------------------------------------- wide GEMM ---
static void check_gemm_wide()
{
    const std::set<Key> table = table_of(kGemmWide, 1);
    for (int setting = 0; setting < 4; ++setting) {
        DenseSwitches sw, fit_on;
        sw.tile_fit = !(setting & 1);
        sw.panel_gemm_wide = !(setting & 2);
        fit_on = sw;
        fit_on.tile_fit = true;
        for (int k = 1; k <= 600; ++k)
            for (int r = 1; r <= 1200; ++r) {
                at("gemm_wide k %lld r %lld fit %lld wide %lld", k, r, sw.tile_fit, sw.panel_gemm_wide);
                const GemmWidePlan p = gemm_wide_plan(k, r, sw), f = gemm_wide_plan(k, r, fit_on);
                const OldWide o = old_gemm_wide(k, r, sw);
                CHECK(p.own_kernel == o.own && f.own_kernel == p.own_kernel);
                if (!p.own_kernel) {
                    CHECK(p.count() == 0);
                    continue;
                }
                CHECK(p.nslices == o.nslices && p.width == o.width && p.ct_doubles == o.ct_doubles && p.count() == o.n && o.n <= 8);
                CHECK(p.count() <= p.nslices); // (the workspace holds nslices packed copies of C)
                CHECK(f.nslices == p.nslices && f.width == p.width && f.ct_doubles == p.ct_doubles && f.count() == p.count());
                int covered = 0;
                for (int j = 0; j < p.count() && j < 8; ++j) {
                    const GemmWideSlice s = p.slice(j), fs = f.slice(j);
                    CHECK(s.j0 == o.j0[j] && s.nc == o.nc[j] && s.tr == o.tr[j]);
                    CHECK(s.j0 == covered && s.nc >= 1 && s.nc <= 288 && 16 * s.tr >= s.nc && table.count(Key{s.tr}) == 1);
                    // the packed rows of C (16 TR + 4 doubles) fit the slice's share of the workspace
                    CHECK((size_t)((k + 31) / 32 * 32) * (16 * s.tr + 4) <= p.ct_doubles);
                    CHECK(fs.j0 == s.j0 && fs.nc == s.nc);
                    covered += s.nc;
                    if (k == 32 && reach_is_news("k_panel_gemm_wide", Key{s.tr}, setting))
                        reach("k_panel_gemm_wide", Key{s.tr}, setting,
                              fmt("{\"primitive\": \"gemm_wide\", \"kernel\": \"k_panel_gemm_wide\", \"inst\": [%d], \"m\": 1003, \"k\": 32, \"r\": %d, \"slice\": %d, \"switches\": "
                                  "{\"tile_fit\": %d}}",
                                  s.tr, r, j, (int)sw.tile_fit));
                }
                CHECK(covered == r);
            }
    }
    reach_equals_table("k_panel_gemm_wide", table);
}

int main(int argc, char **argv)
{
    const bool table = argc > 1 && !std::strcmp(argv[1], "--table");
    check_gram();
    check_update_gram();
    check_panel_gemm();
    check_gemm_wide();
    // the alignment predicate: a 16-byte aligned first row and an even leading dimension
    at("rows_vec_ok");
    alignas(16) static double buf[4];
    CHECK(rows_vec_ok(buf, 2) && rows_vec_ok(buf + 2, 16) && !rows_vec_ok(buf + 1, 2) && !rows_vec_ok(buf, 3) && !rows_vec_ok(buf + 1, 3));
    if (table) {
        for (const auto &kernel : reached)
            for (const auto &kv : kernel.second) std::printf("%s\n", kv.second.line.c_str());
        return failed ? 1 : 0;
    }
    std::printf("%ld checks, %ld failed\n", checks, failed);
    if (!failed) std::printf("ALL PASSED\n");
    return failed ? 1 : 0;
}
