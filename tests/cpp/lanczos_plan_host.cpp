// What the fused residual Lanczos decides without computing (rails_amd/csrc/lanczos_plan.h) alone, on the host: no HIP, no library.  Built
// by rails_amd/csrc/Makefile into rails_amd/lib/lanczos_plan_host, run by tests/test_lanczos_plan_host.py (which also builds it once more,
// as host code, under the address and undefined-behaviour sanitizers).  Prints ALL PASSED at the end.
//
// The rules the header replaced are written out below as they stood inside lanczos.hip (old_*: the checks, sizes and H loops of lz_run,
// the ten ifs of launch_pass with its sizing mode, pass_unroll, lz_unroll), and the header's answers are compared with them over the
// ranges of main().  Beside that: every plan's instantiation is a row of the table and every row is reached, the small block's parts
// follow one another without overlap with state, alphas and betas in one piece, H is assembled as the old loops did and nothing outside
// its (L+1) x (L+1) block is touched, and the refusals and the valid cases of the device tests get the verdicts they get there.
// With --table: one JSON line per instantiation and form, with the smallest k and the RAILS_LZ_UNROLL that reach it.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "lanczos_plan.h"

static long failed = 0, checks = 0;
// where a check failed: a text, or (in the innermost loops) a function that writes the text only when it is printed
static char where[256] = "";
static void (*where_late)() = nullptr;
#define AT(...) (where_late = nullptr, std::snprintf(where, sizeof where, __VA_ARGS__))
#define CHECK(cond)                                                                                                                            \
    do {                                                                                                                                       \
        ++checks;                                                                                                                              \
        if (!(cond)) {                                                                                                                         \
            ++failed;                                                                                                                          \
            if (where_late) where_late();                                                                                                      \
            if (failed <= 20) std::printf("line %d (%s): %s\n", __LINE__, where, #cond);                                                       \
        }                                                                                                                                      \
    } while (0)

// ------------------------------------------------------------------------------------------------- the rules as they stood ---
// lz_unroll (without its once-per-process cache) and pass_unroll
static int old_lz_unroll(const char *e)
{
    int u = e ? atoi(e) : 4;
    if (u != 1 && u != 2 && u != 4) u = 4;
    return u;
}
static int old_pass_unroll(int nch, const char *e)
{
    int u = old_lz_unroll(e);
    return (nch >= 3 && u > 2) ? 2 : u;
}

// launch_pass in sizing mode: the ten ifs with no final case; a pair outside the list left *nblocks_io as it was (0)
static bool old_launch_pass_listed(int nch, int u)
{
#define OLD_LZ_CASE(N, UU) \
    if (nch == N && u == UU) return true;
    OLD_LZ_CASE(1, 1) OLD_LZ_CASE(1, 2) OLD_LZ_CASE(1, 4) OLD_LZ_CASE(2, 1) OLD_LZ_CASE(2, 2) OLD_LZ_CASE(2, 4)
    OLD_LZ_CASE(3, 1) OLD_LZ_CASE(3, 2) OLD_LZ_CASE(4, 1) OLD_LZ_CASE(4, 2)
#undef OLD_LZ_CASE
    return false;
}
static void old_size_only(int nch, const char *env, int num_cu, bool query_ok, int occ, int *nblocks_io)
{
    if (!old_launch_pass_listed(nch, old_pass_unroll(nch, env))) return;
    if (!query_ok || occ < 1) occ = 2;
    if (occ > 4) occ = 4;
    *nblocks_io = num_cu * occ;
}

struct OldRun {
    int64_t mpad;
    size_t qbytes, nsmall, ws_bytes, pinned_bytes, start_pinned_bytes, nback;
    int ncoef, npart, nch, unroll, nblocks, last_step;
    size_t dT, dcoef, dsums, dstate, dalpha, dbeta, cleared;
    int random_grid;
    unsigned reduce_grid;
};

// the sizes of lz_run, statement by statement (SR: the sparse form; only_start: rails_lanczos_start)
static OldRun old_run(bool SR, bool only_start, int64_t m, int k, int p, int L, int num_cu, const char *env, bool query_ok, int query_value)
{
    OldRun o{};
    const int64_t mpad = (m + 63) / 64 * 64;
    o.qbytes = (size_t)(L + 2) * (size_t)std::max<int64_t>(mpad, 64) * sizeof(double);
    o.mpad = std::max<int64_t>(mpad, 64);
    const int ncoef = 2 * k + p + 1;
    const int npart = SR ? 2 * k + 1 : ncoef;
    int64_t ngroups = o.mpad / 64;
    const int nch = std::min(4, std::max(1, (k + 127) / 128));
    int nblocks = 0;
    old_size_only(nch, env, num_cu, query_ok, query_value, &nblocks);
    nblocks = (int)std::min<int64_t>((ngroups + 3) / 4, (int64_t)nblocks);
    if (nblocks < 1) nblocks = 1;
    o.nch = nch;
    o.unroll = old_pass_unroll(nch, env);
    o.nblocks = nblocks;
    size_t nsmall = (size_t)k * k + ncoef + ncoef + 8 + 2 * (size_t)(L + 2);
    o.nsmall = nsmall;
    o.dT = 0;
    o.dcoef = o.dT + (size_t)k * k;
    o.dsums = o.dcoef + ncoef;
    o.dstate = o.dsums + ncoef;
    o.dalpha = o.dstate + 8;
    o.dbeta = o.dalpha + (L + 2);
    o.ws_bytes = (size_t)nblocks * npart * sizeof(double);
    o.pinned_bytes = std::max<size_t>((size_t)k * k, (size_t)(2 * (L + 2) + 8)) * sizeof(double);
    o.cleared = nsmall - (size_t)k * k;
    o.random_grid = (int)std::min<int64_t>((o.mpad + 255) / 256, (int64_t)num_cu * 8);
    o.last_step = only_start ? 0 : L;
    o.reduce_grid = SR ? (unsigned)((npart + 63) / 64) : (unsigned)((ncoef + 63) / 64);
    o.start_pinned_bytes = only_start ? (size_t)ncoef * sizeof(double) : 0;
    o.nback = 8 + 2 * (size_t)(L + 2);
    o.ncoef = ncoef, o.npart = npart;
    return o;
}

// the RAILS_REQUIRE chain of lz_run: the text of the first one that fails, "" when none does
static std::string old_check(const lz::Call &q)
{
    const bool only_start = q.form == lz::Form::StartOnly, SR = q.form == lz::Form::SparseB;
    const int k = q.k, p = q.p, L = q.L, ldh = q.ldh, ldt = q.ldt, avc0 = q.avc0, mvc0 = q.mvc0, bc0 = q.bc0;
    char buf[256];
#define OLD_REQUIRE(cond, ...)                        \
    do {                                              \
        if (!(cond)) {                                \
            std::snprintf(buf, sizeof buf, __VA_ARGS__); \
            return buf;                               \
        }                                             \
    } while (0)
    OLD_REQUIRE(q.have_inputs && (only_start || q.have_outputs), "rails_resid_lanczos: null argument");
    OLD_REQUIRE(k >= 0 && p >= 0 && L >= 1 && (only_start || ldh >= L + 1), "rails_resid_lanczos: bad sizes k=%d p=%d L=%d ldh=%d", k, p, L, ldh);
    OLD_REQUIRE(avc0 >= 0 && avc0 + k <= q.av_cap && mvc0 >= 0 && mvc0 + k <= q.mv_cap && bc0 >= 0 && (SR || bc0 + p <= q.b_cap),
                "rails_resid_lanczos: column windows outside capacity");
    OLD_REQUIRE(q.av_m == q.mv_m && q.av_m == q.b_m, "rails_resid_lanczos: row mismatch");
    OLD_REQUIRE(((avc0 | mvc0 | bc0) & 1) == 0, "rails_resid_lanczos: column windows must start at even columns");
    OLD_REQUIRE(k <= 512 && (SR || p <= 128), "rails_resid_lanczos: fused kernel supports k <= 512, p <= 128 (got %d, %d)", k, p);
    OLD_REQUIRE(k == 0 || only_start || (q.have_T && ldt >= k), "rails_resid_lanczos: bad T");
#undef OLD_REQUIRE
    return "";
}

// the read-back of lz_run: hstate, halpha, hbeta into H
static int old_assemble(double *H_host, int ldh, int L, const double *hstate, const double *halpha, const double *hbeta)
{
    const bool broke = hstate[3] != 0.0;
    int steps = broke ? (int)hstate[4] : L;
    for (int j = 0; j <= L; ++j)
        for (int i = 0; i <= L; ++i) H_host[i + (size_t)j * ldh] = 0.0;
    for (int i = 0; i < steps; ++i) {
        H_host[i + (size_t)i * ldh] = halpha[i];
        bool last_broke = broke && (i == steps - 1);
        if (!last_broke) {
            H_host[(i + 1) + (size_t)i * ldh] = hbeta[i];
            H_host[i + (size_t)(i + 1) * ldh] = hbeta[i];
        }
    }
    return steps;
}

// -------------------------------------------------------------------------------------------------------------- the ranges ---
static const int64_t kM[] = {0, 1, 63, 64, 65, 255, 256, 257, 741, 2 * 262144 + 229, ((int64_t)1 << 31) + 5};
static const int kNumCu[] = {1, 8, 256, 304};
struct Query {
    bool ok;
    int value;
};
static const Query kQuery[] = {{false, 0}, {true, 0}, {true, 1}, {true, 2}, {true, 3}, {true, 4}, {true, 5}, {true, 8}};
static const char *const kEnv[] = {nullptr, "1", "2", "4", "0", "3", "8", "x"};
static const int kSparseP[] = {0, 1, 129, 1000};
template <typename T, size_t N>
static constexpr int count_of(const T (&)[N])
{
    return (int)N;
}

static lz::Form form_of(int f) { return f == 0 ? lz::Form::DenseB : f == 1 ? lz::Form::SparseB : lz::Form::StartOnly; }

static std::map<std::pair<int, int>, std::string> reached[2]; // [sparse]: (NCH, U) -> the JSON line of the first plan that reached it

static struct {
    int f, k, p, L, num_cu;
    int64_t m;
    const char *env;
    Query qu;
} cmp;
static void where_compare()
{
    std::snprintf(where, sizeof where, "form %d m %lld k %d p %d L %d num_cu %d env %s query %d/%d", cmp.f, (long long)cmp.m, cmp.k, cmp.p, cmp.L, cmp.num_cu,
                  cmp.env ? cmp.env : "(unset)", (int)cmp.qu.ok, cmp.qu.value);
}

static void compare(int f, int64_t m, int k, int p, int L, int num_cu, const char *env, Query qu)
{
    cmp = {f, k, p, L, num_cu, m, env, qu};
    where_late = where_compare;
    const lz::Form form = form_of(f);
    const OldRun o = old_run(f == 1, f == 2, m, k, p, L, num_cu, env, qu.ok, qu.value);
    const lz::Plan pl = lz::plan(form, m, k, p, L, num_cu, lz::unroll_setting(env), qu.ok, qu.value);
    CHECK(pl.mpad == o.mpad && pl.ngroups == o.mpad / 64 && pl.m == m);
    CHECK(pl.nch == o.nch && pl.unroll == o.unroll && pl.nblocks == o.nblocks);
    CHECK(pl.pass >= 0 && pl.pass < lz::kPassCount && lz::kPass[pl.pass].nch == pl.nch && lz::kPass[pl.pass].u == pl.unroll);
    CHECK(old_launch_pass_listed(pl.nch, pl.unroll));
    CHECK(pl.occ >= 1 && pl.occ <= 4 && pl.nblocks >= 1 && pl.nblocks <= std::max<int64_t>(1, (int64_t)num_cu * pl.occ));
    CHECK(pl.ncoef == o.ncoef && pl.npart == o.npart && pl.last_step == o.last_step);
    CHECK(pl.vector_bytes == o.qbytes && pl.ws_bytes == o.ws_bytes && pl.pinned_bytes == o.pinned_bytes && pl.start_pinned_bytes == o.start_pinned_bytes);
    CHECK((int)pl.random_grid == o.random_grid && pl.partial_grid == o.reduce_grid);
    const lz::SmallBlock &b = pl.small;
    CHECK(b.T == o.dT && b.coef == o.dcoef && b.sums == o.dsums && b.state == o.dstate && b.alphas == o.dalpha && b.betas == o.dbeta);
    CHECK(b.total == o.nsmall && b.cleared() == o.cleared && b.read_back() == o.nback);
    // increasing, one behind the other, state | alphas | betas in one piece up to the end
    CHECK(b.T == 0 && b.coef - b.T == (size_t)k * k && b.sums - b.coef == (size_t)pl.ncoef && b.state - b.sums == (size_t)pl.ncoef);
    CHECK(b.alphas - b.state == (size_t)lz::STATE_SLOTS && b.betas - b.alphas == (size_t)(L + 2) && b.total - b.betas == (size_t)(L + 2));
    CHECK(lz::STEPS < lz::STATE_SLOTS && pl.pinned_bytes >= b.read_back() * sizeof(double));
    const int sparse = f == 1;
    if (f != 2 && !reached[sparse].count({pl.nch, pl.unroll})) {
        char line[256];
        std::snprintf(line, sizeof line, "{\"kernel\": \"%s\", \"inst\": [%d, %d], \"k\": %d, \"unroll_env\": %s%s%s}", sparse ? "k_lanczos_pass_sparse" : "k_lanczos_pass",
                      pl.nch, pl.unroll, k, env ? "\"" : "", env ? env : "null", env ? "\"" : "");
        reached[sparse][{pl.nch, pl.unroll}] = line;
    }
}

// every k, p, L of every form, with m, num_cu, the occupancy result and the switch taken in turn from their lists (they do not enter what
// k, p and L decide); then every m, num_cu, occupancy result and switch setting against every k
static void check_plans()
{
    long turn = 0;
    for (int f = 0; f < 3; ++f)
        for (int k = 0; k <= 512; ++k)
            for (int pi = 0; pi < (f == 1 ? count_of(kSparseP) : 129); ++pi)
                for (int L = 1; L <= 64; ++L, ++turn)
                    compare(f, kM[turn % count_of(kM)], k, f == 1 ? kSparseP[pi] : pi, L, kNumCu[turn % count_of(kNumCu)], kEnv[(turn / 3) % count_of(kEnv)],
                            kQuery[(turn / 5) % count_of(kQuery)]);
    for (int f = 0; f < 3; ++f)
        for (int k = 0; k <= 512; ++k)
            for (int64_t m : kM)
                for (int num_cu : kNumCu)
                    for (const Query &qu : kQuery)
                        for (const char *env : kEnv) compare(f, m, k, f == 1 ? 129 : 5, 4, num_cu, env, qu);
    // the rule in words: NCH from k, U from the switch, the grid from the row groups and the resident blocks
    for (int k = 0; k <= 512; ++k) {
        AT("nch k %d", k);
        CHECK(lz::pass_nch(k) == (k <= 128 ? 1 : k <= 256 ? 2 : k <= 384 ? 3 : 4));
    }
    AT("grid");
    CHECK(lz::pass_blocks(1, 256, 2) == 1 && lz::pass_blocks(4, 256, 2) == 1 && lz::pass_blocks(5, 256, 2) == 2 && lz::pass_blocks(8194, 256, 2) == 512);
    CHECK(lz::pass_blocks(8194, 256, 4) == 1024 && lz::pass_blocks(0, 256, 4) == 1);
    CHECK(lz::pass_occupancy(false, 7) == 2 && lz::pass_occupancy(true, 0) == 2 && lz::pass_occupancy(true, 3) == 3 && lz::pass_occupancy(true, 8) == 4);
    // the table: ten rows, each reached in both forms, nothing else; a pair outside it is "not in the table"
    AT("table");
    CHECK(lz::kPassCount == 10 && reached[0].size() == 10 && reached[1].size() == 10);
    for (int nch = 0; nch <= 5; ++nch)
        for (int u = 0; u <= 8; ++u) {
            AT("table nch %d u %d", nch, u);
            const int i = lz::pass_index(nch, u);
            CHECK((i >= 0) == old_launch_pass_listed(nch, u));
            if (i >= 0) CHECK(lz::kPass[i].nch == nch && lz::kPass[i].u == u && reached[0].count({nch, u}) == 1 && reached[1].count({nch, u}) == 1);
        }
    for (int i = 0; i < lz::kPassCount; ++i)
        for (int j = 0; j < i; ++j) CHECK(lz::kPass[i].nch != lz::kPass[j].nch || lz::kPass[i].u != lz::kPass[j].u);
}

// ------------------------------------------------------------------------------------------------------- the side launches ---
static void check_side_launches()
{
    for (int p : {0, 1, 255, 256, 257, 1000, 70000})
        for (int64_t n_items : {(int64_t)0, (int64_t)1, (int64_t)3, (int64_t)4, (int64_t)5, (int64_t)100001})
            for (int64_t n_long : {(int64_t)0, (int64_t)1, (int64_t)4, (int64_t)5, (int64_t)999}) {
                AT("bt p %d items %lld long %lld", p, (long long)n_items, (long long)n_long);
                const lz::BtGrids g = lz::bt_grids(p, n_items, n_long);
                const int nshort = (p + 255) / 256; // lz_run: bt.nshort, grid, and the launch of k_sprhs_bt_long under n_long > 0
                const int64_t grid = nshort + (n_items + 3) / 4;
                CHECK(g.nshort == nshort && g.bt == grid && (g.bt_long > 0) == (n_long > 0) && (n_long == 0 || g.bt_long == (n_long + 3) / 4));
                CHECK((int64_t)g.nshort * 256 >= p && (g.bt - g.nshort) * 4 >= n_items && g.bt_long * 4 >= n_long);
            }
    for (int n = 0; n <= 1200; ++n) {
        AT("reduce n %d", n);
        CHECK(lz::reduce_grid(n) == (unsigned)((n + 63) / 64));
    }
    // rails_lanczos_vectors: for (j0 = 0; j0 < w; j0 += 16) wc = min(16, w - j0), grid (m + 255) / 256, steps * 16 doubles of LDS
    for (int64_t m : kM)
        for (int steps : {1, 7, 64})
            for (int w = 0; w <= 70; ++w) {
                AT("vectors m %lld steps %d w %d", (long long)m, steps, w);
                const lz::VectorsPlan v = lz::vectors_plan(m, steps, w);
                CHECK(v.s_bytes == (size_t)steps * w * sizeof(double) && v.grid == (unsigned)((m + 255) / 256));
                CHECK(lz::vectors_lds_bytes(steps) == (size_t)steps * 16 * sizeof(double));
                int ch = 0;
                for (int j0 = 0; j0 < w; j0 += 16, ++ch) {
                    int wc = std::min(16, w - j0);
                    CHECK(ch < v.nchunks && v.first(ch) == j0 && v.width(ch) == wc);
                }
                CHECK(ch == v.nchunks);
            }
}

// ------------------------------------------------------------------------------------------------------- the assembly of H ---
static void check_assembly()
{
    const double sentinel = -7.25;
    for (int L = 1; L <= 64; ++L)
        for (int pad = 0; pad <= 3; pad += 3)
            for (int broke = 0; broke <= 1; ++broke)
                for (int steps = 1; steps <= L; ++steps) {
                    AT("assembly L %d ldh %d broke %d steps %d", L, L + 1 + pad, broke, steps);
                    const int ldh = L + 1 + pad;
                    std::vector<double> back(lz::small_block(0, 1, L).read_back());
                    for (size_t i = 0; i < back.size(); ++i) back[i] = 100.0 + (double)i; // stale values everywhere: none may reach H but through the rule
                    back[lz::DONE] = broke ? 1.0 : 0.0;
                    back[lz::STEPS] = (double)steps;
                    const double *alphas = back.data() + lz::STATE_SLOTS, *betas = alphas + (L + 2);
                    std::vector<double> Hn((size_t)ldh * (L + 2), sentinel), Ho(Hn);
                    const int sn = lz::assemble_H(Hn.data(), ldh, L, back.data(), alphas, betas);
                    const int so = old_assemble(Ho.data(), ldh, L, back.data(), alphas, betas);
                    CHECK(sn == so && sn == (broke ? steps : L) && Hn == Ho);
                    bool outside = true;
                    for (int j = 0; j < L + 2; ++j)
                        for (int i = 0; i < ldh; ++i)
                            if (i > L || j > L) outside = outside && Hn[i + (size_t)j * ldh] == sentinel;
                    CHECK(outside);
                    CHECK(Hn[0] == alphas[0] && Hn[(size_t)(sn - 1) * (ldh + 1)] == alphas[sn - 1]);
                    if (broke) CHECK(Hn[sn + (size_t)(sn - 1) * ldh] == 0.0 && Hn[(sn - 1) + (size_t)sn * ldh] == 0.0); // no off-diagonal behind the breakdown
                    else CHECK(Hn[L + (size_t)(L - 1) * ldh] == betas[L - 1]);
                }
}

// ---------------------------------------------------------------------------------------------------------------- the checks ---
static lz::Call a_call(lz::Form form, int64_t m, int k, int p, int L, int avc0 = 0, int av_cap = -1, int mvc0 = 0, int mv_cap = -1, int bc0 = 0, int b_cap = -1)
{
    auto pad16 = [](int c) { return (std::max(c, 1) + 15) / 16 * 16; };
    lz::Call q;
    q.form = form;
    q.have_inputs = true;
    q.have_outputs = form != lz::Form::StartOnly;
    q.have_T = form != lz::Form::StartOnly;
    q.k = k, q.p = p, q.L = L;
    q.ldh = form == lz::Form::StartOnly ? 0 : L + 1;
    q.ldt = form == lz::Form::StartOnly ? 0 : std::max(1, k);
    q.avc0 = avc0, q.mvc0 = mvc0, q.bc0 = bc0;
    q.av_cap = av_cap < 0 ? pad16(k) : av_cap, q.mv_cap = mv_cap < 0 ? pad16(k) : mv_cap, q.b_cap = b_cap < 0 ? pad16(p) : b_cap;
    q.av_m = q.mv_m = q.b_m = m;
    return q;
}

static void verdict(const lz::Call &q, const char *expect) // expect: a substring of the refusal, or nullptr for "ok"
{
    const lz::Verdict v = lz::check(q);
    const std::string o = old_check(q);
    CHECK(v.ok == o.empty() && o == v.text);
    CHECK(v.ok == (expect == nullptr));
    if (expect) CHECK(std::strstr(v.text, expect) != nullptr);
}

static void check_checks()
{
    using lz::Form;
    // tests/test_gpu_lanczos_steps.py::test_refusals_launch_nothing: variations of a valid call with m = 40, k = 4, p = 2, L = 3
    const lz::Call base = a_call(Form::DenseB, 40, 4, 2, 3);
    lz::Call q;
    AT("refusals, dense");
    verdict(base, nullptr);
    q = base, q.avc0 = 1, verdict(q, "even columns");
    q = base, q.mvc0 = 3, verdict(q, "even columns");
    q = base, q.bc0 = 1, verdict(q, "even columns");
    lz::Call wide = a_call(Form::DenseB, 8, 4, 2, 3, 0, 528, 0, 528, 0, 144); // (T stays 4 x 4 there: ldt = 4)
    q = wide, q.k = 513, verdict(q, "k <= 512");
    q = wide, q.p = 129, verdict(q, "k <= 512");
    q = base, q.L = 0, q.ldh = 4, verdict(q, "bad sizes");
    q = base, q.ldh = 3, verdict(q, "bad sizes");
    q = base, q.mv_m = 41, verdict(q, "row mismatch");
    q = base, q.b_m = 39, verdict(q, "row mismatch");
    // tests/test_gpu_sparse_rhs.py::test_lanczos_refusals_launch_nothing: the first sparse case, m = 741, k = 6, p = 5, L = 4
    AT("refusals, sparse");
    const lz::Call sbase = a_call(Form::SparseB, 741, 6, 5, 4);
    verdict(sbase, nullptr);
    q = sbase, q.avc0 = 1, verdict(q, "even columns");
    q = sbase, q.mv_m = 740, verdict(q, "row mismatch");
    // the remaining texts
    AT("refusals, the other texts");
    q = base, q.have_inputs = false, verdict(q, "null argument");
    q = base, q.have_outputs = false, verdict(q, "null argument");
    q = base, q.avc0 = 14, verdict(q, "column windows outside capacity");
    q = base, q.bc0 = -2, verdict(q, "column windows outside capacity");
    q = base, q.have_T = false, verdict(q, "bad T");
    q = base, q.ldt = 3, verdict(q, "bad T");
    q = sbase, q.p = 1000, q.b_cap = 0, verdict(q, nullptr); // a sparse B has no panel and no limit on p
    q = a_call(Form::StartOnly, 741, 37, 3, 1, 2, 80, 40, 80, 6, 16), verdict(q, nullptr); // rails_lanczos_start: no T, no H
    q.have_outputs = false, q.ldh = 0, verdict(q, nullptr);
    // every valid case of tests/lanczos_reference.py ...
    AT("valid cases, dense");
    for (int k : {6, 128, 129, 255, 257, 384, 385, 512}) verdict(a_call(Form::DenseB, 741, k, 5, 4), nullptr);
    verdict(a_call(Form::DenseB, 330, 37, 3, 5, 2, 80, 40, 80, 6, 16), nullptr);
    verdict(a_call(Form::DenseB, 330, 37, 3, 5, 4, 48, 10, 64), nullptr);
    verdict(a_call(Form::DenseB, 330, 46, 3, 5, 2, 48, 18, 64, 12, 16), nullptr);
    for (int64_t m : {1, 63, 64, 65}) verdict(a_call(Form::DenseB, m, 2, 1, 2), nullptr);
    verdict(a_call(Form::DenseB, 200, 0, 3, 3), nullptr);
    verdict(a_call(Form::DenseB, 200, 4, 0, 3), nullptr);
    verdict(a_call(Form::DenseB, 2 * 262144 + 229, 6, 3, 3), nullptr);
    verdict(a_call(Form::DenseB, 500, 2, 1, 10), nullptr);
    // ... and of tests/sparse_rhs_reference.py, with its GRID_STRIDE
    AT("valid cases, sparse");
    verdict(a_call(Form::SparseB, 741, 6, 5, 4), nullptr);
    verdict(a_call(Form::SparseB, 741, 129, 300, 4), nullptr);
    verdict(a_call(Form::SparseB, 741, 37, 129, 5, 2, 80, 40, 80), nullptr);
    verdict(a_call(Form::SparseB, 330, 37, 200, 5, 4, 48, 10, 64), nullptr);
    verdict(a_call(Form::SparseB, 65, 2, 1, 2), nullptr);
    verdict(a_call(Form::SparseB, 64, 2, 3, 2), nullptr);
    verdict(a_call(Form::SparseB, 63, 2, 130, 2, 6, 16, 12, 16), nullptr);
    verdict(a_call(Form::SparseB, 1, 2, 1, 2), nullptr);
    verdict(a_call(Form::SparseB, 200, 0, 260, 3), nullptr);
    verdict(a_call(Form::SparseB, 200, 4, 0, 3), nullptr);
    verdict(a_call(Form::SparseB, 500, 2, 1, 10), nullptr);
    verdict(a_call(Form::SparseB, 741, 385, 16, 4), nullptr);
    verdict(a_call(Form::SparseB, 2 * 262144 + 229, 6, 1000, 3), nullptr);
    // the header against the old chain over a grid of calls around every limit, in all three forms
    for (int f = 0; f < 3; ++f)
        for (int k : {-1, 0, 1, 4, 512, 513})
            for (int p : {-1, 0, 2, 128, 129})
                for (int L : {0, 1, 3})
                    for (int c0 : {-2, 0, 1, 2, 14})
                        for (int which = 0; which < 3; ++which)
                            for (int flags = 0; flags < 16; ++flags) {
                                AT("grid of calls form %d k %d p %d L %d c0 %d which %d flags %d", f, k, p, L, c0, which, flags);
                                lz::Call g = a_call(form_of(f), 40, 4, 2, 3, 0, 16, 0, 528, 0, 144);
                                g.k = k, g.p = p, g.L = L;
                                (which == 0 ? g.avc0 : which == 1 ? g.mvc0 : g.bc0) = c0;
                                g.have_inputs = !(flags & 1), g.have_outputs = !(flags & 2), g.have_T = !(flags & 4);
                                g.ldh = (flags & 8) ? L : L + 1, g.ldt = (flags & 8) ? k - 1 : k, g.b_m = (flags & 8) && c0 == 2 ? 39 : 40;
                                const lz::Verdict v = lz::check(g);
                                CHECK(old_check(g) == v.text && v.ok == (v.text[0] == 0));
                            }
}

static void check_unroll()
{
    for (const char *env : kEnv)
        for (int nch = 1; nch <= 4; ++nch) {
            AT("unroll env %s nch %d", env ? env : "(unset)", nch);
            CHECK(lz::unroll_setting(env) == old_lz_unroll(env) && lz::pass_unroll(nch, lz::unroll_setting(env)) == old_pass_unroll(nch, env));
        }
}

int main(int argc, char **argv)
{
    const bool table = argc > 1 && !std::strcmp(argv[1], "--table");
    check_unroll();
    check_plans();
    check_side_launches();
    check_assembly();
    check_checks();
    if (table) {
        for (int sparse = 0; sparse < 2; ++sparse)
            for (const auto &kv : reached[sparse]) std::printf("%s\n", kv.second.c_str());
        return failed ? 1 : 0;
    }
    std::printf("%ld checks, %ld failed\n", checks, failed);
    if (!failed) std::printf("ALL PASSED\n");
    return failed ? 1 : 0;
}
