// lanczos_plan.h -- what the fused residual Lanczos (lanczos.hip) decides without computing: the three forms of a run, the argument
// checks and their texts, which instantiation of the pass kernel takes a run and on how many blocks, the widths and byte counts of its
// buffers, the layout of the small device block, the grids of the side launches, and the assembly of H from what is read back.  Plain
// arithmetic: no HIP, no environment, no globals (the one switch, RAILS_LZ_UNROLL, comes in as the string the caller read).  Checked on
// the host alone by tests/cpp/lanczos_plan_host.cpp against the rules as they stood inside lanczos.hip before this header.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

namespace lz {

// ------------------------------------------------------------------------------------------------------------------- the forms ---
// DenseB: rails_resid_lanczos; SparseB: rails_resid_lanczos_sparse (B is a rails_sprhs: no B panel, bc0 = 0); StartOnly:
// rails_lanczos_start (the init pass alone: no T, no H, L = 1)
enum class Form { DenseB, SparseB, StartOnly };

// ------------------------------------------------------------------------------------------------------------- the state slots ---
// the state doubles of the small block, shared by the pass, k_lz_small, k_sprhs_bt[_long] and the host's read-back
enum State : int {
    ALPHA = 0,     // alpha_i of the step the next pass takes
    BETA_PREV = 1, // beta_{i-1}
    INV_BETA = 2,  // 1 / beta_{i-1}: the pass normalises q_i with it
    DONE = 3,      // nonzero: the run has stopped (breakdown), every later launch returns at once
    STEPS = 4,     // steps completed so far
    STATE_SLOTS = 8
};

// ------------------------------------------------------------------------------------------------------------------ the checks ---
struct Call {
    Form form = Form::DenseB;
    bool have_inputs = false;  // context, AV, MV and B (or the sparse right-hand side)
    bool have_outputs = false; // H and steps (StartOnly: not asked for)
    bool have_T = false;
    int k = 0, p = 0, L = 0, ldh = 0, ldt = 0;
    int avc0 = 0, mvc0 = 0, bc0 = 0;       // first columns of the three windows
    int av_cap = 0, mv_cap = 0, b_cap = 0; // capacities of the panels (b_cap unused in the sparse form)
    int64_t av_m = 0, mv_m = 0, b_m = 0;   // rows of AV, MV and B
};

struct Verdict {
    bool ok = true;
    char text[160] = "";
};

// "ok", or the text of the first check that fails, in the order the checks have always had
inline Verdict check(const Call &q)
{
    Verdict v;
    const bool start = q.form == Form::StartOnly, sparse = q.form == Form::SparseB;
    auto refuse = [&v](const char *fmt, int a = 0, int b = 0, int c = 0, int d = 0) {
        v.ok = false;
        std::snprintf(v.text, sizeof v.text, fmt, a, b, c, d);
        return v;
    };
    if (!(q.have_inputs && (start || q.have_outputs))) return refuse("rails_resid_lanczos: null argument");
    if (!(q.k >= 0 && q.p >= 0 && q.L >= 1 && (start || q.ldh >= q.L + 1)))
        return refuse("rails_resid_lanczos: bad sizes k=%d p=%d L=%d ldh=%d", q.k, q.p, q.L, q.ldh);
    if (!(q.avc0 >= 0 && q.avc0 + q.k <= q.av_cap && q.mvc0 >= 0 && q.mvc0 + q.k <= q.mv_cap && q.bc0 >= 0 && (sparse || q.bc0 + q.p <= q.b_cap)))
        return refuse("rails_resid_lanczos: column windows outside capacity");
    if (!(q.av_m == q.mv_m && q.av_m == q.b_m)) return refuse("rails_resid_lanczos: row mismatch");
    if (((q.avc0 | q.mvc0 | q.bc0) & 1) != 0) return refuse("rails_resid_lanczos: column windows must start at even columns");
    if (!(q.k <= 512 && (sparse || q.p <= 128))) return refuse("rails_resid_lanczos: fused kernel supports k <= 512, p <= 128 (got %d, %d)", q.k, q.p);
    if (!(q.k == 0 || start || (q.have_T && q.ldt >= q.k))) return refuse("rails_resid_lanczos: bad T");
    return v;
}

// ------------------------------------------------------------------------------------------------------ the pass instantiation ---
// X(NCH, U): k_lanczos_pass<NCH, U> and k_lanczos_pass_sparse<NCH, U>.  Lane l owns the column pairs l + 64 c, c < NCH, of AV and MV;
// U rows are in flight per trip of the row loop (at NCH >= 3 more than two do not fit the registers).
#define RAILS_LZ_PASS_TABLE(X) X(1, 1) X(1, 2) X(1, 4) X(2, 1) X(2, 2) X(2, 4) X(3, 1) X(3, 2) X(4, 1) X(4, 2)

struct PassInst {
    int nch, u;
};
#define RAILS_LZ_PASS_INST(N, U) {N, U},
constexpr PassInst kPass[] = {RAILS_LZ_PASS_TABLE(RAILS_LZ_PASS_INST)};
#undef RAILS_LZ_PASS_INST
constexpr int kPassCount = (int)(sizeof(kPass) / sizeof(kPass[0]));

// the row of the table, or -1: not in the table
inline int pass_index(int nch, int u)
{
    for (int i = 0; i < kPassCount; ++i)
        if (kPass[i].nch == nch && kPass[i].u == u) return i;
    return -1;
}

inline int pass_nch(int k) { return std::min(4, std::max(1, (k + 127) / 128)); }

// RAILS_LZ_UNROLL as the caller read it (nullptr: not set): 1, 2 or 4, anything else is 4
inline int unroll_setting(const char *env)
{
    const int u = env ? std::atoi(env) : 4;
    return (u == 1 || u == 2 || u == 4) ? u : 4;
}

inline int pass_unroll(int nch, int setting) { return (nch >= 3 && setting > 2) ? 2 : setting; }

// ------------------------------------------------------------------------------------------------------------ the small block ---
// T | coef | sums | state | alphas | betas, in doubles from the start of the block.  State, alphas and betas are read back in one copy;
// everything behind T is cleared before a run.
struct SmallBlock {
    size_t T = 0, coef = 0, sums = 0, state = 0, alphas = 0, betas = 0, total = 0;
    size_t cleared() const { return total - coef; }   // doubles from coef on
    size_t read_back() const { return total - state; } // doubles from state on: state, alphas, betas
};

inline SmallBlock small_block(int k, int ncoef, int L)
{
    SmallBlock b;
    b.T = 0;
    b.coef = b.T + (size_t)k * k;
    b.sums = b.coef + (size_t)ncoef;
    b.state = b.sums + (size_t)ncoef;
    b.alphas = b.state + STATE_SLOTS;
    b.betas = b.alphas + (size_t)(L + 2);
    b.total = b.betas + (size_t)(L + 2);
    return b;
}

// -------------------------------------------------------------------------------------------------------------------- the plan ---
inline unsigned reduce_grid(int n) { return (unsigned)((n + 63) / 64); } // k_lz_reduce[_last_at]: 64 entries per block

// c'_B = B'r of the sparse form: k_sprhs_bt on `bt` blocks (the first nshort of them one thread per transposed row, the others one wave
// per item of a long row), then k_sprhs_bt_long on `bt_long` blocks (one wave per long row); 0 blocks: no launch
struct BtGrids {
    int nshort = 0;
    int64_t bt = 0, bt_long = 0;
};
inline BtGrids bt_grids(int p, int64_t n_items, int64_t n_long)
{
    BtGrids g;
    g.nshort = (p + 255) / 256;
    g.bt = g.nshort + (n_items + 3) / 4;
    g.bt_long = (n_long + 3) / 4;
    return g;
}

struct Plan {
    Form form = Form::DenseB;
    int k = 0, p = 0, L = 0;
    int64_t m = 0, mpad = 0, ngroups = 0; // rows, rows padded to whole groups of 64 (at least one), groups
    int nch = 0, unroll = 0, pass = -1;   // the instantiation and its row of kPass
    int occ = 0, nblocks = 0;             // resident blocks per CU counted on, blocks of the pass (each walks the groups with a grid stride)
    int ncoef = 0, npart = 0;             // [c'_AV | c'_MV | c'_B | rr]; entries of a block's partial sums (c'_B of a sparse B is not made by the pass)
    int last_step = 0;                    // the passes run step = -1 (init) .. last_step - 1
    SmallBlock small;
    size_t vector_bytes = 0, ws_bytes = 0, pinned_bytes = 0, start_pinned_bytes = 0;
    unsigned random_grid = 0, partial_grid = 0; // k_lz_random; the reduction of the partials
};

// The instantiation alone (the occupancy query needs it before the rest of the plan can be made).  pass = -1: not in the table.
inline void plan_pass(Plan &pl, int k, int setting)
{
    pl.nch = pass_nch(k);
    pl.unroll = pass_unroll(pl.nch, setting);
    pl.pass = pass_index(pl.nch, pl.unroll);
}

// occupancy counted on: 2 where the query failed or gave less than one block, at most 4
inline int pass_occupancy(bool query_ok, int query_value)
{
    const int occ = (!query_ok || query_value < 1) ? 2 : query_value;
    return std::min(occ, 4);
}

// the grid: resident blocks only, and no more than there are sets of four row groups (a block's four waves take one group each per trip)
inline int pass_blocks(int64_t ngroups, int num_cu, int occ)
{
    const int nblocks = (int)std::min<int64_t>((ngroups + 3) / 4, (int64_t)(num_cu * occ));
    return std::max(1, nblocks);
}

// setting: unroll_setting(getenv("RAILS_LZ_UNROLL")); query_ok / query_value: the occupancy query of the instantiation plan_pass names
inline Plan plan(Form form, int64_t m, int k, int p, int L, int num_cu, int setting, bool query_ok, int query_value)
{
    Plan pl;
    pl.form = form;
    pl.k = k, pl.p = p, pl.L = L, pl.m = m;
    pl.mpad = std::max<int64_t>((m + 63) / 64 * 64, 64);
    pl.ngroups = pl.mpad / 64;
    plan_pass(pl, k, setting);
    pl.occ = pass_occupancy(query_ok, query_value);
    pl.nblocks = pass_blocks(pl.ngroups, num_cu, pl.occ);
    pl.ncoef = 2 * k + p + 1;
    pl.npart = form == Form::SparseB ? 2 * k + 1 : pl.ncoef;
    pl.last_step = form == Form::StartOnly ? 0 : L;
    pl.small = small_block(k, pl.ncoef, L);
    pl.vector_bytes = (size_t)(L + 2) * (size_t)pl.mpad * sizeof(double);
    pl.ws_bytes = (size_t)pl.nblocks * pl.npart * sizeof(double);
    // the staging buffer holds T on the way up and state, alphas, betas on the way back; the start sums take a reserve of their own
    pl.pinned_bytes = std::max<size_t>((size_t)k * k, pl.small.read_back()) * sizeof(double);
    pl.start_pinned_bytes = form == Form::StartOnly ? (size_t)pl.ncoef * sizeof(double) : 0;
    pl.random_grid = (unsigned)std::min<int64_t>((pl.mpad + 255) / 256, (int64_t)num_cu * 8);
    pl.partial_grid = reduce_grid(pl.npart);
    return pl;
}

// ----------------------------------------------------------------------------------------------------- rails_lanczos_vectors ---
// Out[:, oc0 + j] for j < w from `steps` stored vectors: S is uploaded packed (steps x w), the kernel takes 16 columns per launch
struct VectorsPlan {
    size_t s_bytes = 0;
    unsigned grid = 0; // blocks of 256 rows
    int nchunks = 0;
    int w = 0;
    int first(int chunk) const { return 16 * chunk; }
    int width(int chunk) const { return std::min(16, w - 16 * chunk); }
};
inline VectorsPlan vectors_plan(int64_t m, int steps, int w)
{
    VectorsPlan v;
    v.w = w;
    v.s_bytes = (size_t)steps * w * sizeof(double);
    v.grid = (unsigned)((m + 255) / 256);
    v.nchunks = (w + 15) / 16;
    return v;
}
inline size_t vectors_lds_bytes(int steps) { return (size_t)steps * 16 * sizeof(double); }

// ----------------------------------------------------------------------------------------------------------- the assembly of H ---
// H ((L+1) x (L+1) of a column-major array with leading dimension ldh) from the state, alphas and betas read back; returns the steps
// taken.  A run that stopped early reports no off-diagonal entry for its last step (src/LyapunovSolver.hpp:428-429).
inline int assemble_H(double *H, int ldh, int L, const double *state, const double *alphas, const double *betas)
{
    const bool broke = state[DONE] != 0.0;
    const int steps = broke ? (int)state[STEPS] : L;
    for (int j = 0; j <= L; ++j)
        for (int i = 0; i <= L; ++i) H[i + (size_t)j * ldh] = 0.0; // H = 0.0 (:377)
    for (int i = 0; i < steps; ++i) {
        H[i + (size_t)i * ldh] = alphas[i]; // :407
        if (broke && i == steps - 1) break;
        H[(i + 1) + (size_t)i * ldh] = betas[i];
        H[i + (size_t)(i + 1) * ldh] = betas[i];
    }
    return steps;
}

} // namespace lz
