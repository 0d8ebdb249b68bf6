// itsolve.hip -- A^-1 X (or A^-T X) by an iteration that stays on the device, as a library object: the approximate inverse the reference
// allows for its inverse and extended Krylov projections (matlab/RAILSsolver.m:19-23, opts.Ainv: "This can be approximate") where a
// sparse LU (splu.hip) is latency-bound or cannot be formed at all.  Conjugate gradients for a definite operator of either sign,
// BiCGStab (right-preconditioned) for a general one, both with an optional Jacobi preconditioner; conjugate gradients also with a
// Chebyshev polynomial in the Jacobi-scaled operator ("poly_degree", cheb_coef.h), whose steps -- a product and its
// recurrence update -- are one kernel each for a stored CSR operator (k_cheb_step_csr); or, instead, with one V-cycle of smoothed-
// aggregation multigrid ("amg", amg_host.h for the set-up on the host, Run::vcycle below) that smooths with the
// same kernels and adds three of its own (k_amg_residual_csr, k_amg_prolong_add, k_amg_coarse_dense); or, for both methods, with block
// Jacobi ("block_jacobi", rails_iter_block_jacobi; block_jacobi_host.h for the blocks and their inverses on the host, DESIGN.md section
// 18): the inverses of the b x b diagonal blocks in place of the diagonal's, in block forms of the passes that apply it (k_cg_init_bj,
// k_cg_update_bj, k_bi_dir_bj, k_bi_s_bj, k_bj_apply on iter_pass_block), every pass of such a solve on slabs of whole block rows
// (rails_iter_pass_geom_block); or, for conjugate gradients on a block-CSR operator, with one V-cycle of block multigrid ("block_amg",
// rails_iter_block_amg_setup; block_amg_host.h for the set-up on the host): the same Run::vcycle on block-CSR level
// matrices with the inverse diagonal blocks as the smoother's G, the step fused with the block-CSR product on bsr_row_gather.inc
// (k_cheb_step_bsr, k_amg_residual_bsr) or unfused (k_cheb_init_bj, k_cheb_pass_bj), as block_amg_choice.h decides.  This file is the host code; the
// kernels are iter_kernels.inc, the geometry of a pass is iter_geom.h.  Both preconditioners are Chebyshev sweeps (struct Sweep,
// Run::sweep_start, Run::sweep_step); what a call needs of them -- coefficients, the choice of the fused step, geometry -- is its plan,
// made before anything is queued (begin_call, plan_call, plan_group), and every refusal is there.
//
// Every column is a system of its own with its own scalars (rails_iter_col, iter_scalars.h) in a device block the object owns: no block
// method, no small matrix on the host.  The iteration runs on work panels of the object (ordinary panels, window at column 0, so the
// SpMM kernels see the layout they are tested on and the passes below always load 16 bytes); X's window is copied in, the result copied
// out.  Solves of more than RAILS_ITER_GROUP columns run in groups.  The host queues `check_every` iterations, reads one number back
// through pinned memory (how many columns are still active) and stops when that is zero or max_iterations have been queued; a column
// that has stopped gets zero coefficients from the scalar step, so what is queued after it leaves its x alone and the result does not
// depend on check_every.
//
// Passes: thread (tx, ty) of a block owns the column pair 2 tx, 2 tx + 1 and every TY-th row of its block's slab (k_colnorms2's shape,
// dense_gram.hip), adds its rows in increasing order, the TY row classes meet in an LDS tree of fixed shape, the per-block partial sums go to
// the context workspace, and the one-workgroup kernel k_iter_scalars sums them over the blocks in a fixed order (iter_reduce) and then
// computes the scalars (iter_compute).  No floating-point atomics: two runs give the same bits.
//
// On a context that reduces (more than one rank, an all-reduce hook, a communicator) the two device functions are two kernels with an
// all-reduce of the sums between them (k_iter_reduce, rails_allreduce_dev, k_iter_compute): every rank holds the same scalars bit for bit,
// so every rank queues the same iterations and issues the same collectives.  A is then a row block with its ghost-row plan; the products
// exchange ghost rows inside rails_spmm, the fused polynomial step in its ghost-row form behind an exchange of the object's own.  What
// the ranks must agree on when the object is made is iter_agree.h.  DESIGN.md section 14, "On a row partition".
#include "rails_internal.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>

#include "amg_host.h"
#include "block_amg_choice.h"
#include "block_amg_host.h"
#include "block_jacobi_host.h"
#include "bsr_choice.h"
#include "cheb_coef.h"
#include "iter_agree.h"
#include "iter_geom.h"
#include "iter_scalars.h"

namespace {

constexpr int RAILS_ITER_GROUP = 32; // columns per group: the widest panel every SpMM kernel takes in one chunk
// default of "poly_ratio" (hi / lo): the smallest worst case of products relative to plain CG over the table of DESIGN.md section 15
constexpr double RAILS_ITER_POLY_RATIO = 10.0;
using PassGeom = rails_pass_geom; // (the name the kernels use)

#include "iter_kernels.inc"

// CG: x r p q [z]; BiCGStab: x r p v(=Q) [p^(=Z)] r^ t [s^]; the polynomial: z, its direction d, the second z of the fused step's ping-pong
enum { W_X = 0, W_R, W_P, W_Q, W_Z, W_RH, W_T, W_SH, W_D, W_Z2, W_COUNT };

// The multigrid hierarchy on the device (amg_host.h builds it on the host).  Level 0 works in the object's own work panels (r = W_R, z =
// W_Z / W_Z2, d = W_D, q = W_Q) on the object's operator; the levels below own their operators and five panels of the same row stride;
// the last matrix is its dense inverse with two panels (none when there is no level: W_R and W_Z then).  A call reaches every level's
// panels through its Sweep (plan_call), level 0's like the others.
enum { L_R = 0, L_Z, L_Z2, L_D, L_Q, L_COUNT };
struct AmgLevel {
    int64_t n = 0, nnz = 0;
    double hi = 0.0;
    rails_csr *A = nullptr; // level 0: the object's operator (not owned)
    rails_csr *P = nullptr, *R = nullptr;
    double *dinv = nullptr;
    double *ginv = nullptr; // the block hierarchy: the inverses of the level's diagonal blocks (dinv is null then)
    rails_panel *w[L_COUNT] = {};
};
struct Amg {
    std::vector<AmgLevel> lv;
    int64_t n_coarse = 0, coarse_nnz = 0;
    double *Ainv = nullptr;
    rails_panel *rc = nullptr, *zc = nullptr;
    int cols = 0; // columns of the level panels
    int b = 0;    // 0: the scalar hierarchy of "amg"; else the block size of the block hierarchy of "block_amg" 
    double host_seconds = 0.0, upload_seconds = 0.0;
};

} // namespace

struct rails_iter {
    rails_ctx *ctx = nullptr;
    rails_csr *A = nullptr;
    int method = 0;
    int64_t m = 0;
    double *dinv = nullptr; // 1 / diagonal (null: no preconditioner available)
    double defsign = 1.0;   // -1 when every diagonal entry is known and negative (CG without the preconditioner, iter_scalars.h)
    double tol = 1e-10;
    int maxit = 1000, jacobi = 1, check_every = 8, strict = 0;
    rails_panel *w[W_COUNT] = {};
    int work_cols = 0;
    rails_iter_col *cols_dev = nullptr;
    int cols_cap = 0;
    int32_t *status_dev = nullptr;
    void *pinned = nullptr;
    size_t pinned_bytes = 0;
    std::vector<rails_iter_col> last; // the columns of the last solve
    // statistics: last solve, totals
    long last_dots = 0, last_launches = 0, last_products = 0;
    // the Chebyshev polynomial preconditioner (cheb_coef.h): degree 0 is off
    int poly_degree = 0, poly_fused = 1;
    double poly_ratio = RAILS_ITER_POLY_RATIO, eig_max = 0.0;
    double hi_jacobi = 0.0, hi_plain = 0.0; // Gershgorin bounds on D^-1 A and on +-A from the host CSR arrays (0: none)
    long last_poly = 0, last_fused = 0;
    // a context that reduces (rails_allreduce_dev does something on it): the scalar step in three parts around an all-reduce of `sums_dev`
    bool reduces = false;
    double *sums_dev = nullptr; // 64 doubles
    long last_allreduces = 0, last_halo = 0; // all-reduces of the last call; ghost-row exchanges the object issued itself (fused steps)
    // the multigrid preconditioner ("amg"): off by default; the hierarchy is built on first use (rails_iter_amg_setup)
    int amg = 0, amg_degree = 1, amg_coarse = RAILS_AMG_COARSE;
    double amg_ratio = 4.0, amg_theta = RAILS_AMG_THETA;
    Amg *hier = nullptr;
    // the block multigrid preconditioner ("block_amg"): the same cycle on a block hierarchy (hier->b is the block size)
    int block_amg = 0;
    long last_cycles = 0, last_cycle_products = 0, last_cycle_launches = 0; // of the last call: cycles, and the products and launches inside them
    // block Jacobi ("block_jacobi"): the inverses of the m / bj_b diagonal blocks, row-major, on the device and as
    // uploaded on the host (rails_iter_block_jacobi_info); the setting is on only while there are blocks
    int block_jacobi = 0, bj_b = 0;
    double *bj_dev = nullptr;
    std::vector<double> bj_host;
    double tot_solves = 0, tot_iterations = 0, tot_flagged = 0, tot_products = 0, tot_columns = 0;
};

namespace {

void release_work(rails_iter *it)
{
    for (rails_panel *&p : it->w) {
        rails_panel_destroy(p);
        p = nullptr;
    }
    it->work_cols = 0;
}

void amg_release_panels(Amg *H)
{
    for (AmgLevel &L : H->lv)
        for (rails_panel *&p : L.w) {
            rails_panel_destroy(p);
            p = nullptr;
        }
    rails_panel_destroy(H->rc);
    rails_panel_destroy(H->zc);
    H->rc = H->zc = nullptr;
    H->cols = 0;
}

// drops the hierarchy (a changed "amg_theta" or "amg_coarse", a rebuild, the end of the object)
void amg_release(rails_iter *it)
{
    Amg *H = it->hier;
    if (!H) return;
    if (it->ctx) hipStreamSynchronize(it->ctx->stream);
    amg_release_panels(H);
    for (size_t l = 0; l < H->lv.size(); ++l) {
        AmgLevel &L = H->lv[l];
        if (l > 0) rails_csr_destroy(L.A);
        rails_csr_destroy(L.P);
        rails_csr_destroy(L.R);
        hipFree(L.dinv);
        hipFree(L.ginv);
    }
    hipFree(H->Ainv);
    delete H;
    it->hier = nullptr;
}

// the level panels follow the work panels: the same columns, so the same row stride; they grow only when a wider group arrives
int amg_grow(rails_ctx *c, rails_iter *it)
{
    Amg *H = it->hier;
    if (H->cols == it->work_cols) return RAILS_OK;
    amg_release_panels(H);
    for (size_t l = 1; l < H->lv.size(); ++l)
        for (rails_panel *&p : H->lv[l].w) RAILS_TRY(rails_panel_create(c, H->lv[l].n, it->work_cols, &p)); // (zeroed: the pad column is)
    if (!H->lv.empty()) {
        RAILS_TRY(rails_panel_create(c, H->n_coarse, it->work_cols, &H->rc));
        RAILS_TRY(rails_panel_create(c, H->n_coarse, it->work_cols, &H->zc));
    }
    H->cols = it->work_cols;
    return RAILS_OK;
}

// What the multigrid preconditioner refuses, by reason.  "amg" cannot be on without having passed here (rails_iter_set is the gate, and it
// holds the polynomial off afterwards), so a solve needs no check of its own; rails_iter_amg_setup, which may be called with "amg" off,
// checks again.  A sparse right-hand side or a rectangular operator never gets this far: rails_iter_create refuses them.
int amg_check(const rails_iter *it, const char *who)
{
    const rails_csr *A = it->A;
    RAILS_REQUIRE(it->method == RAILS_ITER_CG, "%s: \"amg\" on a BiCGStab object: the multigrid preconditioner is for conjugate gradients (a symmetric definite operator)", who);
    RAILS_REQUIRE(it->poly_degree == 0, "%s: \"amg\" together with poly_degree %d: one preconditioner at a time", who, it->poly_degree);
    RAILS_REQUIRE(!it->block_jacobi, "%s: \"amg\" together with \"block_jacobi\": one preconditioner at a time", who);
    RAILS_REQUIRE(!it->block_amg, "%s: \"amg\" together with \"block_amg\": one preconditioner at a time", who);
    RAILS_REQUIRE(A->kind != rails_csr::CALLBACK, "%s: \"amg\" needs the entries of the matrix: the operator is a callback", who);
    RAILS_REQUIRE(A->kind != rails_csr::LU && A->kind != rails_csr::ITER, "%s: \"amg\" needs the entries of the matrix: the operator is an LU or an iterative solve", who);
    RAILS_REQUIRE(A->kind != rails_csr::BSR, "%s: \"amg\" needs the entries of the matrix as scalar CSR arrays: the operator is block-CSR (keep a CSR handle for the preconditioner)", who);
    RAILS_REQUIRE(!it->reduces && A->n_ghost == 0 && A->n_send == 0,
                  "%s: \"amg\" on a context that reduces (more than one rank, an all-reduce hook or a communicator): the multigrid preconditioner is single GPU", who);
    RAILS_REQUIRE(it->m < ((int64_t)1 << 24), "%s: \"amg\" on %lld rows: the multigrid preconditioner takes fewer than 2^24", who, (long long)it->m);
    return RAILS_OK;
}

// What the block multigrid preconditioner refuses before it looks at the entries (block_amg_host.cpp refuses those), by reason; nothing
// here touches the device.  rails_iter_set is the gate of "block_amg" as it is of "amg"; rails_iter_block_amg_setup checks again.
int bamg_check(const rails_iter *it, const char *who)
{
    const rails_csr *A = it->A;
    RAILS_REQUIRE(it->method == RAILS_ITER_CG, "%s: \"block_amg\" on a BiCGStab object: the multigrid preconditioner is for conjugate gradients (a symmetric definite operator)", who);
    RAILS_REQUIRE(it->poly_degree == 0, "%s: \"block_amg\" together with poly_degree %d: one preconditioner at a time", who, it->poly_degree);
    RAILS_REQUIRE(!it->block_jacobi, "%s: \"block_amg\" together with \"block_jacobi\": one preconditioner at a time", who);
    RAILS_REQUIRE(!it->amg, "%s: \"block_amg\" together with \"amg\": one preconditioner at a time", who);
    int b = 0;
    int64_t mb = 0;
    const int64_t *browptr = nullptr;
    const int32_t *bcol = nullptr;
    const double *bval = nullptr;
    RAILS_REQUIRE(A->kind == rails_csr::BSR && rails_bsr_host_arrays(A, &b, &mb, &browptr, &bcol, &bval),
                  "%s: \"block_amg\" needs the blocks of the matrix: the operator is not a block-CSR handle with a host copy (rails_csr_create_bsr)", who);
    RAILS_REQUIRE(!it->reduces, "%s: \"block_amg\" on a context that reduces (more than one rank, an all-reduce hook or a communicator): the multigrid preconditioner is single GPU", who);
    RAILS_REQUIRE(rails_bamg_rows_ok(it->m, b), "%s: \"block_amg\" on %lld rows of block size %d: the multigrid cycle's kernels address fewer than 2^24 rows", who,
                  (long long)it->m, b);
    return RAILS_OK;
}

bool uses_panel(const rails_iter *it, int which)
{
    const bool jac = it->dinv != nullptr || it->bj_dev != nullptr;
    const bool mg = it->amg || it->block_amg;
    if (which == W_D || which == W_Z2) return it->poly_degree > 0 || mg;
    if (which == W_Z && (it->poly_degree > 0 || mg)) return true;
    if (it->method == RAILS_ITER_CG) return which == W_X || which == W_R || which == W_P || which == W_Q || (which == W_Z && jac);
    return which == W_X || which == W_R || which == W_P || which == W_Q || which == W_RH || which == W_T || ((which == W_Z || which == W_SH) && jac);
}

// `also`: panels (bits 1 << W_...) wanted beside those the method uses (rails_iter_precondition)
int grow_work(rails_ctx *c, rails_iter *it, int cols, unsigned also = 0)
{
    bool missing = false; // a setting made after the last solve may ask for a panel that is not there yet
    for (int k = 0; k < W_COUNT; ++k) missing = missing || ((uses_panel(it, k) || (also >> k & 1)) && !it->w[k]);
    if (cols <= it->work_cols && !missing) return RAILS_OK;
    cols = std::max(cols, it->work_cols);
    for (int k = 0; k < W_COUNT; ++k) also |= it->w[k] ? 1u << k : 0u;
    release_work(it);
    for (int k = 0; k < W_COUNT; ++k)
        if (uses_panel(it, k) || (also >> k & 1)) {
            RAILS_TRY(rails_panel_create(c, it->m, cols, &it->w[k]));
            RAILS_HIP_CHECK(hipMemsetAsync(it->w[k]->d, 0, (size_t)it->m * it->w[k]->ld * sizeof(double), c->stream));
        }
    it->work_cols = cols;
    return RAILS_OK;
}

int grow_cols(rails_ctx *c, rails_iter *it, int nc)
{
    if (nc > it->cols_cap) {
        RAILS_HIP_CHECK(hipStreamSynchronize(c->stream));
        if (it->cols_dev) RAILS_HIP_CHECK(hipFree(it->cols_dev));
        it->cols_dev = nullptr;
        it->cols_cap = 0;
        const int cap = (nc + 31) / 32 * 32;
        RAILS_HIP_CHECK(hipMalloc((void **)&it->cols_dev, (size_t)cap * sizeof(rails_iter_col)));
        it->cols_cap = cap;
        c->n_dev_alloc++;
    }
    const size_t want = 64 + (size_t)it->cols_cap * sizeof(rails_iter_col);
    if (want > it->pinned_bytes) {
        RAILS_HIP_CHECK(hipStreamSynchronize(c->stream));
        if (it->pinned) RAILS_HIP_CHECK(hipHostFree(it->pinned));
        it->pinned = nullptr;
        it->pinned_bytes = 0;
        RAILS_HIP_CHECK(hipHostMalloc(&it->pinned, want, hipHostMallocDefault));
        it->pinned_bytes = want;
    }
    return RAILS_OK;
}

// The block forms of the passes that apply G, by block size: one switch per kernel, expanded from RAILS_BJ_TABLE (iter_kernels.inc).  A
// block size outside the table gives a null pointer, which the call refuses before anything is queued (begin_call).
#define RAILS_BJ_PICK(fn, expr)                                                                                                                   \
    auto fn(int b, bool trans)->decltype(expr(2))                                                                                                   \
    {                                                                                                                                             \
        (void)trans;                                                                                                                              \
        switch (b) {                                                                                                                              \
            RAILS_BJ_TABLE(expr##_CASE)                                                                                                           \
        default: return nullptr;                                                                                                                  \
        }                                                                                                                                         \
    }
#define BJ_CG_INIT(B) (&k_cg_init_bj<B>)
#define BJ_CG_INIT_CASE(B) case B: return BJ_CG_INIT(B);
#define BJ_CG_UPDATE(B) (&k_cg_update_bj<B>)
#define BJ_CG_UPDATE_CASE(B) case B: return BJ_CG_UPDATE(B);
#define BJ_APPLY(B) (&k_bj_apply<B>)
#define BJ_APPLY_CASE(B) case B: return BJ_APPLY(B);
#define BJ_BI_DIR(B) (trans ? &k_bi_dir_bj<B, true> : &k_bi_dir_bj<B, false>)
#define BJ_BI_DIR_CASE(B) case B: return BJ_BI_DIR(B);
#define BJ_BI_S(B) (trans ? &k_bi_s_bj<B, true> : &k_bi_s_bj<B, false>)
#define BJ_BI_S_CASE(B) case B: return BJ_BI_S(B);
RAILS_BJ_PICK(bj_cg_init, BJ_CG_INIT)
RAILS_BJ_PICK(bj_cg_update, BJ_CG_UPDATE)
RAILS_BJ_PICK(bj_apply, BJ_APPLY)
RAILS_BJ_PICK(bj_bi_dir, BJ_BI_DIR)
#define BJ_CHEB_INIT(B) (&k_cheb_init_bj<B>)
#define BJ_CHEB_INIT_CASE(B) case B: return BJ_CHEB_INIT(B);
#define BJ_CHEB_PASS(B) (&k_cheb_pass_bj<B>)
#define BJ_CHEB_PASS_CASE(B) case B: return BJ_CHEB_PASS(B);
RAILS_BJ_PICK(bj_bi_s, BJ_BI_S)
RAILS_BJ_PICK(bj_cheb_init, BJ_CHEB_INIT)
RAILS_BJ_PICK(bj_cheb_pass, BJ_CHEB_PASS)
#undef RAILS_BJ_PICK

// A Chebyshev sweep on an operator: z = p(G A) G r by d = z = G r / theta, then steps d = a d + b G (r - A z), z += d.  The polynomial
// preconditioner is one sweep on the object's operator in the object's panels; the multigrid cycle smooths with one per level.  What does
// not depend on the group is filled in by plan_call, the geometry by plan_group.
struct Sweep {
    rails_csr *A;
    int64_t n;
    const double *gvec; // G: the inverse of a diagonal, or the scalar gs = +-1 where this is null
    double gs;
    rails_panel *r, *z[2], *d, *q; // z[0] holds the result; z[1] is the other panel of the fused step's ping-pong, q holds A z unfused
    bool fused = false, ghost = false; // ghost: the fused step in its ghost-row form, with an exchange of the object's own before it
    double theta = 1.0, a[RAILS_CHEB_MAX_DEGREE], b[RAILS_CHEB_MAX_DEGREE];
    PassGeom g;
    int64_t slabs = 0;
    int at = 0; // the z panel that holds z now
    // the block form of G (the block multigrid cycle): the inverses of the diagonal blocks of a block-CSR A, bs > 0 their size; the level
    // matrix's device arrays and the step the level takes (block_amg_choice.h), filled in by plan_call and plan_group
    const double *ginv = nullptr;
    int bs = 0;
    int64_t mb = 0, max_brow = 0;
    const int64_t *browptr = nullptr;
    const int32_t *bcol = nullptr;
    const double *bval = nullptr;
    BamgStep step{};
};

struct Run {
    rails_ctx *c;
    rails_iter *it;
    int trans;
    PassGeom g;
    int64_t nslab;
    rails_iter_col *cols;
    bool jac; // a preconditioner applied inside the passes: the Jacobi diagonal, or (bj) the diagonal blocks
    int bj = 0; // block Jacobi in effect: the block size (the passes that apply G take their block form, on the block geometry)
    double tol2;
    // the preconditioner beyond Jacobi: the polynomial's degree (0: off) or the multigrid cycle (K is 0 then); sw[0] is the polynomial's
    // sweep, or sw[l] the smoother of level l; the last level's passes run on gc
    int K = 0;
    bool amg = false, other = false; // other: K > 0 or amg
    bool cycle = false;              // inside a cycle: the cycle's counters count too
    Sweep sw[RAILS_AMG_MAX_LEVELS]; // (about 1 KB each, 17 KB on the stack of a call: one struct for the polynomial, degree up to 64, and the levels, up to 8)
    PassGeom gc;
    int64_t slabs_c = 0;

    double *d(int k) const { return it->w[k]->d; }
    // every kernel of the object is launched, and counted, here
    template <class Kern, class... Args>
    void launch(Kern kernel, int64_t blocks, int threads, Args... args)
    {
        RAILS_LAUNCH(kernel, dim3((unsigned)blocks), dim3((unsigned)threads), 0, c->stream, args...);
        it->last_launches++;
        if (cycle) it->last_cycle_launches++;
    }
    void count_product()
    {
        it->last_products++;
        if (cycle) it->last_cycle_products++;
    }
    // a pass on the geometry pg, one block per slab
    template <class Kern, class... Args>
    void pass(const PassGeom &pg, int64_t slabs, Kern kernel, Args... args)
    {
        launch(kernel, slabs, 256, pg, args...);
    }
    // a pass of the group that writes partial sums: they go to the context workspace, the kernel's last argument
    template <class Kern, class... Args>
    int pass_sums(Kern kernel, Args... args)
    {
        RAILS_TRY(rails_ws_reserve(c, (size_t)nslab * 2 * g.ncw * sizeof(double)));
        pass(g, nslab, kernel, args..., c->ws);
        return RAILS_OK;
    }
    // a kernel on the shared row gather in its 8-lane form up to 16 columns, in its 16-lane form above
    template <class Kern>
    Kern lanes(Kern k8, Kern k16) const
    {
        return g.ncw <= 16 ? k8 : k16;
    }
    // such a kernel over a sweep's matrix: 64 rows per block, the blocks dealt over the 8 XCDs.  `rest` is what follows the gather's own
    // arguments.  One product.
    template <class Kern, class... Rest>
    void gather(Kern kernel, const Sweep &s, const double *zin, Rest... rest)
    {
        const int64_t bpx = ((s.n + 63) / 64 + 7) / 8;
        launch(kernel, bpx * 8, 256, s.n, s.A->rowptr, s.A->col, s.A->val, zin, g.ld, g.ncw, bpx, rest...);
        count_product();
    }
    int scalars(int step, int nq)
    {
        // (with the polynomial r.z carries the sign of the operator itself, as with Jacobi)
        const double sign = (jac || other) ? 1.0 : it->defsign;
        if (!it->reduces) {
            launch(k_iter_scalars, 1, 1024, step, c->ws, nslab, g.ncw, nq, cols, it->status_dev, tol2, it->maxit, sign);
            return RAILS_OK;
        }
        launch(k_iter_reduce, 1, 1024, c->ws, nslab, nq * g.ncw, it->sums_dev);
        RAILS_TRY(rails_allreduce_dev(c, it->sums_dev, (size_t)(nq * g.ncw)));
        it->last_allreduces++;
        launch(k_iter_compute, 1, 64, step, it->sums_dev, g.ncw, nq, cols, it->status_dev, tol2, it->maxit, sign);
        return RAILS_OK;
    }
    int product(rails_csr *A, int tr, rails_panel *from, rails_panel *to)
    {
        count_product();
        return rails_spmm(c, A, tr, from, 0, g.ncw, to, 0);
    }
    int product(int from, int to) { return product(it->A, it->method == RAILS_ITER_CG ? 0 : trans, it->w[from], it->w[to]); } // CG: a symmetric operator
    int dots(int np, int a1, int b1, int a2, int b2)
    {
        it->last_dots += np * g.ncw;
        return pass_sums(np == 1 ? k_iter_dots<1> : k_iter_dots<2>, d(a1), d(b1), d(a2), d(b2));
    }

    // ---- the sweep.  The fused steps read one z panel and write the other, and start in the one that makes the last of them write z[0]
    // (rails_cheb_start_panel); the unfused ones work in z[0] with A z in q.
    void sweep_start(Sweep &s, int steps)
    {
        s.at = rails_cheb_start_panel(s.fused, steps);
        if (s.bs)
            pass(s.g, s.slabs, bj_cheb_init(s.bs, false), s.ginv, s.theta, (const double *)s.r->d, s.d->d, s.z[s.at]->d);
        else
            pass(s.g, s.slabs, k_cheb_init, s.gvec, s.gs, s.theta, s.r->d, s.d->d, s.z[s.at]->d);
    }
    // a kernel on the shared block-row body over a block sweep's matrix, launched as k_spmm_bsr is for the group's width.  One product.
    int block_step(Sweep &s, const double *zin, double a, double b, double *zout)
    {
        const BsrChoice &k = s.step.k;
#define RAILS_BAMG_CASE(B, LPR)                                                                                                                   \
    case rails_bsr_inst(B, LPR):                                                                                                                  \
        launch((k_cheb_step_bsr<B, LPR>), k.grid, k.threads, s.mb, s.browptr, s.bcol, s.bval, zin, g.ld, g.ncw, k.rpg, k.bpx, s.ginv, a, b, (const double *)s.r->d, s.d->d, \
               zout);                                                                                                                             \
        break;
        switch (k.key()) {
            RAILS_BSR_TABLE(RAILS_BAMG_CASE)
        default: rails_set_error("rails_iter: k_cheb_step_bsr<%d, %d> is not among the instantiations of bsr_choice.h", k.b, k.lpr); return RAILS_EINVAL;
        }
#undef RAILS_BAMG_CASE
        count_product();
        return RAILS_OK;
    }
    int block_residual(Sweep &s, const double *z)
    {
        const BsrChoice &k = s.step.k;
#define RAILS_BAMG_CASE(B, LPR)                                                                                                                   \
    case rails_bsr_inst(B, LPR):                                                                                                                  \
        launch((k_amg_residual_bsr<B, LPR>), k.grid, k.threads, s.mb, s.browptr, s.bcol, s.bval, z, g.ld, g.ncw, k.rpg, k.bpx, (const double *)s.r->d, s.q->d);        \
        break;
        switch (k.key()) {
            RAILS_BSR_TABLE(RAILS_BAMG_CASE)
        default: rails_set_error("rails_iter: k_amg_residual_bsr<%d, %d> is not among the instantiations of bsr_choice.h", k.b, k.lpr); return RAILS_EINVAL;
        }
#undef RAILS_BAMG_CASE
        count_product();
        return RAILS_OK;
    }
    int sweep_step(Sweep &s, double a, double b)
    {
        rails_panel *zin = s.z[s.at];
        if (!s.fused) {
            RAILS_TRY(product(s.A, 0, zin, s.q));
            if (s.bs)
                pass(s.g, s.slabs, bj_cheb_pass(s.bs, false), s.ginv, a, b, (const double *)s.q->d, (const double *)s.r->d, s.d->d, zin->d);
            else
                pass(s.g, s.slabs, k_cheb_pass, s.gvec, s.gs, a, b, s.q->d, s.r->d, s.d->d, zin->d);
            return RAILS_OK;
        }
        if (s.bs) {
            s.at ^= 1;
            RAILS_TRY(block_step(s, zin->d, a, b, s.z[s.at]->d));
            it->last_fused++;
            return RAILS_OK;
        }
        int nce = 0;
        if (s.ghost) {
            // one exchange per step, as the unfused step's rails_spmm makes one: ranks that choose differently stay in step.  An even
            // number of columns, so that ghost rows are as aligned as panel rows: at an odd width the panel's column ncw travels too.
            // That is the pad column (zeroed at allocation, never written) when the group is as wide as the panels, and a column a
            // wider group has used otherwise; on the receiving side nobody reads it, since the lane of an odd last column takes its
            // one-entry path -- what it holds reaches no result, as with the pair loads of every pass (section 14's last test)
            nce = (g.ncw + 1) & ~1;
            RAILS_TRY(rails_halo_exchange(c, s.A, zin->d, g.ld, nce));
            it->last_halo++;
        }
        s.at ^= 1;
        gather(s.ghost ? lanes(k_cheb_step_csr<2, 8, true>, k_cheb_step_csr<4, 16, true>) : lanes(k_cheb_step_csr<2, 8, false>, k_cheb_step_csr<4, 16, false>), s, zin->d, s.gvec,
               s.gs, a, b, (const double *)s.r->d, s.d->d, s.z[s.at]->d, (const double *)(s.ghost ? s.A->ext : nullptr), nce);
        it->last_fused++;
        return RAILS_OK;
    }
    // W_Z = p_K(G A) G W_R (K = 0: G W_R)
    int polynomial()
    {
        it->last_poly++;
        sweep_start(sw[0], K);
        for (int k = 0; k < K; ++k) RAILS_TRY(sweep_step(sw[0], sw[0].a[k], sw[0].b[k]));
        return RAILS_OK;
    }
    // ---- the multigrid V-cycle: W_Z = M W_R.  Down: smooth from zero, residual, restrict; the dense inverse at
    // the bottom; up: prolong and correct, smooth from z.  Nothing in here synchronises, allocates, reads back or refuses: the
    // coefficients, the choice of the fused step and the geometry of every level are the plan of the call.
    int vcycle()
    {
        Amg &H = *it->hier;
        const int nl = (int)H.lv.size(), S = it->amg_degree;
        it->last_cycles++;
        for (int l = 0; l < nl; ++l) {
            Sweep &s = sw[l];
            sweep_start(s, 2 * S + 1); // S steps here, 1 + S on the way up
            for (int k = 0; k < S; ++k) RAILS_TRY(sweep_step(s, s.a[k], s.b[k]));
            rails_panel *z = s.z[s.at];
            if (s.fused && s.bs) {
                RAILS_TRY(block_residual(s, z->d));
            } else if (s.fused) {
                gather(lanes(k_amg_residual_csr<2, 8>, k_amg_residual_csr<4, 16>), s, z->d, (const double *)s.r->d, s.q->d);
            } else {
                RAILS_TRY(product(s.A, 0, z, s.q));
                pass(s.g, s.slabs, k_amg_residual_pass, s.r->d, s.q->d);
            }
            RAILS_TRY(product(H.lv[(size_t)l].R, 0, s.q, l + 1 < nl ? sw[l + 1].r : H.rc)); // r_{l+1} = P' q
        }
        pass(gc, slabs_c, k_amg_coarse_dense, H.Ainv, nl ? H.rc->d : d(W_R), nl ? H.zc->d : d(W_Z));
        for (int l = nl - 1; l >= 0; --l) {
            Sweep &s = sw[l];
            const rails_csr *P = H.lv[(size_t)l].P;
            pass(s.g, s.slabs, k_amg_prolong_add, P->rowptr, P->col, P->val, l + 1 < nl ? sw[l + 1].z[0]->d : H.zc->d, s.z[s.at]->d);
            count_product();
            // the post-smoother from z, the adjoint of the pre-smoother: one step with (a, b) = (0, 1 / theta) -- d is finite, k_cheb_init wrote
            // it whatever S is -- then S steps with the recurrence's coefficients.  It ends in z[0], where the level above looks for it.
            RAILS_TRY(sweep_step(s, 0.0, 1.0 / s.theta));
            for (int k = 0; k < S; ++k) RAILS_TRY(sweep_step(s, s.a[k], s.b[k]));
        }
        return RAILS_OK;
    }
    int precondition()
    {
        if (bj) { // (neither the polynomial nor the cycle is on: rails_iter_set)
            it->last_poly++;
            pass(g, nslab, bj_apply(bj, false), (const double *)it->bj_dev, (const double *)d(W_R), d(W_Z));
            return RAILS_OK;
        }
        cycle = amg; // (off again however the cycle ends)
        const int rc = amg ? vcycle() : polynomial();
        cycle = false;
        return rc;
    }
    int start()
    {
        if (it->method != RAILS_ITER_CG) {
            RAILS_TRY(pass_sums(k_bi_init, d(W_R), d(W_RH), d(W_P), d(W_Q), d(W_X)));
            it->last_dots += 2 * g.ncw;
            return scalars(STEP_BI_INIT, 2);
        }
        if (other) {
            RAILS_TRY(precondition());
            RAILS_TRY(pass_sums(k_cg_init_poly, d(W_R), d(W_Z), d(W_P), d(W_X)));
        } else if (bj)
            RAILS_TRY(pass_sums(bj_cg_init(bj, false), (const double *)it->bj_dev, (const double *)d(W_R), d(W_Z), d(W_P), d(W_X)));
        else
            RAILS_TRY(pass_sums(jac ? k_cg_init<true> : k_cg_init<false>, it->dinv, d(W_R), jac ? d(W_Z) : nullptr, d(W_P), d(W_X)));
        it->last_dots += 2 * g.ncw;
        return scalars(STEP_CG_INIT, 2);
    }
    int iteration()
    {
        if (it->method == RAILS_ITER_CG) {
            RAILS_TRY(product(W_P, W_Q));
            RAILS_TRY(dots(1, W_P, W_Q, W_P, W_Q));
            RAILS_TRY(scalars(STEP_CG_ALPHA, 1));
            if (other) {
                // the update without its own z (its partial sums are overwritten below), the polynomial, then r.z and r.r in the layout
                // the scalar step reads; K products in a row without an inner product, a scalar kernel or a read-back between them
                RAILS_TRY(pass_sums(k_cg_update<false>, cols, it->dinv, d(W_P), d(W_Q), d(W_X), d(W_R), nullptr));
                RAILS_TRY(precondition());
                RAILS_TRY(dots(2, W_R, W_Z, W_R, W_R));
            } else {
                if (bj)
                    RAILS_TRY(pass_sums(bj_cg_update(bj, false), (const rails_iter_col *)cols, (const double *)it->bj_dev, (const double *)d(W_P), (const double *)d(W_Q), d(W_X),
                                        d(W_R), d(W_Z)));
                else
                    RAILS_TRY(pass_sums(jac ? k_cg_update<true> : k_cg_update<false>, cols, it->dinv, d(W_P), d(W_Q), d(W_X), d(W_R), jac ? d(W_Z) : nullptr));
                it->last_dots += 2 * g.ncw;
            }
            RAILS_TRY(scalars(STEP_CG_BETA, 2));
            pass(g, nslab, k_cg_dir, cols, d(other || jac ? W_Z : W_R), d(W_P));
            return RAILS_OK;
        }
        const int ph = jac ? W_Z : W_P, sh = jac ? W_SH : W_R;
        if (bj)
            pass(g, nslab, bj_bi_dir(bj, trans != 0), (const rails_iter_col *)cols, (const double *)it->bj_dev, (const double *)d(W_R), (const double *)d(W_Q), d(W_P), d(W_Z));
        else
            pass(g, nslab, jac ? k_bi_dir<true> : k_bi_dir<false>, cols, it->dinv, d(W_R), d(W_Q), d(W_P), jac ? d(W_Z) : nullptr);
        RAILS_TRY(product(ph, W_Q)); // v = A p^
        RAILS_TRY(dots(1, W_RH, W_Q, W_RH, W_Q));
        RAILS_TRY(scalars(STEP_BI_ALPHA, 1));
        if (bj)
            pass(g, nslab, bj_bi_s(bj, trans != 0), (const rails_iter_col *)cols, (const double *)it->bj_dev, (const double *)d(W_Q), d(W_R), d(W_SH));
        else
            pass(g, nslab, jac ? k_bi_s<true> : k_bi_s<false>, cols, it->dinv, d(W_Q), d(W_R), jac ? d(W_SH) : nullptr);
        RAILS_TRY(product(sh, W_T)); // t = A s^
        RAILS_TRY(dots(2, W_T, W_R, W_T, W_T));
        RAILS_TRY(scalars(STEP_BI_OMEGA, 2));
        RAILS_TRY(pass_sums(k_bi_update, cols, d(ph), d(sh), d(W_T), d(W_RH), d(W_X), d(W_R)));
        it->last_dots += 2 * g.ncw;
        return scalars(STEP_BI_END, 2);
    }
};

// the upper end of the polynomial's interval: "eig_max", else the Gershgorin bound that goes with the preconditioner in effect (0: none)
double poly_hi(const rails_iter *it)
{
    if (it->eig_max > 0.0) return it->eig_max;
    return (it->jacobi && it->dinv) ? it->hi_jacobi : it->hi_plain;
}

// The plan of a call, made before anything is queued: the sweeps (operator, panels, interval, coefficients, whether the steps run on the
// fused kernel) of the polynomial or of every multigrid level.  Every refusal of a preconditioner is here.  The work panels and the
// hierarchy must be there (the fused kernel's rule looks at the panels' row stride).
int plan_call(Run &run, const char *who)
{
    rails_iter *it = run.it;
    rails_csr *A = it->A;
    const int ld = it->w[W_R]->ld;
    run.K = it->poly_degree;
    run.amg = it->amg != 0 || it->block_amg != 0; // (either cycle: Run::vcycle on the sweeps made here)
    run.other = run.K > 0 || run.amg;
    run.sw[0] = Sweep{A, it->m, run.jac ? it->dinv : nullptr, it->defsign, it->w[W_R], {it->w[W_Z], it->w[W_Z2]}, it->w[W_D], it->w[W_Q]};
    if (run.amg) {
        const Amg &H = *it->hier;
        for (size_t l = 0; l < H.lv.size(); ++l) {
            const AmgLevel &L = H.lv[l];
            Sweep &s = run.sw[l];
            if (l > 0) s = Sweep{L.A, L.n, L.dinv, 1.0, L.w[L_R], {L.w[L_Z], L.w[L_Z2]}, L.w[L_D], L.w[L_Q]};
            s.gvec = L.dinv; // (level 0: the object's operator in the object's panels, with the hierarchy's diagonal)
            s.gs = 1.0;
            RAILS_REQUIRE(rails_cheb_coef(L.hi / it->amg_ratio, L.hi, it->amg_degree, &s.theta, s.a, s.b), "rails_iter: no smoother of degree %d on [%g, %g] (level %d)",
                          it->amg_degree, L.hi / it->amg_ratio, L.hi, (int)l);
            if (H.b) { // the block hierarchy: G is the level's inverse diagonal blocks; whether the step is fused depends on the group (plan_group)
                s.gvec = nullptr;
                s.ginv = L.ginv;
                s.bs = H.b;
                RAILS_REQUIRE(rails_bsr_device_arrays(L.A, &s.mb, &s.max_brow, &s.browptr, &s.bcol, &s.bval), "%s: level %d of the block hierarchy is not a block-CSR handle", who, (int)l);
                RAILS_REQUIRE(bj_cheb_init(s.bs, false), "%s: no block kernels for block size %d (RAILS_BJ_TABLE)", who, s.bs);
                s.fused = false;
            } else
                s.fused = it->poly_fused && rails_cheb_fused_eligible(true, 0, L.n, ld);
        }
        return RAILS_OK;
    }
    if (run.K == 0) return RAILS_OK;
    Sweep &s = run.sw[0];
    const double hi = poly_hi(it);
    RAILS_REQUIRE((hi > 0.0 && rails_iter_finite(hi)) || run.it->A->kind != rails_csr::BSR,
                  "%s: poly_degree %d needs an upper bound on the spectrum: a block-CSR operator keeps no scalar CSR arrays to take one from, set \"eig_max\"", who, run.K);
    RAILS_REQUIRE(hi > 0.0 && rails_iter_finite(hi),
                  "%s: poly_degree %d needs an upper bound on the spectrum: the operator keeps no CSR arrays on the host to take one from, set \"eig_max\"", who, run.K);
    RAILS_REQUIRE(rails_cheb_coef(hi / it->poly_ratio, hi, run.K, &s.theta, s.a, s.b), "%s: no polynomial of degree %d on [%g, %g]", who, run.K, hi / it->poly_ratio, hi);
    const bool stored = A->kind == rails_csr::STORED && !A->rect && A->rowptr && A->col && A->val;
    // an operator that exchanges (rows to send or ghost rows to receive: rails_spmm's own condition, so that a step issues an exchange in
    // the fused form exactly when it does in the unfused one -- a rank that only sends, or only receives, takes part; a rank whose plan is
    // empty issues none in either form) takes the ghost-row form; its ghost buffer's row stride is the group's width rounded up to even,
    // at most RAILS_ITER_GROUP
    s.ghost = A->n_ghost > 0 || A->n_send > 0;
    if (s.ghost)
        s.fused = it->poly_fused && rails_cheb_fused_ghost_eligible(stored, it->m, A->n_ghost, ld, RAILS_ITER_GROUP);
    else
        s.fused = it->poly_fused && rails_cheb_fused_eligible(stored, A->n_ghost, it->m, ld);
    return RAILS_OK;
}

// what of the plan depends on the width w of a group: the geometry of its passes (iter_geom.h), every sweep's and the last level's
void plan_group(Run &run, int w)
{
    const rails_iter *it = run.it;
    const int ld = it->w[W_R]->ld;
    const int nl = run.amg ? (int)it->hier->lv.size() : 0;
    const int hb = run.amg ? it->hier->b : 0; // the block hierarchy: every pass of every level on slabs of whole block rows
    for (int l = 0; l < std::max(1, nl); ++l) {
        Sweep &s = run.sw[l];
        s.g = hb ? rails_iter_pass_geom_block(s.n, w, ld, hb, &s.slabs) : rails_iter_pass_geom(s.n, w, ld, &s.slabs);
        if (hb && nl) {
            BsrFacts f;
            f.b = hb; f.nc = w; f.mb = s.mb; f.max_brow = s.max_brow; f.num_cu = run.c->num_cu;
            f.ldx = f.ldy = ld;
            f.y_vec2 = ld % 2 == 0;
            s.step = rails_bamg_step(f, it->poly_fused != 0);
            s.fused = s.step.ok && s.step.fused;
        }
    }
    run.g = run.sw[0].g; // (level 0 has the operator's rows)
    run.nslab = run.sw[0].slabs;
    if (run.bj) run.g = rails_iter_pass_geom_block(it->m, w, ld, run.bj, &run.nslab); // every pass of the group, the point ones too
    if (run.amg) run.gc = hb ? rails_iter_pass_geom_block(it->hier->n_coarse, w, ld, hb, &run.slabs_c) : rails_iter_pass_geom(it->hier->n_coarse, w, ld, &run.slabs_c);
}

} // namespace

extern "C" void rails_iter_destroy(rails_iter *it)
{
    if (!it) return;
    if (it->ctx) {
        hipSetDevice(it->ctx->device);
        hipStreamSynchronize(it->ctx->stream);
    }
    amg_release(it);
    release_work(it);
    hipFree(it->dinv);
    hipFree(it->bj_dev);
    hipFree(it->cols_dev);
    hipFree(it->status_dev);
    hipFree(it->sums_dev);
    if (it->pinned) hipHostFree(it->pinned);
    delete it;
}

namespace {

// The gather of iter_agree.h: this rank's slot of a zeroed vector of nranks slots, one sum all-reduce, the whole vector back on the host.
int gather_slots(rails_ctx *c, const double *mine, std::vector<double> &all)
{
    const int nr = std::max(1, c->nranks), n = nr * RAILS_AGREE_SLOT;
    RAILS_REQUIRE(c->rank >= 0 && c->rank < nr, "rails_iter_create: rank %d of %d", c->rank, nr);
    all.assign((size_t)n, 0.0);
    std::copy(mine, mine + RAILS_AGREE_SLOT, all.begin() + (size_t)c->rank * RAILS_AGREE_SLOT);
    double *dev = nullptr;
    RAILS_HIP_CHECK(hipMalloc((void **)&dev, (size_t)n * sizeof(double)));
    int rc = RAILS_OK;
    hipError_t e = hipMemcpyAsync(dev, all.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream); // (the source is pageable host memory)
    if (e == hipSuccess) rc = rails_allreduce_dev(c, dev, (size_t)n);
    if (e == hipSuccess && rc == RAILS_OK) e = hipMemcpyAsync(all.data(), dev, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && rc == RAILS_OK) e = rails_stream_sync(c);
    hipFree(dev);
    if (rc != RAILS_OK) return rc;
    RAILS_HIP_CHECK(e);
    return RAILS_OK;
}

} // namespace

// On a context that reduces, create is a collective call (one all-reduce).  Refusals that every rank reaches alike -- the method, the
// context, a partition without a hook or communicator -- come before it; what only this rank can see (its block's shape, a zero in the
// diagonal it was given) travels through it, so that every rank refuses and none is left waiting.
extern "C" int rails_iter_create(rails_ctx *c, rails_csr *A, int method, const double *diag_host, rails_iter **out)
{
    if (c) hipSetDevice(c->device);
    RAILS_REQUIRE(c && A && out, "rails_iter_create: null argument");
    RAILS_REQUIRE(method == RAILS_ITER_CG || method == RAILS_ITER_BICGSTAB, "rails_iter_create: method %d is neither RAILS_ITER_CG nor RAILS_ITER_BICGSTAB", method);
    RAILS_REQUIRE(c == A->ctx, "rails_iter_create: the operator belongs to another context");
    RAILS_REQUIRE(c->nranks <= 1 || c->allreduce || c->rccl,
                  "rails_iter_create: the context is row-partitioned but has neither an all-reduce hook nor a communicator: without one this object is single GPU only");
    const bool reduces = c->nranks > 1 || c->allreduce || c->rccl; // rails_allreduce_dev's own condition
    const int64_t m = A->m;
    // square: globally, for a stored row block whose halo plan is set (rails_csr_set_halo: m + n_ghost == ncols_ext)
    const bool ghosted = reduces && A->kind == rails_csr::STORED && !A->rect && A->ncols_ext > m && A->n_ghost == A->ncols_ext - m;
    char refusal[192] = "";
    if (A->rect || A->kind == rails_csr::SPRHS || (A->ncols_ext != m && !ghosted))
        snprintf(refusal, sizeof refusal, "rails_iter_create: the operator is rectangular (%lld x %lld)", (long long)m, (long long)rails_csr_cols(A));
    else if (m < 1)
        snprintf(refusal, sizeof refusal, "rails_iter_create: an operator without rows");
    const bool host_csr = !refusal[0] && A->kind == rails_csr::STORED && (int64_t)A->h_rowptr.size() == m + 1 && (int64_t)A->h_val.size() == A->h_rowptr[m];
    std::vector<double> dinv;
    if (refusal[0]) {
    } else if (diag_host) {
        dinv.assign(diag_host, diag_host + m);
        for (int64_t i = 0; i < m && !refusal[0]; ++i)
            if (!(dinv[i] != 0.0 && rails_iter_finite(dinv[i]))) snprintf(refusal, sizeof refusal, "rails_iter_create: diagonal entry %lld is %g", (long long)i, dinv[i]);
    } else if (host_csr) {
        // the CSR diagonal, when every entry of it is stored and nonzero; otherwise no preconditioner
        dinv.assign((size_t)m, 0.0);
        bool ok = true;
        for (int64_t i = 0; i < m && ok; ++i) {
            bool found = false;
            for (int64_t q = A->h_rowptr[i]; q < A->h_rowptr[i + 1]; ++q)
                if (A->h_col[q] == i) {
                    dinv[i] += A->h_val[q];
                    found = true;
                }
            ok = found && dinv[i] != 0.0 && rails_iter_finite(dinv[i]);
        }
        if (!ok) dinv.clear();
    }
    if (refusal[0] && !reduces) {
        rails_set_error("%s", refusal);
        return RAILS_EINVAL;
    }
    if (refusal[0]) dinv.clear();
    bool negative = !dinv.empty();
    for (double &v : dinv) {
        negative = negative && v < 0.0;
        v = 1.0 / v;
    }
    double defsign = negative ? -1.0 : 1.0, hi_plain = 0.0, hi_jacobi = 0.0;
    if (host_csr) {
        // the polynomial preconditioner's upper bounds (two numbers; used only with "poly_degree" above 0).  A row block's rows hold their
        // ghost columns' entries: the local row sums are complete
        hi_plain = rails_cheb_gershgorin(m, A->h_rowptr.data(), A->h_val.data(), nullptr);
        if (!dinv.empty()) hi_jacobi = rails_cheb_gershgorin(m, A->h_rowptr.data(), A->h_val.data(), dinv.data());
    }
    if (reduces) {
        double mine[RAILS_AGREE_SLOT];
        rails_iter_agree_fill(mine, refusal[0] ? RAILS_AGREE_REFUSED : dinv.empty() ? RAILS_AGREE_NO_DIAG : RAILS_AGREE_DIAG, negative, hi_plain, hi_jacobi);
        std::vector<double> all;
        RAILS_TRY(gather_slots(c, mine, all));
        const rails_iter_agreed ag = rails_iter_agree(all.data(), std::max(1, c->nranks));
        if (ag.refused) {
            rails_set_error("%s", refusal[0] ? refusal : "rails_iter_create: another rank refused its arguments");
            return RAILS_EINVAL;
        }
        if (!ag.jacobi) dinv.clear();
        defsign = ag.defsign;
        hi_plain = ag.hi_plain;
        hi_jacobi = ag.hi_jacobi;
    }
    rails_iter *it = new rails_iter;
    it->ctx = c;
    it->A = A;
    it->method = method;
    it->m = m;
    it->reduces = reduces;
    it->defsign = defsign;
    it->hi_plain = hi_plain;
    it->hi_jacobi = hi_jacobi;
    hipError_t e = hipMalloc((void **)&it->status_dev, 16 * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemset(it->status_dev, 0, 16 * sizeof(int32_t));
    if (e == hipSuccess && !dinv.empty()) {
        e = hipMalloc((void **)&it->dinv, (size_t)m * sizeof(double));
        if (e == hipSuccess) e = hipMemcpy(it->dinv, dinv.data(), (size_t)m * sizeof(double), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess && reduces) {
        e = hipMalloc((void **)&it->sums_dev, 64 * sizeof(double));
        if (e == hipSuccess) e = hipMemset(it->sums_dev, 0, 64 * sizeof(double));
    }
    if (e != hipSuccess) {
        rails_set_error("rails_iter_create: device allocation or upload failed: %s", hipGetErrorString(e));
        rails_iter_destroy(it);
        return RAILS_EHIP;
    }
    *out = it;
    return RAILS_OK;
}

extern "C" int rails_iter_set(rails_iter *it, const char *name, double value)
{
    RAILS_REQUIRE(it && name, "rails_iter_set: null argument");
    RAILS_REQUIRE(rails_iter_finite(value), "rails_iter_set: %s = %g", name, value);
    const std::string n(name);
    if (n == "tolerance") {
        RAILS_REQUIRE(value >= 0.0, "rails_iter_set: tolerance %g", value);
        it->tol = value;
    } else if (n == "max_iterations") {
        RAILS_REQUIRE(value >= 0.0 && value <= 1e9, "rails_iter_set: max_iterations %g", value);
        it->maxit = (int)value;
    } else if (n == "jacobi")
        it->jacobi = value != 0.0;
    else if (n == "check_every") {
        RAILS_REQUIRE(value >= 1.0 && value <= 1e9, "rails_iter_set: check_every %g", value);
        it->check_every = (int)value;
    } else if (n == "strict")
        it->strict = value != 0.0;
    else if (n == "poly_degree") {
        RAILS_REQUIRE(value >= 0.0 && value <= RAILS_CHEB_MAX_DEGREE && value == std::floor(value), "rails_iter_set: poly_degree %g is not a whole number in 0 .. %d", value,
                      RAILS_CHEB_MAX_DEGREE);
        RAILS_REQUIRE(value == 0.0 || !it->amg, "rails_iter_set: poly_degree %g together with \"amg\": one preconditioner at a time", value);
        RAILS_REQUIRE(value == 0.0 || !it->block_jacobi, "rails_iter_set: poly_degree %g together with \"block_jacobi\": one preconditioner at a time", value);
        RAILS_REQUIRE(value == 0.0 || !it->block_amg, "rails_iter_set: poly_degree %g together with \"block_amg\": one preconditioner at a time", value);
        RAILS_REQUIRE(value == 0.0 || it->method == RAILS_ITER_CG,
                      "rails_iter_set: poly_degree %g on a BiCGStab object: the polynomial preconditioner is for conjugate gradients (a real spectrum)", value);
        it->poly_degree = (int)value;
    } else if (n == "poly_ratio") {
        RAILS_REQUIRE(value > 1.0, "rails_iter_set: poly_ratio %g is not above 1", value);
        it->poly_ratio = value;
    } else if (n == "eig_max") {
        RAILS_REQUIRE(value >= 0.0, "rails_iter_set: eig_max %g", value);
        it->eig_max = value;
    } else if (n == "poly_fused")
        it->poly_fused = value != 0.0;
    else if (n == "block_jacobi") {
        if (value != 0.0) {
            RAILS_REQUIRE(it->bj_dev, "rails_iter_set: \"block_jacobi\" 1 without blocks: install them first (rails_iter_block_jacobi)");
            RAILS_REQUIRE(it->poly_degree == 0, "rails_iter_set: \"block_jacobi\" together with poly_degree %d: one preconditioner at a time", it->poly_degree);
            RAILS_REQUIRE(!it->amg, "rails_iter_set: \"block_jacobi\" together with \"amg\": one preconditioner at a time");
            RAILS_REQUIRE(!it->block_amg, "rails_iter_set: \"block_jacobi\" together with \"block_amg\": one preconditioner at a time");
        }
        it->block_jacobi = value != 0.0;
    } else if (n == "amg") {
        if (value != 0.0) RAILS_TRY(amg_check(it, "rails_iter_set"));
        it->amg = value != 0.0;
    } else if (n == "block_amg") {
        if (value != 0.0) RAILS_TRY(bamg_check(it, "rails_iter_set"));
        it->block_amg = value != 0.0;
    } else if (n == "amg_degree") {
        RAILS_REQUIRE(value >= 0.0 && value <= 8.0 && value == std::floor(value), "rails_iter_set: amg_degree %g is not a whole number in 0 .. 8", value);
        it->amg_degree = (int)value;
    } else if (n == "amg_ratio") {
        RAILS_REQUIRE(value > 1.0, "rails_iter_set: amg_ratio %g is not above 1", value);
        it->amg_ratio = value;
    } else if (n == "amg_theta") {
        RAILS_REQUIRE(value >= 0.0 && value < 1.0, "rails_iter_set: amg_theta %g is not in [0, 1)", value);
        if (value != it->amg_theta) amg_release(it);
        it->amg_theta = value;
    } else if (n == "amg_coarse") {
        RAILS_REQUIRE(value >= 1.0 && value <= RAILS_AMG_MAX_COARSE && value == std::floor(value), "rails_iter_set: amg_coarse %g is not a whole number in 1 .. %d", value,
                      RAILS_AMG_MAX_COARSE);
        if ((int)value != it->amg_coarse) amg_release(it);
        it->amg_coarse = (int)value;
    } else {
        rails_set_error("rails_iter_set: no setting named '%s' (tolerance, max_iterations, jacobi, check_every, strict, poly_degree, poly_ratio, eig_max, poly_fused, amg, amg_degree, "
                        "amg_ratio, amg_theta, amg_coarse, block_jacobi, block_amg)", name);
        return RAILS_EINVAL;
    }
    return RAILS_OK;
}

// Installs (or clears) the block-Jacobi preconditioner: where the diagonal blocks come from and every refusal is rails_bj_plan
// (block_jacobi_host.h), the extraction and the long-double inverses are host code there too; nothing touches the device before the
// inverses stand.  Installing sets "block_jacobi" to 1.
extern "C" int rails_iter_block_jacobi(rails_ctx *c, rails_iter *it, int b, const double *blocks_host)
{
    if (c) hipSetDevice(c->device);
    RAILS_REQUIRE(c && it, "rails_iter_block_jacobi: null argument");
    RAILS_REQUIRE(c == it->ctx, "rails_iter_block_jacobi: the object belongs to another context");
    const rails_csr *A = it->A;
    const int64_t m = it->m;
    int hb = 0;
    int64_t hmb = 0;
    const int64_t *browptr = nullptr;
    const int32_t *bcol = nullptr;
    const double *bval = nullptr;
    const bool host_csr = A->kind == rails_csr::STORED && (int64_t)A->h_rowptr.size() == m + 1 && (int64_t)A->h_val.size() == A->h_rowptr[m] && A->h_col.size() == A->h_val.size();
    int op = RAILS_BJ_OP_CALLBACK;
    switch (A->kind) {
    case rails_csr::STORED: op = host_csr ? RAILS_BJ_OP_CSR : RAILS_BJ_OP_CSR_NO_HOST; break;
    case rails_csr::BSR:
        RAILS_REQUIRE(rails_bsr_host_arrays(A, &hb, &hmb, &browptr, &bcol, &bval), "rails_iter_block_jacobi: the block-CSR operator keeps no host copy");
        op = RAILS_BJ_OP_BSR;
        break;
    case rails_csr::LU: op = RAILS_BJ_OP_LU; break;
    case rails_csr::ITER: op = RAILS_BJ_OP_ITER; break;
    default: op = RAILS_BJ_OP_CALLBACK; break;
    }
    const bool reduces = it->reduces || A->n_ghost > 0 || A->n_send > 0;
    int source = RAILS_BJ_CLEAR, be = 0;
    char err[256] = "";
    if (rails_bj_plan(op, hb, reduces, m, b, blocks_host != nullptr, &source, &be, err, sizeof err)) {
        rails_set_error("%s", err);
        return RAILS_EINVAL;
    }
    if (source == RAILS_BJ_CLEAR) {
        RAILS_HIP_CHECK(hipStreamSynchronize(c->stream));
        hipFree(it->bj_dev);
        it->bj_dev = nullptr;
        it->bj_host.clear();
        it->bj_b = it->block_jacobi = 0;
        return RAILS_OK;
    }
    RAILS_REQUIRE(it->poly_degree == 0, "rails_iter_block_jacobi: together with poly_degree %d: one preconditioner at a time", it->poly_degree);
    RAILS_REQUIRE(!it->amg, "rails_iter_block_jacobi: together with \"amg\": one preconditioner at a time");
    RAILS_REQUIRE(!it->block_amg, "rails_iter_block_jacobi: together with \"block_amg\": one preconditioner at a time");
    const int64_t nb = m / be;
    const size_t n = (size_t)nb * be * be;
    std::vector<double> blocks, inv(n);
    if (source != RAILS_BJ_FROM_ARGUMENT) {
        blocks.resize(n);
        if (source == RAILS_BJ_FROM_BSR)
            rails_bj_from_bsr(nb, be, browptr, bcol, bval, blocks.data());
        else
            rails_bj_from_csr(nb, be, A->h_rowptr.data(), A->h_col.data(), A->h_val.data(), blocks.data());
        blocks_host = blocks.data();
    }
    if (rails_bj_invert(nb, be, blocks_host, inv.data(), err, sizeof err)) {
        rails_set_error("%s", err);
        return RAILS_EINVAL;
    }
    double *dev = nullptr;
    RAILS_HIP_CHECK(hipStreamSynchronize(c->stream)); // (a solve still queued reads the old blocks)
    RAILS_HIP_CHECK(hipMalloc((void **)&dev, n * sizeof(double)));
    const hipError_t e = hipMemcpy(dev, inv.data(), n * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        hipFree(dev);
        RAILS_HIP_CHECK(e);
    }
    hipFree(it->bj_dev);
    it->bj_dev = dev;
    it->bj_host.swap(inv);
    it->bj_b = be;
    it->block_jacobi = 1;
    c->n_dev_alloc++;
    return RAILS_OK;
}

// the number of blocks (0: none installed) and their size; the first cap_blocks inverses exactly as uploaded
extern "C" int64_t rails_iter_block_jacobi_info(const rails_iter *it, int *b, double *inv_blocks_host, int64_t cap_blocks)
{
    RAILS_REQUIRE(it, "rails_iter_block_jacobi_info: null argument");
    const int64_t nb = it->bj_b ? it->m / it->bj_b : 0;
    if (b) *b = it->bj_b;
    if (inv_blocks_host && cap_blocks > 0 && nb > 0)
        std::copy(it->bj_host.begin(), it->bj_host.begin() + (size_t)std::min(nb, cap_blocks) * it->bj_b * it->bj_b, inv_blocks_host);
    return nb;
}

// Builds (or rebuilds) the multigrid hierarchy from the CSR arrays the operator's handle keeps on the host and uploads it: the level operators, P and R = P' as rectangular operators, the inverse diagonals, the dense inverse.
extern "C" int rails_iter_amg_setup(rails_ctx *c, rails_iter *it)
{
    if (c) hipSetDevice(c->device);
    RAILS_REQUIRE(c && it, "rails_iter_amg_setup: null argument");
    RAILS_REQUIRE(c == it->ctx, "rails_iter_amg_setup: the object belongs to another context");
    RAILS_TRY(amg_check(it, "rails_iter_amg_setup"));
    amg_release(it);
    rails_csr *A = it->A;
    const int64_t m = it->m;
    // the CSR arrays every stored handle keeps on the host (rails_csr_create); a handle without them would need a copy back from the device
    RAILS_REQUIRE((int64_t)A->h_rowptr.size() == m + 1 && (int64_t)A->h_val.size() == A->h_rowptr[m] && A->h_col.size() == A->h_val.size(),
                  "rails_iter_amg_setup: the operator keeps no CSR arrays on the host to build the hierarchy from");
    const int64_t *rowptr = A->h_rowptr.data();
    const int32_t *col = A->h_col.data();
    const double *val = A->h_val.data();
    const auto t0 = std::chrono::steady_clock::now();
    rails_amg_hierarchy h;
    RAILS_TRY(rails_amg_build_host(m, rowptr, col, val, it->amg_theta, it->amg_coarse, &h));
    const auto t1 = std::chrono::steady_clock::now();
    Amg *H = new Amg;
    it->hier = H; // (released by amg_release, also when an upload below fails)
    H->n_coarse = h.coarse.n_rows;
    H->coarse_nnz = h.coarse.nnz();
    H->lv.resize(h.levels.size());
    int rc = RAILS_OK;
    hipError_t e = hipSuccess;
    for (size_t l = 0; l < h.levels.size() && rc == RAILS_OK && e == hipSuccess; ++l) {
        const rails_amg_level &S = h.levels[l];
        AmgLevel &L = H->lv[l];
        L.n = S.A.n_rows;
        L.nnz = S.A.nnz();
        L.hi = S.hi;
        if (l == 0)
            L.A = A;
        else
            rc = rails_csr_create(c, L.n, L.n, S.A.rowptr.data(), S.A.col.data(), S.A.val.data(), &L.A);
        if (rc == RAILS_OK) rc = rails_csr_create_rect(c, S.P.n_rows, S.P.n_cols, S.P.rowptr.data(), S.P.col.data(), S.P.val.data(), &L.P);
        if (rc == RAILS_OK) rc = rails_csr_create_rect(c, S.R.n_rows, S.R.n_cols, S.R.rowptr.data(), S.R.col.data(), S.R.val.data(), &L.R);
        if (rc == RAILS_OK) e = hipMalloc((void **)&L.dinv, (size_t)L.n * sizeof(double));
        if (rc == RAILS_OK && e == hipSuccess) e = hipMemcpy(L.dinv, S.dinv.data(), (size_t)L.n * sizeof(double), hipMemcpyHostToDevice);
    }
    if (rc == RAILS_OK && e == hipSuccess) e = hipMalloc((void **)&H->Ainv, h.coarse_inv.size() * sizeof(double));
    if (rc == RAILS_OK && e == hipSuccess) e = hipMemcpy(H->Ainv, h.coarse_inv.data(), h.coarse_inv.size() * sizeof(double), hipMemcpyHostToDevice);
    if (rc != RAILS_OK || e != hipSuccess) {
        if (rc == RAILS_OK) rails_set_error("rails_iter_amg_setup: device allocation or upload failed: %s", hipGetErrorString(e));
        amg_release(it);
        return rc != RAILS_OK ? rc : RAILS_EHIP;
    }
    H->host_seconds = std::chrono::duration<double>(t1 - t0).count();
    H->upload_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
    return RAILS_OK;
}

namespace {
int hierarchy_info(const rails_iter *it, int block, int64_t *rows, int64_t *nnz, double *hi, int cap);
}

// Builds (or rebuilds) the block hierarchy from the block-CSR arrays the operator's handle keeps on the host (block_amg_host.h) and uploads
// it: the level operators as block-CSR handles, P and R = P' as rectangular operators, the inverse diagonal blocks, the dense inverse.
// Every refusal comes before any device work.
extern "C" int rails_iter_block_amg_setup(rails_ctx *c, rails_iter *it)
{
    if (c) hipSetDevice(c->device);
    RAILS_REQUIRE(c && it, "rails_iter_block_amg_setup: null argument");
    RAILS_REQUIRE(c == it->ctx, "rails_iter_block_amg_setup: the object belongs to another context");
    RAILS_TRY(bamg_check(it, "rails_iter_block_amg_setup"));
    rails_csr *A = it->A;
    int b = 0;
    int64_t mb = 0;
    const int64_t *browptr = nullptr;
    const int32_t *bcol = nullptr;
    const double *bval = nullptr;
    RAILS_REQUIRE(rails_bsr_host_arrays(A, &b, &mb, &browptr, &bcol, &bval), "rails_iter_block_amg_setup: the block-CSR operator keeps no host copy");
    const auto t0 = std::chrono::steady_clock::now();
    rails_bamg_hierarchy h;
    RAILS_TRY(rails_bamg_build_host(mb, b, browptr, bcol, bval, it->amg_theta, it->amg_coarse, &h));
    const auto t1 = std::chrono::steady_clock::now();
    amg_release(it); // (a refused rebuild leaves the hierarchy there was)
    Amg *H = new Amg;
    it->hier = H; // (released by amg_release, also when an upload below fails)
    H->b = b;
    H->n_coarse = h.coarse.mb * b;
    H->coarse_nnz = h.coarse.nnzb() * b * b;
    H->lv.resize(h.levels.size());
    int rc = RAILS_OK;
    hipError_t e = hipSuccess;
    for (size_t l = 0; l < h.levels.size() && rc == RAILS_OK && e == hipSuccess; ++l) {
        const rails_bamg_level &S = h.levels[l];
        AmgLevel &L = H->lv[l];
        L.n = S.A.mb * b;
        L.nnz = S.A.nnzb() * b * b;
        L.hi = S.hi;
        if (l == 0)
            L.A = A;
        else
            rc = rails_csr_create_bsr(c, S.A.mb, S.A.mb, b, S.A.browptr.data(), S.A.bcol.data(), S.A.bval.data(), &L.A);
        if (rc == RAILS_OK) rc = rails_csr_create_rect(c, S.P.n_rows, S.P.n_cols, S.P.rowptr.data(), S.P.col.data(), S.P.val.data(), &L.P);
        if (rc == RAILS_OK) rc = rails_csr_create_rect(c, S.R.n_rows, S.R.n_cols, S.R.rowptr.data(), S.R.col.data(), S.R.val.data(), &L.R);
        if (rc == RAILS_OK) e = hipMalloc((void **)&L.ginv, S.ginv.size() * sizeof(double));
        if (rc == RAILS_OK && e == hipSuccess) e = hipMemcpy(L.ginv, S.ginv.data(), S.ginv.size() * sizeof(double), hipMemcpyHostToDevice);
    }
    if (rc == RAILS_OK && e == hipSuccess) e = hipMalloc((void **)&H->Ainv, h.coarse_inv.size() * sizeof(double));
    if (rc == RAILS_OK && e == hipSuccess) e = hipMemcpy(H->Ainv, h.coarse_inv.data(), h.coarse_inv.size() * sizeof(double), hipMemcpyHostToDevice);
    if (rc == RAILS_OK && e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (rc != RAILS_OK || e != hipSuccess) {
        if (rc == RAILS_OK) rails_set_error("rails_iter_block_amg_setup: device allocation or upload failed: %s", hipGetErrorString(e));
        amg_release(it);
        return rc != RAILS_OK ? rc : RAILS_EHIP;
    }
    H->host_seconds = std::chrono::duration<double>(t1 - t0).count();
    H->upload_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
    return RAILS_OK;
}

// rails_iter_amg_info's conventions on the block hierarchy: rows, scalar entries (blocks times b^2) and the smoother's bound per matrix,
// then the two trailing entries.  0 when no block hierarchy has been built.
extern "C" int rails_iter_block_amg_info(const rails_iter *it, int64_t *rows, int64_t *nnz, double *hi, int cap)
{
    RAILS_REQUIRE(it && cap >= 0, "rails_iter_block_amg_info: bad argument");
    return hierarchy_info(it, 1, rows, nnz, hi, cap);
}

// The hierarchy by its matrices, the last (dense) one included: rows, entries and the Gershgorin bound hi of the smoother's interval (0 for
// the last) of matrix l in rows[l], nnz[l], hi[l], l < n.  Two more entries where cap allows: [n] the last call's cycles, the products
// inside them (with A_l, P and R) and the launches of the object's own kernels inside them; [n + 1] the set-up's host time and its upload
// time in microseconds, and in hi[n + 1] the operator complexity (the entries of all matrices over those of the first).  Returns n, 0
// when no hierarchy has been built; at most cap entries are written.
extern "C" int rails_iter_amg_info(const rails_iter *it, int64_t *rows, int64_t *nnz, double *hi, int cap)
{
    RAILS_REQUIRE(it && cap >= 0, "rails_iter_amg_info: bad argument");
    return hierarchy_info(it, 0, rows, nnz, hi, cap);
}

namespace {

// rails_iter_amg_info (block 0) and rails_iter_block_amg_info (block 1) on the hierarchy of their kind
int hierarchy_info(const rails_iter *it, int block, int64_t *rows, int64_t *nnz, double *hi, int cap)
{
    const Amg *H = it->hier;
    if (!H || (H->b != 0) != (block != 0)) return 0;
    const int n = (int)H->lv.size() + 1;
    double total = (double)H->coarse_nnz;
    for (const AmgLevel &L : H->lv) total += (double)L.nnz;
    for (int l = 0; l < n + 2 && l < cap; ++l) {
        int64_t r, z;
        double v;
        if (l < n - 1) {
            r = H->lv[(size_t)l].n;
            z = H->lv[(size_t)l].nnz;
            v = H->lv[(size_t)l].hi;
        } else if (l == n - 1) {
            r = H->n_coarse;
            z = H->coarse_nnz;
            v = 0.0;
        } else if (l == n) {
            r = it->last_cycles;
            z = it->last_cycle_products;
            v = (double)it->last_cycle_launches;
        } else {
            r = (int64_t)(H->host_seconds * 1e6);
            z = (int64_t)(H->upload_seconds * 1e6);
            v = total / (double)(H->lv.empty() ? H->coarse_nnz : H->lv[0].nnz);
        }
        if (rows) rows[l] = r;
        if (nnz) nnz[l] = z;
        if (hi) hi[l] = v;
    }
    return n;
}

// before a solve or an application with "amg" on: the hierarchy when there is none yet, the level panels at the work panels' width
int amg_prepare(rails_ctx *c, rails_iter *it)
{
    if (it->block_amg) {
        if (!it->hier || !it->hier->b) RAILS_TRY(rails_iter_block_amg_setup(c, it));
    } else if (!it->hier || it->hier->b)
        RAILS_TRY(rails_iter_amg_setup(c, it));
    return amg_grow(c, it);
}

// What rails_iter_solve (`solve`) and rails_iter_precondition begin with: the checks of the arguments, the counters of the call at zero,
// the work panels (`also`: panels wanted beside those the method uses), the hierarchy, the columns' scalars, and the plan in `run`.
// Nothing is queued before it has returned.  With nc == 0 nothing is allocated or planned.
//
// Collective on a context that reduces.  The rule that keeps the ranks from deadlocking: every decision that changes how many
// collectives are issued -- a refusal, the group loop, the number of iterations queued, the early exit, the non-finite right-hand side's
// RAILS_EINVAL -- is a function of the arguments and settings every rank passes alike (nc, trans, max_iterations, check_every) and of
// all-reduced data (the columns' scalars and the counts in `status`, the same bits on every rank), never of this rank's rows.
int begin_call(rails_ctx *c, rails_iter *it, const char *who, bool solve, int trans, const rails_panel *X, int xc0, int nc, rails_panel *Y, int yc0, unsigned also, Run &run)
{
    RAILS_REQUIRE(c && it && X && Y, "%s: null argument", who);
    RAILS_REQUIRE(c == it->ctx, "%s: the object belongs to another context", who);
    RAILS_REQUIRE(!trans || (it->A->n_ghost == 0 && it->A->n_send == 0 && it->A->ncols_ext == it->A->m),
                  "%s: the transposed solve of a row-partitioned operator (ghost rows) is not available: rails_spmm's transposed product is single GPU", who);
    RAILS_REQUIRE(X->m == it->m && Y->m == it->m, "%s: the operator has %lld rows, X %lld, Y %lld", who, (long long)it->m, (long long)X->m, (long long)Y->m);
    RAILS_REQUIRE(xc0 >= 0 && nc >= 0 && xc0 + nc <= X->cap && yc0 >= 0 && yc0 + nc <= Y->cap, "%s: column windows outside the panels", who);
    if (X->d == Y->d) RAILS_REQUIRE(xc0 + nc <= yc0 || yc0 + nc <= xc0, "%s: X and Y windows alias", who);
    it->last_dots = it->last_launches = it->last_products = it->last_poly = it->last_fused = it->last_allreduces = it->last_halo = 0;
    it->last_cycles = it->last_cycle_products = it->last_cycle_launches = 0;
    if (solve) it->last.clear();
    if (nc == 0) return RAILS_OK;
    RAILS_TRY(grow_work(c, it, std::min(nc, RAILS_ITER_GROUP), also));
    if (it->amg || it->block_amg) RAILS_TRY(amg_prepare(c, it));
    if (solve) RAILS_TRY(grow_cols(c, it, nc));
    run.c = c;
    run.it = it;
    run.trans = trans ? 1 : 0;
    run.bj = it->block_jacobi && it->bj_dev ? it->bj_b : 0;
    RAILS_REQUIRE(!run.bj || bj_apply(run.bj, false), "%s: no block-Jacobi kernels for block size %d (RAILS_BJ_TABLE)", who, run.bj);
    run.jac = run.bj || (it->jacobi && it->dinv);
    run.tol2 = solve ? it->tol * it->tol : 0.0;
    run.cols = nullptr;
    return plan_call(run, who);
}

} // namespace

extern "C" int rails_iter_solve(rails_ctx *c, rails_iter *it, int trans, const rails_panel *X, int xc0, int nc, rails_panel *Y, int yc0)
{
    if (c) hipSetDevice(c->device);
    rails_slow_guard slow__(c, "rails_iter_solve", nc, it ? it->m : 0);
    Run run;
    RAILS_TRY(begin_call(c, it, "rails_iter_solve", true, trans, X, xc0, nc, Y, yc0, 0, run));
    if (nc == 0) return RAILS_OK;
    int32_t *status = (int32_t *)it->pinned;
    for (int g0 = 0; g0 < nc; g0 += RAILS_ITER_GROUP) {
        const int w = std::min(RAILS_ITER_GROUP, nc - g0);
        plan_group(run, w);
        run.cols = it->cols_dev + g0;
        RAILS_TRY(rails_panel_copy(c, X, xc0 + g0, w, it->w[W_R], 0));
        RAILS_TRY(run.start());
        for (int queued = 0, first = 1;; first = 0) {
            const int n = std::max(0, std::min(it->check_every, it->maxit - queued));
            for (int k = 0; k < n; ++k) RAILS_TRY(run.iteration());
            queued += n;
            RAILS_HIP_CHECK(hipGetLastError());
            RAILS_HIP_CHECK(hipMemcpyAsync(status, it->status_dev, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
            RAILS_HIP_CHECK(rails_stream_sync(c));
            if (first && status[1] > 0) {
                rails_set_error("rails_iter_solve: %d column(s) of the right-hand side in columns [%d, %d) are not finite", (int)status[1], g0, g0 + w);
                return RAILS_EINVAL;
            }
            if (status[0] == 0 || queued >= it->maxit) break;
        }
        RAILS_TRY(rails_panel_copy(c, it->w[W_X], 0, w, Y, yc0 + g0));
    }
    rails_iter_col *host_cols = (rails_iter_col *)((char *)it->pinned + 64);
    RAILS_HIP_CHECK(hipMemcpyAsync(host_cols, it->cols_dev, (size_t)nc * sizeof(rails_iter_col), hipMemcpyDeviceToHost, c->stream));
    RAILS_HIP_CHECK(rails_stream_sync(c));
    it->last.assign(host_cols, host_cols + nc);
    int flagged = 0;
    for (const rails_iter_col &col : it->last) {
        it->tot_iterations += col.iter;
        flagged += (col.flags & RAILS_ITER_CONVERGED) ? 0 : 1;
    }
    it->tot_solves += 1;
    it->tot_columns += nc;
    it->tot_flagged += flagged;
    it->tot_products += it->last_products;
    if (flagged && it->strict) {
        rails_set_error("rails_iter_solve: %d of %d columns did not reach the tolerance %g (strict)", flagged, nc, it->tol);
        return RAILS_ENOCONV;
    }
    return RAILS_OK;
}

// Y = p_K(G A) G X, the preconditioner the CG solve applies to its residual, on its own: a fixed linear approximate inverse.  K = 0: G X.
extern "C" int rails_iter_precondition(rails_ctx *c, rails_iter *it, const rails_panel *X, int xc0, int nc, rails_panel *Y, int yc0)
{
    if (c) hipSetDevice(c->device);
    Run run;
    RAILS_TRY(begin_call(c, it, "rails_iter_precondition", false, 0, X, xc0, nc, Y, yc0, 1u << W_R | 1u << W_Z | 1u << W_D, run));
    if (nc == 0) return RAILS_OK;
    for (int g0 = 0; g0 < nc; g0 += RAILS_ITER_GROUP) {
        const int w = std::min(RAILS_ITER_GROUP, nc - g0);
        plan_group(run, w);
        RAILS_TRY(rails_panel_copy(c, X, xc0 + g0, w, it->w[W_R], 0));
        RAILS_TRY(run.precondition());
        RAILS_TRY(rails_panel_copy(c, it->w[W_Z], 0, w, Y, yc0 + g0));
    }
    RAILS_HIP_CHECK(hipGetLastError());
    return RAILS_OK;
}

// info[0] most iterations of a column in the last solve, [1] inner products of the last solve (per column and quantity), [2] kernel
// launches of the library's own passes in it, [3] its columns that did not converge (any flag but converged), [4] those of them that
// broke down, [5] worst relative residual of the recurrence, [6] work-panel columns, [7] products with A in the last solve; totals since
// creation: [8] solves, [9] columns, [10] iterations summed over the columns, [11] flagged columns, [12] products with A; the polynomial
// preconditioner: [13] its applications in the last solve, [14] launches of the fused step kernel in it, [15] hi and [16] lo of the
// interval in use (0 with degree 0); a context that reduces: [17] all-reduces issued in the last call (per group of columns CG 1 at the start
// and 2 per queued iteration, BiCGStab 1 and 3; the polynomial adds none), [18] ghost-row exchanges the object issued itself (one before
// every fused step in its ghost-row form; those inside rails_spmm are not counted).  [7] counts every product, those inside the fused step
// included.
extern "C" int rails_iter_stats(const rails_iter *it, double *info, int cap)
{
    RAILS_REQUIRE(it && info && cap >= 0, "rails_iter_stats: bad argument");
    double most = 0, unconv = 0, broke = 0, worst = 0;
    for (const rails_iter_col &c : it->last) {
        most = std::max(most, (double)c.iter);
        if (!(c.flags & RAILS_ITER_CONVERGED)) unconv += 1;
        if (c.flags & RAILS_ITER_BREAKDOWN) broke += 1;
        const double rel = c.bb > 0.0 ? std::sqrt(c.rr / c.bb) : 0.0;
        if (!(rel <= worst)) worst = rel; // a NaN shows
    }
    const double hi = it->poly_degree > 0 ? poly_hi(it) : 0.0;
    const double v[19] = {most, (double)it->last_dots, (double)it->last_launches, unconv, broke, worst, (double)it->work_cols, (double)it->last_products,
                          it->tot_solves, it->tot_columns, it->tot_iterations, it->tot_flagged, it->tot_products,
                          (double)it->last_poly, (double)it->last_fused, hi, hi / it->poly_ratio, (double)it->last_allreduces, (double)it->last_halo};
    const int k = std::min(cap, 19);
    for (int i = 0; i < k; ++i) info[i] = v[i];
    return k;
}

// per column of the last solve: iterations, relative residual of the recurrence, flags (RAILS_ITER_* of iter_scalars.h: 2 converged,
// 4 stopped at max_iterations, 8 breakdown, 16 non-finite).  Returns the number of columns of the last solve; at most cap are written.
extern "C" int rails_iter_columns(const rails_iter *it, int32_t *iterations, double *relres, int32_t *flags, int cap)
{
    RAILS_REQUIRE(it && cap >= 0, "rails_iter_columns: bad argument");
    const int n = (int)it->last.size();
    for (int j = 0; j < std::min(n, cap); ++j) {
        const rails_iter_col &c = it->last[j];
        if (iterations) iterations[j] = c.iter;
        if (relres) relres[j] = c.bb > 0.0 ? std::sqrt(c.rr / c.bb) : 0.0;
        if (flags) flags[j] = c.flags;
    }
    return n;
}

extern "C" int rails_csr_create_iter(rails_ctx *c, rails_iter *it, rails_csr **out)
{
    RAILS_REQUIRE(c && it && out, "rails_csr_create_iter: null argument");
    RAILS_REQUIRE(c == it->ctx, "rails_csr_create_iter: the object belongs to another context");
    rails_csr *A = new rails_csr();
    A->ctx = c;
    A->m = it->m;
    A->ncols_ext = it->m;
    A->kind = rails_csr::ITER;
    A->delegate = it;
    A->last_kernel = it->method == RAILS_ITER_CG ? "iter_cg" : "iter_bicgstab";
    *out = A;
    return RAILS_OK;
}
