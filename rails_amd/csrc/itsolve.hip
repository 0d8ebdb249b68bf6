// itsolve.hip -- A^-1 X (or A^-T X) by an iteration that stays on the device, as a library object: the approximate inverse the reference
// allows for its inverse and extended Krylov projections (matlab/RAILSsolver.m:19-23, opts.Ainv: "This can be approximate") where a
// sparse LU (splu.hip) is latency-bound or cannot be formed at all.  Conjugate gradients and right-preconditioned BiCGStab, with Jacobi,
// a Chebyshev polynomial, a multigrid cycle, block Jacobi or a block multigrid cycle (DESIGN.md sections 14 to 19).  The files:
//   iter_precond.h      which preconditioner may be turned on and what is in effect for a call: the one rule, host-tested
//   iter_object.h       struct rails_iter, the hierarchy, what the three sources share
//   iter_setup.hip      create and destroy, rails_iter_set, the work panels, the statistics
//   iter_hierarchy.hip  the hierarchies' upload, set-up and info, the install of the block-Jacobi blocks
//   itsolve.hip         this file: every launch.  The kernels (iter_kernels.inc), a sweep and a call (struct Sweep, struct Run), the plan
//                       of a call, made before anything is queued (begin_call, plan_call, plan_group), rails_iter_solve and
//                       rails_iter_precondition
// and beside them iter_geom.h (the geometry of a pass), iter_scalars.h, cheb_coef.h, block_amg_choice.h, iter_agree.h.
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
#include "iter_object.h"

#include <algorithm>
#include <cmath>

#include "block_amg_choice.h"
#include "bsr_choice.h"
#include "cheb_coef.h"
#include "iter_geom.h"

namespace {

using PassGeom = rails_pass_geom; // (the name the kernels use)

#include "iter_kernels.inc"

// The block forms of the passes that apply G, one row of kernels per block size of RAILS_BJ_TABLE (iter_kernels.inc).  A block size
// outside the table has no row, which the call refuses before anything is queued (begin_call, plan_call).
struct BjKernels {
    int b;
    decltype(&k_cg_init_bj<2>) cg_init;
    decltype(&k_cg_update_bj<2>) cg_update;
    decltype(&k_bj_apply<2>) apply;
    decltype(&k_bi_dir_bj<2, false>) bi_dir[2]; // [transposed]
    decltype(&k_bi_s_bj<2, false>) bi_s[2];
    decltype(&k_cheb_init_bj<2>) cheb_init;
    decltype(&k_cheb_pass_bj<2>) cheb_pass;
};
#define RAILS_BJ_ROW(B) {B, &k_cg_init_bj<B>, &k_cg_update_bj<B>, &k_bj_apply<B>, {&k_bi_dir_bj<B, false>, &k_bi_dir_bj<B, true>}, {&k_bi_s_bj<B, false>, &k_bi_s_bj<B, true>}, &k_cheb_init_bj<B>, &k_cheb_pass_bj<B>},
const BjKernels kBjKernels[] = {RAILS_BJ_TABLE(RAILS_BJ_ROW)};
#undef RAILS_BJ_ROW
const BjKernels *bj_kernels(int b)
{
    for (const BjKernels &k : kBjKernels)
        if (k.b == b) return &k;
    return nullptr;
}

// The two kernels on the shared block-row body (bsr_row_gather.inc), by instantiation of RAILS_BSR_TABLE (bsr_choice.h)
struct ChebStepBsr {
    static constexpr const char *name = "k_cheb_step_bsr";
    template <int B, int LPR>
    static auto kernel() { return &k_cheb_step_bsr<B, LPR>; }
};
struct AmgResidualBsr {
    static constexpr const char *name = "k_amg_residual_bsr";
    template <int B, int LPR>
    static auto kernel() { return &k_amg_residual_bsr<B, LPR>; }
};

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
    rails_precond_effect pc;         // what is in effect (iter_precond.h): every branch on the preconditioner below reads this and nothing else
    const BjKernels *bjk = nullptr; // pc.pass is RAILS_PC_PASS_BLOCKS: the block forms of the passes for pc.b
    double tol2;
    // sw[0] is the polynomial's sweep, or sw[l] the smoother of level l of a cycle; the last level's passes run on gc
    bool cycle = false; // inside a cycle: the cycle's counters count too
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
        const double sign = pc.sign;
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
            pass(s.g, s.slabs, bj_kernels(s.bs)->cheb_init, s.ginv, s.theta, (const double *)s.r->d, s.d->d, s.z[s.at]->d);
        else
            pass(s.g, s.slabs, k_cheb_init, s.gvec, s.gs, s.theta, s.r->d, s.d->d, s.z[s.at]->d);
    }
    // a kernel on the shared block-row body (ChebStepBsr, AmgResidualBsr) over a block sweep's matrix, launched as k_spmm_bsr is for the
    // group's width.  `rest` is what follows the body's own arguments.  One product.
    template <class Which, class... Rest>
    int block_gather(Which, const Sweep &s, const double *zin, Rest... rest)
    {
        const BsrChoice &k = s.step.k;
#define RAILS_BAMG_CASE(B, LPR)                                                                                                                   \
    case rails_bsr_inst(B, LPR): launch(Which::template kernel<B, LPR>(), k.grid, k.threads, s.mb, s.browptr, s.bcol, s.bval, zin, g.ld, g.ncw, k.rpg, k.bpx, rest...); break;
        switch (k.key()) {
            RAILS_BSR_TABLE(RAILS_BAMG_CASE)
        default: rails_set_error("rails_iter: %s<%d, %d> is not among the instantiations of bsr_choice.h", Which::name, k.b, k.lpr); return RAILS_EINVAL;
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
                pass(s.g, s.slabs, bj_kernels(s.bs)->cheb_pass, s.ginv, a, b, (const double *)s.q->d, (const double *)s.r->d, s.d->d, zin->d);
            else
                pass(s.g, s.slabs, k_cheb_pass, s.gvec, s.gs, a, b, s.q->d, s.r->d, s.d->d, zin->d);
            return RAILS_OK;
        }
        if (s.bs) {
            s.at ^= 1;
            RAILS_TRY(block_gather(ChebStepBsr{}, s, (const double *)zin->d, s.ginv, a, b, (const double *)s.r->d, s.d->d, s.z[s.at]->d));
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
        sweep_start(sw[0], pc.K);
        for (int k = 0; k < pc.K; ++k) RAILS_TRY(sweep_step(sw[0], sw[0].a[k], sw[0].b[k]));
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
                RAILS_TRY(block_gather(AmgResidualBsr{}, s, (const double *)z->d, (const double *)s.r->d, s.q->d));
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
        if (pc.pass == RAILS_PC_PASS_BLOCKS) { // (neither the polynomial nor a cycle is on: iter_precond.h)
            it->last_poly++;
            pass(g, nslab, bjk->apply, (const double *)it->bj_dev, (const double *)d(W_R), d(W_Z));
            return RAILS_OK;
        }
        cycle = pc.cycle(); // (off again however the cycle ends)
        const int rc = cycle ? vcycle() : polynomial();
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
        const bool diag = pc.pass == RAILS_PC_PASS_DIAG;
        if (pc.beyond != RAILS_PC_BEYOND_NONE) {
            RAILS_TRY(precondition());
            RAILS_TRY(pass_sums(k_cg_init_poly, d(W_R), d(W_Z), d(W_P), d(W_X)));
        } else if (pc.pass == RAILS_PC_PASS_BLOCKS)
            RAILS_TRY(pass_sums(bjk->cg_init, (const double *)it->bj_dev, (const double *)d(W_R), d(W_Z), d(W_P), d(W_X)));
        else
            RAILS_TRY(pass_sums(diag ? k_cg_init<true> : k_cg_init<false>, it->dinv, d(W_R), diag ? d(W_Z) : nullptr, d(W_P), d(W_X)));
        it->last_dots += 2 * g.ncw;
        return scalars(STEP_CG_INIT, 2);
    }
    int iteration()
    {
        const bool beyond = pc.beyond != RAILS_PC_BEYOND_NONE, blocks = pc.pass == RAILS_PC_PASS_BLOCKS, diag = pc.pass == RAILS_PC_PASS_DIAG;
        if (it->method == RAILS_ITER_CG) {
            RAILS_TRY(product(W_P, W_Q));
            RAILS_TRY(dots(1, W_P, W_Q, W_P, W_Q));
            RAILS_TRY(scalars(STEP_CG_ALPHA, 1));
            if (beyond) {
                // the update without its own z (its partial sums are overwritten below), the polynomial, then r.z and r.r in the layout
                // the scalar step reads; K products in a row without an inner product, a scalar kernel or a read-back between them
                RAILS_TRY(pass_sums(k_cg_update<false>, cols, it->dinv, d(W_P), d(W_Q), d(W_X), d(W_R), nullptr));
                RAILS_TRY(precondition());
                RAILS_TRY(dots(2, W_R, W_Z, W_R, W_R));
            } else {
                if (blocks)
                    RAILS_TRY(pass_sums(bjk->cg_update, (const rails_iter_col *)cols, (const double *)it->bj_dev, (const double *)d(W_P), (const double *)d(W_Q), d(W_X),
                                        d(W_R), d(W_Z)));
                else
                    RAILS_TRY(pass_sums(diag ? k_cg_update<true> : k_cg_update<false>, cols, it->dinv, d(W_P), d(W_Q), d(W_X), d(W_R), diag ? d(W_Z) : nullptr));
                it->last_dots += 2 * g.ncw;
            }
            RAILS_TRY(scalars(STEP_CG_BETA, 2));
            pass(g, nslab, k_cg_dir, cols, d(beyond || blocks || diag ? W_Z : W_R), d(W_P));
            return RAILS_OK;
        }
        const int ph = blocks || diag ? W_Z : W_P, sh = blocks || diag ? W_SH : W_R;
        if (blocks)
            pass(g, nslab, bjk->bi_dir[trans != 0], (const rails_iter_col *)cols, (const double *)it->bj_dev, (const double *)d(W_R), (const double *)d(W_Q), d(W_P), d(W_Z));
        else
            pass(g, nslab, diag ? k_bi_dir<true> : k_bi_dir<false>, cols, it->dinv, d(W_R), d(W_Q), d(W_P), diag ? d(W_Z) : nullptr);
        RAILS_TRY(product(ph, W_Q)); // v = A p^
        RAILS_TRY(dots(1, W_RH, W_Q, W_RH, W_Q));
        RAILS_TRY(scalars(STEP_BI_ALPHA, 1));
        if (blocks)
            pass(g, nslab, bjk->bi_s[trans != 0], (const rails_iter_col *)cols, (const double *)it->bj_dev, (const double *)d(W_Q), d(W_R), d(W_SH));
        else
            pass(g, nslab, diag ? k_bi_s<true> : k_bi_s<false>, cols, it->dinv, d(W_Q), d(W_R), diag ? d(W_SH) : nullptr);
        RAILS_TRY(product(sh, W_T)); // t = A s^
        RAILS_TRY(dots(2, W_T, W_R, W_T, W_T));
        RAILS_TRY(scalars(STEP_BI_OMEGA, 2));
        RAILS_TRY(pass_sums(k_bi_update, cols, d(ph), d(sh), d(W_T), d(W_RH), d(W_X), d(W_R)));
        it->last_dots += 2 * g.ncw;
        return scalars(STEP_BI_END, 2);
    }
};

// The plan of a call, made before anything is queued: the sweeps (operator, panels, interval, coefficients, whether the steps run on the
// fused kernel) of the polynomial or of every multigrid level.  Every refusal of a preconditioner is here.  The work panels and the
// hierarchy must be there (the fused kernel's rule looks at the panels' row stride).
int plan_call(Run &run, const char *who)
{
    rails_iter *it = run.it;
    rails_csr *A = it->A;
    const int ld = it->w[W_R]->ld;
    const rails_precond_effect &pc = run.pc;
    run.sw[0] = Sweep{A, it->m, pc.pass == RAILS_PC_PASS_DIAG ? it->dinv : nullptr, it->defsign, it->w[W_R], {it->w[W_Z], it->w[W_Z2]}, it->w[W_D], it->w[W_Q]};
    if (pc.cycle()) { // (either cycle: Run::vcycle on the sweeps made here)
        const Amg &H = *it->hier;
        for (size_t l = 0; l < H.lv.size(); ++l) {
            const AmgLevel &L = H.lv[l];
            Sweep &s = run.sw[l];
            if (l > 0) s = Sweep{L.A, L.n, L.dinv, 1.0, L.w[L_R], {L.w[L_Z], L.w[L_Z2]}, L.w[L_D], L.w[L_Q]};
            s.gvec = L.dinv; // (level 0: the object's operator in the object's panels, with the hierarchy's diagonal)
            s.gs = 1.0;
            RAILS_REQUIRE(rails_cheb_coef(L.hi / it->amg_ratio, L.hi, it->amg_degree, &s.theta, s.a, s.b), "rails_iter: no smoother of degree %d on [%g, %g] (level %d)",
                          it->amg_degree, L.hi / it->amg_ratio, L.hi, (int)l);
            if (pc.beyond == RAILS_PC_BEYOND_BLOCK_CYCLE) { // the block hierarchy: G is the level's inverse diagonal blocks; whether the step is fused depends on the group (plan_group)
                s.gvec = nullptr;
                s.ginv = L.ginv;
                s.bs = H.b;
                RAILS_REQUIRE(rails_bsr_device_arrays(L.A, &s.mb, &s.max_brow, &s.browptr, &s.bcol, &s.bval), "%s: level %d of the block hierarchy is not a block-CSR handle", who, (int)l);
                RAILS_REQUIRE(bj_kernels(s.bs), "%s: no block kernels for block size %d (RAILS_BJ_TABLE)", who, s.bs);
                s.fused = false;
            } else
                s.fused = it->poly_fused && rails_cheb_fused_eligible(true, 0, L.n, ld);
        }
        return RAILS_OK;
    }
    if (pc.beyond != RAILS_PC_BEYOND_POLY) return RAILS_OK;
    Sweep &s = run.sw[0];
    const double hi = rails_iter_poly_hi(it, pc.pass);
    RAILS_REQUIRE((hi > 0.0 && rails_iter_finite(hi)) || run.it->A->kind != rails_csr::BSR,
                  "%s: poly_degree %d needs an upper bound on the spectrum: a block-CSR operator keeps no scalar CSR arrays to take one from, set \"eig_max\"", who, pc.K);
    RAILS_REQUIRE(hi > 0.0 && rails_iter_finite(hi),
                  "%s: poly_degree %d needs an upper bound on the spectrum: the operator keeps no CSR arrays on the host to take one from, set \"eig_max\"", who, pc.K);
    RAILS_REQUIRE(rails_cheb_coef(hi / it->poly_ratio, hi, pc.K, &s.theta, s.a, s.b), "%s: no polynomial of degree %d on [%g, %g]", who, pc.K, hi / it->poly_ratio, hi);
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
    const int nl = run.pc.cycle() ? (int)it->hier->lv.size() : 0;
    const int hb = run.pc.beyond == RAILS_PC_BEYOND_BLOCK_CYCLE ? it->hier->b : 0; // the block hierarchy: every pass of every level on slabs of whole block rows
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
    if (run.pc.pass == RAILS_PC_PASS_BLOCKS) run.g = rails_iter_pass_geom_block(it->m, w, ld, run.pc.b, &run.nslab); // every pass of the group, the point ones too
    if (run.pc.cycle()) run.gc = hb ? rails_iter_pass_geom_block(it->hier->n_coarse, w, ld, hb, &run.slabs_c) : rails_iter_pass_geom(it->hier->n_coarse, w, ld, &run.slabs_c);
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
    run.pc = rails_precond_effect_of(rails_iter_facts(it));
    RAILS_TRY(rails_iter_grow_work(c, it, std::min(nc, RAILS_ITER_GROUP), run.pc.panels | also));
    if (run.pc.cycle()) RAILS_TRY(rails_iter_amg_prepare(c, it, run.pc.beyond == RAILS_PC_BEYOND_BLOCK_CYCLE));
    if (solve) RAILS_TRY(rails_iter_grow_cols(c, it, nc));
    run.c = c;
    run.it = it;
    run.trans = trans ? 1 : 0;
    run.bjk = run.pc.pass == RAILS_PC_PASS_BLOCKS ? bj_kernels(run.pc.b) : nullptr;
    RAILS_REQUIRE(run.pc.pass != RAILS_PC_PASS_BLOCKS || run.bjk, "%s: no block-Jacobi kernels for block size %d (RAILS_BJ_TABLE)", who, run.pc.b);
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
