// orth.hip -- orthonormalisation of newly appended panel columns.
//
// Reference: StlWrapper::orthogonalize (src/StlWrapper.cpp:305-321): for every column past the
// watermark, normalise, twice subtract the projection on ALL previous columns, normalise -- four
// passes over the m x k panel per new column.
//
// Here (auto / block method): the w new columns W are treated as a block,
//     twice:  C = V_old^T W  (MFMA Gram, one all-reduce);  W -= V_old C  (MFMA panel GEMM)
//     twice:  G = W^T W;  G = R^T R (host Cholesky, w x w);  W <- W R^-1          (CholQR2)
// which is two Gram and two update passes for all w columns together.  Gram-Schmidt on the columns
// of W in order and the Cholesky factor of W^T W produce the same Q (QR with positive diagonal is
// unique), so the result equals the reference's up to rounding.  When the block Gram matrix is
// numerically rank deficient (Cholesky fails or its diagonal collapses) the routine falls back to
// the reference's column-wise recurrence, evaluated with the same device kernels.
//
// rails_orthogonalize_deflated does the same with a nullspace N (q orthonormal columns of another panel) projected out in every
// projection round: [N | V_old] is one left operand, so a round is one Gram pass over W, one all-reduce and one update pass
// (rails_gram2_dev, rails_panel_gemm2_dev).  With q = 0 it is rails_orthogonalize.
//
// rails_orthogonalize_range (further down) is the rank-revealing form for a start space: columns that may be dependent, any number of
// them, dropped instead of replaced; it shares project_block with the two above and never takes their column-wise paths.
//
// This file is the algorithm only: every kernel it launches is in dense_gram.hip and dense_gemm.hip, where the one- and two-segment forms share one body.
#include "rails_internal.h"

#include <cmath>
#include <cstdlib>
#include <vector>

namespace {

int sync_small_to_host(rails_ctx *c, size_t n, std::vector<double> &out)
{
    RAILS_TRY(rails_pinned_reserve(c, n * sizeof(double)));
    RAILS_HIP_CHECK(hipMemcpyAsync(c->pinned, c->small, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    RAILS_HIP_CHECK(rails_stream_sync(c));
    out.assign(c->pinned, c->pinned + n);
    return RAILS_OK;
}

int upload_small(rails_ctx *c, const std::vector<double> &in, double *dst)
{
    RAILS_TRY(rails_pinned_begin_write(c, in.size() * sizeof(double)));
    memcpy(c->pinned, in.data(), in.size() * sizeof(double));
    RAILS_HIP_CHECK(hipMemcpyAsync(dst, c->pinned, in.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    RAILS_HIP_CHECK(rails_stream_sync(c));
    return RAILS_OK;
}

// the inverse of the upper triangular R (w x w, column-major): R * Rinv = I solved column by column
std::vector<double> upper_inverse(const std::vector<double> &R, int w)
{
    std::vector<double> Rinv((size_t)w * w, 0.0);
    for (int j = 0; j < w; ++j) {
        Rinv[j + (size_t)j * w] = 1.0 / R[j + (size_t)j * w];
        for (int i = j - 1; i >= 0; --i) {
            double s = 0.0;
            for (int l = i + 1; l <= j; ++l) s += R[i + (size_t)l * w] * Rinv[l + (size_t)j * w];
            Rinv[i + (size_t)j * w] = -s / R[i + (size_t)i * w];
        }
    }
    return Rinv;
}

// 2-norm of one column = sqrt(|v^T v|) (StlWrapper::norm on a single column, src/StlWrapper.cpp:280-288)
int column_norm(rails_ctx *c, const rails_panel *V, int col, double *nrm)
{
    RAILS_TRY(rails_small_reserve(c, sizeof(double)));
    RAILS_TRY(rails_gram_dev(c, V->d + col, V->ld, V->d + col, V->ld, V->m, 1, 1, c->small));
    RAILS_TRY(rails_allreduce_dev(c, c->small, 1));
    std::vector<double> h;
    RAILS_TRY(sync_small_to_host(c, 1, h));
    *nrm = std::sqrt(std::fabs(h[0]));
    return RAILS_OK;
}

// one pass "v -= P (P^T v)" of column i against the columns [c0, c1) of V
int project_column(rails_ctx *c, rails_panel *V, int i, int c0, int c1)
{
    const int n = c1 - c0;
    if (n <= 0) return RAILS_OK;
    RAILS_TRY(rails_small_reserve(c, (size_t)n * sizeof(double)));
    RAILS_TRY(rails_gram_dev(c, V->d + c0, V->ld, V->d + i, V->ld, V->m, n, 1, c->small));
    RAILS_TRY(rails_allreduce_dev(c, c->small, (size_t)n));
    return rails_panel_gemm_dev(c, -1.0, V->d + c0, V->ld, n, c->small, 1, 1.0, V->d + i, V->ld, V->m);
}

// The nullspace of rails_orthogonalize_deflated: columns [c0, c0 + q) of panel N (q = 0: none)
struct Nullspace {
    const rails_panel *N = nullptr;
    int c0 = 0, q = 0;
};

// W (w columns from column k_old of V) -= [N V_old] ([N V_old]' W): one Gram pass over W, one all-reduce, one update pass.  Above 32 columns
// of N or of W the two-segment kernels are not instantiated: two Gram and two update calls, still one all-reduce.  Without a nullspace
// (q = 0) that is the one-segment Gram and update against V_old alone.
int project_block(rails_ctx *c, rails_panel *V, int k_old, int w, Nullspace const &ns)
{
    const int q = ns.q, a = q + k_old;
    if (a == 0) return RAILS_OK;
    const double *Nd = q ? ns.N->d + ns.c0 : nullptr;
    const int ldn = q ? ns.N->ld : 0;
    double *W = V->d + k_old;
    RAILS_TRY(rails_small_reserve(c, (size_t)a * w * sizeof(double)));
    if (q > 0 && q <= 32 && w <= 32) {
        RAILS_TRY(rails_gram2_dev(c, Nd, ldn, q, V->d, V->ld, k_old, W, V->ld, V->m, w, c->small));
        RAILS_TRY(rails_allreduce_dev(c, c->small, (size_t)a * w));
        return rails_panel_gemm2_dev(c, -1.0, Nd, ldn, q, V->d, V->ld, k_old, c->small, w, W, V->ld, V->m);
    }
    double *D = c->small, *Cv = c->small + (size_t)q * w; // N'W (q x w), V_old'W (k_old x w)
    if (q > 0) RAILS_TRY(rails_gram_dev(c, Nd, ldn, W, V->ld, V->m, q, w, D));
    if (k_old > 0) RAILS_TRY(rails_gram_dev(c, V->d, V->ld, W, V->ld, V->m, k_old, w, Cv));
    RAILS_TRY(rails_allreduce_dev(c, c->small, (size_t)a * w));
    for (int j0 = 0; j0 < w; j0 += 256) { // panel GEMM handles <= 256 output columns per launch
        const int wc = w - j0 < 256 ? w - j0 : 256;
        if (q > 0) RAILS_TRY(rails_panel_gemm_dev(c, -1.0, Nd, ldn, q, D + (size_t)j0 * q, wc, 1.0, W + j0, V->ld, V->m));
        if (k_old > 0) RAILS_TRY(rails_panel_gemm_dev(c, -1.0, V->d, V->ld, k_old, Cv + (size_t)j0 * k_old, wc, 1.0, W + j0, V->ld, V->m));
    }
    return RAILS_OK;
}

// one pass of column i against N and the columns [0, i) of V, in the same way
int project_column(rails_ctx *c, rails_panel *V, int i, Nullspace const &ns)
{
    if (ns.q == 0) return project_column(c, V, i, 0, i);
    const int q = ns.q, a = q + i;
    const double *Nd = ns.N->d + ns.c0;
    RAILS_TRY(rails_small_reserve(c, (size_t)a * sizeof(double)));
    RAILS_TRY(rails_gram2_dev(c, Nd, ns.N->ld, q, V->d, V->ld, i, V->d + i, V->ld, V->m, 1, c->small));
    RAILS_TRY(rails_allreduce_dev(c, c->small, (size_t)a));
    return rails_panel_gemm2_dev(c, -1.0, Nd, ns.N->ld, q, V->d, V->ld, i, c->small, 1, V->d + i, V->ld, V->m);
}

// The reference's recurrence (src/StlWrapper.cpp:308-319) for columns [from, to): normalise, twice subtract the
// projection on ALL previous columns (and on the nullspace), normalise.
int columnwise(rails_ctx *c, rails_panel *V, int from, int to, Nullspace const &ns = Nullspace())
{
    for (int i = from; i < to; ++i) {
        double nrm = 0.0;
        RAILS_TRY(column_norm(c, V, i, &nrm));
        RAILS_TRY(rails_panel_scale(c, V, i, 1, 1.0 / nrm));
        for (int pass = 0; pass < 2; ++pass) RAILS_TRY(project_column(c, V, i, ns));
        RAILS_TRY(column_norm(c, V, i, &nrm));
        RAILS_TRY(rails_panel_scale(c, V, i, 1, 1.0 / nrm));
    }
    return RAILS_OK;
}

// Fallback after the block projection against the old columns has already been applied to all new columns: Gram-Schmidt column by
// column, each column twice against ALL columns before it -- the old ones included.  (Until round 3 the two passes ran inside the
// block only, m x w traffic, and a column got the full treatment only when it lost more than five digits there.  A column that keeps a
// fraction f of its length inherits the defects of the block's earlier columns against the old ones magnified by 1 / f, and a chain of
// nearly dependent columns compounds that: the coordinate-space back end's copy of this shortcut cost it eight digits of V'AV on
// BASELINE configs[1], DESIGN.md section 5 (vi).  This path is rare -- the repair round takes the rank-deficient blocks -- so it pays the
// reference's price: src/StlWrapper.cpp:308-319.)
int columnwise_in_block(rails_ctx *c, rails_panel *V, int k_old, int w, Nullspace const &ns = Nullspace())
{
    for (int i = k_old; i < k_old + w; ++i) {
        double n0 = 0.0, n1 = 0.0;
        RAILS_TRY(column_norm(c, V, i, &n0));
        if (n0 > 0.0) RAILS_TRY(rails_panel_scale(c, V, i, 1, 1.0 / n0));
        for (int pass = 0; pass < 2; ++pass) RAILS_TRY(project_column(c, V, i, ns));
        RAILS_TRY(column_norm(c, V, i, &n1));
        if (!(n1 > 0.0) || !std::isfinite(n1)) {
            // nothing at all survived: the column was a bitwise copy of the one before it once that one had been orthogonalised (two
            // dependent columns that the repair round left identical).  The reference would divide by zero here; like the coordinate-space
            // back end's orthogonalize(), take a random direction instead and orthogonalise that.
            RAILS_TRY(rails_panel_random(c, V, i, 1));
            RAILS_TRY(column_norm(c, V, i, &n1));
            RAILS_TRY(rails_panel_scale(c, V, i, 1, 1.0 / n1));
            for (int pass = 0; pass < 2; ++pass) RAILS_TRY(project_column(c, V, i, ns));
            RAILS_TRY(column_norm(c, V, i, &n1));
        }
        if (!(n1 > 1e-5)) { // the column was normalised before the projection: n1 is the fraction that survived -- once more, from unit length
            RAILS_TRY(rails_panel_scale(c, V, i, 1, 1.0 / n1));
            for (int pass = 0; pass < 2; ++pass) RAILS_TRY(project_column(c, V, i, ns));
            RAILS_TRY(column_norm(c, V, i, &n1));
        }
        RAILS_TRY(rails_panel_scale(c, V, i, 1, 1.0 / n1));
    }
    return RAILS_OK;
}

// Repair step of the block method for a numerically rank-deficient block (typical in RAILS: the Ritz values of the
// residual operator come in +/- pairs whose vectors coincide once span(V) is projected out, so about every second
// expansion vector is dependent on its predecessors).  The reference's recurrence turns such a column into the
// normalised rounding noise of its projection and carries on.  Here: Cholesky of the block Gram matrix G with the
// dependent pivots skipped (r_ii = 1, row i of R zero): W <- W R^-1 orthonormalises the independent columns among
// themselves and leaves every dependent column as its (tiny) residual against the independent columns before it; those
// residuals are scaled to unit norm and the block procedure is run once more on the repaired block, which is then
// generically of full rank.  All block operations: no per-column passes over the m x k panel.
int repair_block(rails_ctx *c, rails_panel *V, int k_old, int w, const std::vector<double> &G, int *n_bad)
{
    std::vector<double> R((size_t)w * w, 0.0);
    std::vector<char> bad(w, 0);
    *n_bad = 0;
    for (int i = 0; i < w; ++i) {
        double piv = G[i + (size_t)i * w];
        for (int j = 0; j < i; ++j) {
            if (bad[j]) continue; // row j of R is zero beyond its diagonal
            double s = G[j + (size_t)i * w];
            for (int l = 0; l < j; ++l)
                if (!bad[l]) s -= R[l + (size_t)j * w] * R[l + (size_t)i * w];
            s /= R[j + (size_t)j * w];
            R[j + (size_t)i * w] = s;
            piv -= s * s;
        }
        if (piv > 1e-10 * G[i + (size_t)i * w] && G[i + (size_t)i * w] > 0.0)
            R[i + (size_t)i * w] = std::sqrt(piv);
        else {
            bad[i] = 1;
            R[i + (size_t)i * w] = 1.0;
            (*n_bad)++;
        }
    }
    const std::vector<double> Rinv = upper_inverse(R, w);
    double *W = V->d + k_old;
    RAILS_TRY(rails_small_reserve(c, (size_t)w * w * sizeof(double)));
    RAILS_TRY(upload_small(c, Rinv, c->small));
    RAILS_TRY(rails_panel_gemm_dev(c, 1.0, W, V->ld, w, c->small, w, 0.0, W, V->ld, V->m));
    // norms of the residual columns (one block Gram), then scale them to unit length
    RAILS_TRY(rails_gram_dev(c, W, V->ld, W, V->ld, V->m, w, w, c->small));
    RAILS_TRY(rails_allreduce_dev(c, c->small, (size_t)w * w));
    std::vector<double> G2;
    RAILS_TRY(sync_small_to_host(c, (size_t)w * w, G2));
    for (int i = 0; i < w; ++i) {
        if (!bad[i]) continue;
        double n2 = G2[i + (size_t)i * w];
        if (n2 > 0.0 && std::isfinite(n2)) RAILS_TRY(rails_panel_scale(c, V, k_old + i, 1, 1.0 / std::sqrt(n2)));
    }
    return RAILS_OK;
}

// rails_orthogonalize (ns.q = 0) and rails_orthogonalize_deflated
int orthogonalize(rails_ctx *c, rails_panel *V, int k_old, int w, Nullspace const &ns, int method, int *used)
{
    if (used) *used = 0;
    if (w == 0) return RAILS_OK;
    if (method == 1 || w > 256) {
        if (used) *used = 1;
        c->n_orth_columnwise++;
        return columnwise(c, V, k_old, k_old + w, ns);
    }
    double *W = V->d + k_old;
    for (int round = 0; round < 2; ++round) {
        bool repaired = false;
        // block CGS2 against the nullspace and the old columns
        for (int pass = 0; pass < 2; ++pass) RAILS_TRY(project_block(c, V, k_old, w, ns));
        // CholQR2 inside the block
        RAILS_TRY(rails_small_reserve(c, (size_t)w * w * sizeof(double)));
        for (int pass = 0; pass < 2; ++pass) {
            RAILS_TRY(rails_gram_dev(c, W, V->ld, W, V->ld, V->m, w, w, c->small));
            RAILS_TRY(rails_allreduce_dev(c, c->small, (size_t)w * w));
            std::vector<double> G;
            RAILS_TRY(sync_small_to_host(c, (size_t)w * w, G));
            double dmax = 0.0;
            for (int i = 0; i < w; ++i) dmax = std::max(dmax, G[i + (size_t)i * w]);
            std::vector<double> R = G;
            int info = 0;
            rails_dpotrf('U', w, R.data(), w, &info);
            bool bad = (info != 0) || !(dmax > 0.0);
            if (!bad) {
                // a diagonal of R much smaller than the column norm means the column lies (numerically)
                // in the span of the others: CholQR would amplify rounding by (norm/r_ii)^2
                for (int i = 0; i < w; ++i) {
                    double rii = R[i + (size_t)i * w];
                    double nrm = std::sqrt(G[i + (size_t)i * w]);
                    if (!(rii > 1e-5 * nrm)) bad = true;
                }
            }
            if (bad) {
                static const int repair_env = [] {
                    const char *e = getenv("RAILS_ORTH_REPAIR");
                    return e ? atoi(e) : 1;
                }();
                if (round == 0 && repair_env && dmax > 0.0) {
                    int n_bad = 0;
                    RAILS_TRY(repair_block(c, V, k_old, w, G, &n_bad));
                    if (n_bad > 0) {
                        c->n_orth_repair++;
                        repaired = true;
                        break; // run the block procedure once more on the repaired block
                    }
                }
                if (method == 2) {
                    rails_set_error("rails_orthogonalize: block Gram matrix is rank deficient (dpotrf info %d)", info);
                    return RAILS_ELAPACK;
                }
                if (used) *used = 1;
                c->n_orth_columnwise++;
                return columnwise_in_block(c, V, k_old, w, ns);
            }
            const std::vector<double> Rinv = upper_inverse(R, w);
            RAILS_TRY(upload_small(c, Rinv, c->small));
            RAILS_TRY(rails_panel_gemm_dev(c, 1.0, W, V->ld, w, c->small, w, 0.0, W, V->ld, V->m)); // in place, row-local
        }
        if (!repaired) {
            if (used) *used = round == 0 ? 2 : 3;
            c->n_orth_block++;
            return RAILS_OK;
        }
    }
    if (used) *used = 1; // not reached: the second round either succeeds or takes the column-wise path
    return columnwise_in_block(c, V, k_old, w, ns);
}

// ---- rank-revealing range basis (rails_orthogonalize_range) --------------------------------------------------------------------------
// The reference's Morth for a start space that may be rank deficient (matlab/RAILSsolver.m:567-580): every column is scaled to unit
// length, projected twice against the nullspace and everything kept before it, and dropped when less than `tol` of it survives.  Here in
// blocks of at most RANGE_BLOCK columns, with the block operations of orthogonalize() above and no per-column pass:
//
//   pre-scale   column norms of the block (rails_panel_colnorms2), W <- W diag(1 / norm), packed to the left at k_cur (zero columns go)
//   project     twice W -= [N V(:, 0:k_cur)] ([N V]'W)                                                        (project_block)
//   decide      G = W'W; Cholesky with the dependent pivots skipped (as repair_block); W <- W R^-1
//   measure     a column skipped at the pivot test is not dropped yet: the Gram matrix cannot decide a residual of 1e-8, which is 1e-16 of
//               its diagonal.  After W R^-1 such a column IS its residual against the independent columns before it; its norm (a second
//               rails_panel_colnorms2) is the fraction of the unit length that survived.  Below tol: dropped.  Above: scaled back to unit
//               length and the block goes round once more (the repair idea), which takes the column as an ordinary one.
//   second CholQR round on what remains (after one more projection when the first round left a column less than 1e-2 of its length:
//   its rounding error along [N V] was magnified by the inverse of that fraction).
//
// Every product that moves columns is ONE launch of k_panel_gemm (at most 256 output columns) reading and writing overlapping windows
// of V: see apply_in_place.
constexpr int RANGE_BLOCK = 128;

// V[:, dst : dst + r) <- V[:, src : src + k) C (C host, k x r column-major, ld k), dst <= src, r <= 256, the windows may overlap.
// In place this is safe only because a wave of k_panel_gemm reads all k columns of its 16 rows before it stores anything, and no other
// wave touches those rows (dense_panel_gemm.inc: the accumulators are complete when the store loop starts; beta = 0 reads no Y).  So
// the product stays inside one launch -- r <= 256 -- and goes through the internal entry point: rails_panel_gemm refuses partially
// overlapping windows, rightly, for callers that cannot know this.
int apply_in_place(rails_ctx *c, rails_panel *V, int src, int k, const std::vector<double> &C, int r, int dst)
{
    if (r == 0 || k == 0) return RAILS_OK;
    const size_t bytes = (size_t)k * r * sizeof(double);
    RAILS_TRY(rails_small_reserve(c, bytes));
    RAILS_TRY(rails_pinned_begin_write(c, bytes)); // the upload does not make the host wait (as in rails_panel_gemm)
    memcpy(c->pinned, C.data(), bytes);
    RAILS_HIP_CHECK(hipMemcpyAsync(c->small, c->pinned, bytes, hipMemcpyHostToDevice, c->stream));
    RAILS_TRY(rails_pinned_end_write(c));
    c->n_orth_range_passes++;
    return rails_panel_gemm_dev(c, 1.0, V->d + src, V->ld, k, c->small, r, 0.0, V->d + dst, V->ld, V->m);
}

// Cholesky of the n x n Gram matrix G with the dependent pivots skipped, as in repair_block: r_ii = 1 and row i of R zero beyond the
// diagonal for a column i that keeps at most 1e-5 of its length against the independent columns before it (pivot <= 1e-10 G_ii), or
// that has lost that much to the projection already (G_ii <= 1e-10: the column had unit length before it).  Returns R^-1; min_kept is
// the smallest fraction an independent column keeps of the length it came with.
std::vector<double> skipping_cholesky_inverse(const std::vector<double> &G, int n, std::vector<char> &grey, double *min_kept)
{
    std::vector<double> R((size_t)n * n, 0.0);
    grey.assign(n, 0);
    *min_kept = 1.0;
    for (int i = 0; i < n; ++i) {
        const double gii = G[i + (size_t)i * n];
        double piv = gii;
        for (int j = 0; j < i; ++j) {
            if (grey[j]) continue;
            double s = G[j + (size_t)i * n];
            for (int l = 0; l < j; ++l)
                if (!grey[l]) s -= R[l + (size_t)j * n] * R[l + (size_t)i * n];
            s /= R[j + (size_t)j * n];
            R[j + (size_t)i * n] = s;
            piv -= s * s;
        }
        if (piv > 1e-10 * gii && gii > 1e-10 && std::isfinite(gii)) {
            R[i + (size_t)i * n] = std::sqrt(piv);
            *min_kept = std::min(*min_kept, std::sqrt(piv));
        } else {
            grey[i] = 1;
            R[i + (size_t)i * n] = 1.0;
            for (int j = 0; j < i; ++j)
                if (!std::isfinite(R[j + (size_t)i * n])) R[j + (size_t)i * n] = 0.0;
        }
    }
    return upper_inverse(R, n);
}

int gram_to_host(rails_ctx *c, rails_panel *V, int c0, int n, std::vector<double> &G)
{
    RAILS_TRY(rails_small_reserve(c, (size_t)n * n * sizeof(double)));
    RAILS_TRY(rails_gram_dev(c, V->d + c0, V->ld, V->d + c0, V->ld, V->m, n, n, c->small));
    RAILS_TRY(rails_allreduce_dev(c, c->small, (size_t)n * n));
    c->n_orth_range_passes++;
    c->n_orth_range_syncs++;
    return sync_small_to_host(c, (size_t)n * n, G);
}

// One block: the wb columns from column src on become n <= wb orthonormal columns at k_cur <= src; idx receives their positions in the
// block.  What lies between k_cur + n and src + wb is left as it is (the caller clears the tail once).
int range_block(rails_ctx *c, rails_panel *V, int k_cur, int src, int wb, Nullspace const &ns, double tol, int *n_out, std::vector<int> &idx)
{
    std::vector<double> n2(wb);
    RAILS_TRY(rails_panel_colnorms2(c, V, src, wb, n2.data()));
    c->n_orth_range_passes++;
    c->n_orth_range_syncs++;
    idx.clear();
    for (int i = 0; i < wb; ++i) {
        if (n2[i] > 0.0 && std::isfinite(n2[i]))
            idx.push_back(i);
        else if (n2[i] != 0.0) // not finite: a zero coefficient does not silence such a column in the product below
            RAILS_TRY(rails_panel_fill(c, V, src + i, 1, 0.0));
    }
    int n = (int)idx.size();
    std::vector<double> C((size_t)wb * n, 0.0);
    for (int j = 0; j < n; ++j) C[idx[j] + (size_t)j * wb] = 1.0 / std::sqrt(n2[idx[j]]);
    RAILS_TRY(apply_in_place(c, V, src, wb, C, n, k_cur));
    std::vector<double> kept_of_unit(n, 1.0); // the fraction of its unit length each column still stands for
    int project = 2, clean_rounds = 0;
    // a round with grey columns multiplies the fraction of each by at most 1e-5 or drops it, so the rounds are bounded by tol
    for (int round = 0; n > 0 && clean_rounds < 2; ++round) {
        if (round > 40) {
            rails_set_error("rails_orthogonalize_range: the rank decision of a block did not settle");
            return RAILS_ELAPACK;
        }
        for (int pass = 0; pass < project; ++pass) {
            RAILS_TRY(project_block(c, V, k_cur, n, ns));
            if (ns.q + k_cur > 0) c->n_orth_range_passes += 2;
        }
        std::vector<double> G;
        RAILS_TRY(gram_to_host(c, V, k_cur, n, G));
        std::vector<char> grey;
        double min_kept = 1.0;
        const std::vector<double> Rinv = skipping_cholesky_inverse(G, n, grey, &min_kept);
        RAILS_TRY(apply_in_place(c, V, k_cur, n, Rinv, n, k_cur));
        int n_grey = 0;
        for (int i = 0; i < n; ++i) n_grey += grey[i];
        if (n_grey == 0) {
            ++clean_rounds;
            project = min_kept < 1e-2 ? 1 : 0;
            continue;
        }
        // second stage of the rank decision: the grey columns now hold their residuals
        n2.assign(n, 0.0);
        RAILS_TRY(rails_panel_colnorms2(c, V, k_cur, n, n2.data()));
        c->n_orth_range_passes++;
        c->n_orth_range_syncs++;
        std::vector<int> stay;
        std::vector<double> scale;
        for (int i = 0; i < n; ++i) {
            if (!grey[i]) {
                stay.push_back(i);
                scale.push_back(1.0);
                continue;
            }
            const double res = std::sqrt(n2[i]);
            if (!std::isfinite(res)) RAILS_TRY(rails_panel_fill(c, V, k_cur + i, 1, 0.0)); // (as above)
            if (!(res > 0.0) || !std::isfinite(res) || !(kept_of_unit[i] * res >= tol)) continue;
            kept_of_unit[i] *= res;
            stay.push_back(i);
            scale.push_back(1.0 / res);
        }
        const int n_new = (int)stay.size();
        std::vector<double> S((size_t)n * n_new, 0.0);
        std::vector<int> idx_new(n_new);
        std::vector<double> kept_new(n_new);
        for (int j = 0; j < n_new; ++j) {
            S[stay[j] + (size_t)j * n] = scale[j];
            idx_new[j] = idx[stay[j]];
            kept_new[j] = kept_of_unit[stay[j]];
        }
        RAILS_TRY(apply_in_place(c, V, k_cur, n, S, n_new, k_cur));
        idx.swap(idx_new);
        kept_of_unit.swap(kept_new);
        n = n_new;
        project = 2;
        clean_rounds = 0;
    }
    idx.resize(n);
    *n_out = n;
    return RAILS_OK;
}

int orthogonalize_range(rails_ctx *c, rails_panel *V, int k_old, int w, Nullspace const &ns, double tol, int *kept, int32_t *kept_idx)
{
    c->n_orth_range++;
    int k_cur = k_old;
    std::vector<int> idx;
    for (int b0 = 0; b0 < w; b0 += RANGE_BLOCK) {
        const int wb = std::min(RANGE_BLOCK, w - b0);
        int n = 0;
        RAILS_TRY(range_block(c, V, k_cur, k_old + b0, wb, ns, tol, &n, idx));
        if (kept_idx)
            for (int j = 0; j < n; ++j) kept_idx[k_cur - k_old + j] = (int32_t)(b0 + idx[j]);
        k_cur += n;
    }
    *kept = k_cur - k_old;
    if (k_cur < k_old + w) RAILS_TRY(rails_panel_fill(c, V, k_cur, k_old + w - k_cur, 0.0));
    return RAILS_OK;
}

} // namespace

extern "C" int rails_orthogonalize_range(rails_ctx *c, rails_panel *V, int k_old, int w, const rails_panel *N, int nc0, int q, double tol,
                                         int *kept, int32_t *kept_idx)
{
    if (c) hipSetDevice(c->device);
    RAILS_REQUIRE(c && V && kept && (q == 0 || N), "rails_orthogonalize_range: null argument");
    RAILS_REQUIRE(k_old >= 0 && w >= 0 && k_old + w <= V->cap, "rails_orthogonalize_range: columns [%d,%d) outside capacity %d", k_old, k_old + w,
                  V->cap);
    RAILS_REQUIRE(q >= 0 && (q == 0 || (nc0 >= 0 && nc0 + q <= N->cap)), "rails_orthogonalize_range: nullspace columns [%d,%d) outside capacity %d",
                  nc0, nc0 + q, q ? N->cap : 0);
    RAILS_REQUIRE(q == 0 || N->m == V->m, "rails_orthogonalize_range: the nullspace has %lld rows, V %lld", q ? (long long)N->m : 0LL,
                  (long long)V->m);
    RAILS_REQUIRE(q == 0 || (N != V && N->d != V->d), "rails_orthogonalize_range: the nullspace must be a panel of its own");
    *kept = 0;
    if (w == 0) return RAILS_OK;
    Nullspace ns;
    ns.N = N;
    ns.c0 = nc0;
    ns.q = q;
    return orthogonalize_range(c, V, k_old, w, ns, tol > 0.0 ? tol : 1e-8, kept, kept_idx);
}

extern "C" int rails_orthogonalize(rails_ctx *c, rails_panel *V, int k_old, int w, int method, int *used)
{
    if (c) hipSetDevice(c->device); // allocations and launches go to the context's device whatever the caller's current device is
    RAILS_REQUIRE(c && V, "rails_orthogonalize: null argument");
    RAILS_REQUIRE(k_old >= 0 && w >= 0 && k_old + w <= V->cap, "rails_orthogonalize: columns [%d,%d) outside capacity %d", k_old,
                  k_old + w, V->cap);
    RAILS_REQUIRE(method >= 0 && method <= 2, "rails_orthogonalize: bad method %d", method);
    return orthogonalize(c, V, k_old, w, Nullspace(), method, used);
}

extern "C" int rails_orthogonalize_deflated(rails_ctx *c, rails_panel *V, int k_old, int w, const rails_panel *N, int nc0, int q, int method,
                                            int *used)
{
    if (c) hipSetDevice(c->device);
    RAILS_REQUIRE(c && V && (q == 0 || N), "rails_orthogonalize_deflated: null argument");
    RAILS_REQUIRE(k_old >= 0 && w >= 0 && k_old + w <= V->cap, "rails_orthogonalize_deflated: columns [%d,%d) outside capacity %d", k_old,
                  k_old + w, V->cap);
    RAILS_REQUIRE(q >= 0 && (q == 0 || (nc0 >= 0 && nc0 + q <= N->cap)), "rails_orthogonalize_deflated: nullspace columns [%d,%d) outside capacity %d",
                  nc0, nc0 + q, q ? N->cap : 0);
    RAILS_REQUIRE(q == 0 || N->m == V->m, "rails_orthogonalize_deflated: the nullspace has %lld rows, V %lld", q ? (long long)N->m : 0LL,
                  (long long)V->m);
    RAILS_REQUIRE(q == 0 || N != V, "rails_orthogonalize_deflated: the nullspace must be a panel of its own");
    RAILS_REQUIRE(method >= 0 && method <= 2, "rails_orthogonalize_deflated: bad method %d", method);
    Nullspace ns;
    ns.N = N;
    ns.c0 = nc0;
    ns.q = q;
    return orthogonalize(c, V, k_old, w, ns, method, used);
}
