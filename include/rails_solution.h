/* ============================================================================
 * rails_solution.h -- C ABI of the solution object: X = U S U' with U a device panel (m x k, need not be orthonormal) and S a small
 * symmetric host matrix (k x k).  What a user does WITH the low-rank solution (V, T) of the solver -- the second half of the
 * reference's driver (src/main.cpp:140-170: SetSolution, leading eigenpairs, trace, explained variance) and of its Schur operator
 * (src/SchurOperator.cpp:191-342: Apply with a solution, Trace) -- without forming X and without taking V off the device.
 * Return conventions as in rails_hip.h.  Everything that reduces over rows goes through rails_gram (all-reduced over the ranks of a
 * row partition); variance, apply's update and block's gather are row-local.
 * ==========================================================================*/
#ifndef RAILS_SOLUTION_H
#define RAILS_SOLUTION_H

#include "rails_solver.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rails_solution rails_solution;

/* Rows moved between panels of different row counts: Y row i <- X row idx[i] (scatter == 0) or Y row idx[i] <- X row i (scatter != 0) for
 * i < n, columns [xc0, xc0+nc) to [yc0, yc0+nc).  idx on the HOST, checked against the row counts.  (rails_panel_permute_rows is the form
 * for permutations of one row set with the indices already on the device.)  Asynchronous. */
int rails_panel_move_rows(rails_ctx *ctx, const rails_panel *X, int xc0, int nc, const int32_t *idx_host, int64_t n, int scatter, rails_panel *Y, int yc0);

/* Out[:, oc0] = diag(U[:, c0:c0+k] S U[:, c0:c0+k]'), i.e. out[i] = sum_{j,l} U[i,j] S[j,l] U[i,l] for every local row: one pass over U on the
 * fp64 MFMA path, no m x k temporary (rails_amd/csrc/solution.hip).  S host column-major k x k, leading dimension lds (need not be
 * symmetric: the form is that of S as given).  k <= 512.  Out may be U's panel when column oc0 lies outside the window.  Asynchronous. */
int rails_panel_rowquad(rails_ctx *ctx, const rails_panel *U, int c0, int k, const double *S_host, int lds, rails_panel *Out, int oc0);
/* What the context's last rails_panel_rowquad launched: *nslices slices of S (0 for k = 0, for a panel without rows, or before any call) and, for
 * the first min(cap, *nslices) of them, the template parameter TR of k_panel_rowquad<TR> (2, 4, 8, 12 or 16 column tiles of 16). */
int rails_panel_rowquad_last_plan(const rails_ctx *ctx, int *nslices, int *tr, int cap);
/* out[i] = U[ia[i], c0:c0+k] S U[ib[i], c0:c0+k]'  for i < n  ( = X[ia[i], ib[i]] ).  ia, ib: n LOCAL row indices on the HOST, checked against
 * U's rows before anything is queued; either may be NULL = the identity (then n <= rows of U).  Out has at least n rows; rows from n on
 * and every other column are left alone.  S as in rails_panel_rowquad (as given, need not be symmetric), k <= 512.  The kernel is
 * rails_panel_rowquad's body on gathered rows -- one pass, no n x k temporary, the same slices (reported through
 * rails_panel_rowquad_last_plan) and the same fixed summation order: a pair's bits do not depend on its place i or on n, and with both
 * indices the identity they are rails_panel_rowquad's.  Out may be U's panel when column oc0 lies outside the window.  n == 0 or a panel
 * without rows: nothing is queued; k == 0: zeros in the n rows.  Asynchronous. */
int rails_panel_rowpair(rails_ctx *ctx, const rails_panel *U, int c0, int k, const double *S_host, int lds, const int32_t *ia, const int32_t *ib, int64_t n,
                        rails_panel *Out, int oc0);
/* host[0..n) summed over the ranks of the partition with the context's all-reduce (the one rails_gram uses).  One rank with neither a hook
 * nor a communicator: returns at once, nothing queued.  Synchronises otherwise. */
int rails_allreduce_host(rails_ctx *ctx, double *host, int64_t n);
/* Covariances to correlations: Out[i, oc0+j] /= sqrt(Var[i, vc]) sqrt(rv[j]) for j < q <= 64; 0 wherever either variance is not > 0; exactly 1
 * where i == rows[j] (an unknown with itself) and its variance is > 0.  rv, rows: q host entries (rows[j] = -1: not a local row).  Asynchronous. */
int rails_panel_corr_scale(rails_ctx *ctx, rails_panel *Out, int oc0, int q, const rails_panel *Var, int vc, const double *rv_host, const int32_t *rows_host);

/* U = columns [c0, c0+k) of the panel; copy != 0: the object keeps a device copy of them, copy == 0: it borrows the panel (the caller
 * keeps it alive and unchanged).  S_host column-major k x k, leading dimension lds; it is copied and symmetrised ((S + S')/2). */
int rails_solution_create(rails_ctx *ctx, const rails_panel *U, int c0, int k, const double *S_host, int lds, int copy, rails_solution **out);
/* the V panel and the T the last rails_solver_solve left (device copy of V: no host round trip; with "mass_orthogonalisation" V is
 * M-orthonormal and X = V T V' all the same) */
int rails_solution_from_solver(rails_solver *s, rails_solution **out);
int rails_solution_destroy(rails_solution *sol);
int rails_solution_rank(const rails_solution *sol);     /* k */
int64_t rails_solution_rows(const rails_solution *sol); /* local rows */
/* the object's panel, first column and S (column-major k x k, leading dimension k; owned by the object) */
const rails_panel *rails_solution_panel(const rails_solution *sol, int *c0);
const double *rails_solution_small(const rails_solution *sol);

/* out[:, c0] = diag(X) (rails_panel_rowquad) */
int rails_solution_variance(rails_solution *sol, rails_panel *out, int c0);
/* tr(X) = tr(S U'U): one rails_gram.  The reference's SchurOperator::Trace (src/SchurOperator.cpp:322-342) for a lifted solution. */
int rails_solution_trace(rails_solution *sol, double *tr);
/* Y[:, yc0:yc0+nc] = X W[:, c0:c0+nc] = U (S (U'W)).  Y and W must not be the object's panel. */
int rails_solution_apply(rails_solution *sol, const rails_panel *W, int c0, int nc, rails_panel *Y, int yc0);
/* The `want` eigenpairs of largest modulus of X, exact for the low-rank form (the reference iterates, src/main.cpp:150-160): Q =
 * orthonormal basis of U (rails_orthogonalize), R = Q'U, the symmetric eigenproblem of R S R' on the host, vectors = Q Z.  Sorted by
 * decreasing modulus; pairs with |lambda| <= tol * max|lambda| are dropped; *found = pairs returned.  want <= 0: all k (rank
 * truncation of a solution).  values has room for min(want, k) (k for want <= 0) doubles; vectors (may be NULL) gets columns [0, *found)
 * and needs that capacity. */
int rails_solution_eigs(rails_solution *sol, int want, double tol, double *values, rails_panel *vectors, int *found);
/* out (nr x nc, column-major, leading dimension ld) = X[rows, cols] (local row indices): the rows are gathered on the device, the small
 * product is done on the host.  For spot checks and sections. */
int rails_solution_block(rails_solution *sol, const int32_t *rows, int nr, const int32_t *cols, int nc, double *out, int ld);
/* out[i, c0] = X[ia[i], ib[i]] for i < n (rails_panel_rowpair: LOCAL indices on the host, either may be NULL = the identity; out has at least
 * n rows).  The covariance of pairs of unknowns at scale: the eddy-flux field of two variables per cell, a section's neighbour covariances. */
int rails_solution_pairs(rails_solution *sol, const int32_t *ia, const int32_t *ib, int64_t n, rails_panel *out, int c0);
/* Out[:, oc0+j] = X[:, r_j] for q reference unknowns (correlation == 0), or X[i, r_j] / sqrt(X[i,i] X[r_j,r_j]) (correlation != 0; 0 wherever
 * either variance is not > 0, exactly 1 at the reference unknown's own row when its variance is > 0).  rows[j]: LOCAL index of reference
 * unknown j on the rank that owns it, -1 on every other rank (one GPU: all >= 0).  q <= 64.  var_col >= 0: that column of Out (outside
 * [oc0, oc0+q)) also receives diag(X).  A composition: the q rows are gathered (rails_panel_move_rows), G = S U[r,:]' (k x q) is formed on the
 * host and summed over the ranks together with an owner count per reference unknown -- one that no rank or several ranks claim is refused
 * with RAILS_EINVAL on every rank alike, nothing written -- then Out = U G (rails_panel_gemm); correlations add rails_solution_variance,
 * the q reference variances read from their owners' variance column (summed the same way) and rails_panel_corr_scale.  Synchronises. */
int rails_solution_maps(rails_solution *sol, const int32_t *rows, int q, int correlation, rails_panel *Out, int oc0, int var_col);

#ifdef __cplusplus
}
#endif
#endif
