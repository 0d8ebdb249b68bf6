/* ============================================================================
 * rails_hip.h -- C ABI of librails_hip.so: the MI355X (gfx950) back end of the
 * RAILS inner loop.
 *
 * This is the drop-in boundary.  The reference (Sbte/RAILS) has no FFI: its
 * plug-in seam is C++ template duck typing, Solver<Matrix, MultiVector,
 * DenseMatrix> (src/LyapunovSolverDecl.hpp:9-51).  The header-only wrappers in
 * rails_amd/include/rails/ (HipOperatorWrapper, HipMultiVectorWrapper,
 * HostDenseMatrix) satisfy that contract and are implemented purely in terms of
 * the entry points below, so this C ABI is exactly what a binding for the hot
 * path binds.  Each entry point cites the reference interface it replaces.
 *
 * Conventions
 *   - every function returns 0 on success, a negative RAILS_E* code otherwise
 *     (never throws); rails_last_error() gives the message of the calling
 *     thread's last failure.  This mirrors the reference's "no exceptions, int
 *     codes, message on stderr" behaviour (src/StlWrapper.cpp:173-179).
 *   - host matrices cross the boundary COLUMN-MAJOR with a leading dimension,
 *     like the reference's StlWrapper / DenseMatrix storage
 *     (src/StlVector.cpp:47-50, operator double* at src/StlWrapper.cpp:201).
 *   - device panels are ROW-MAJOR m_local x ld (ld = padded column capacity):
 *     one sparse nonzero gathers one contiguous row segment, reductions run
 *     down the slow index, and view/resize/push_back are O(1) column-window
 *     changes.  The solver never sees MultiVector memory
 *     (src/LyapunovSolver.hpp uses double* only from DenseMatrix, :357,:458),
 *     so the layout is free.
 *   - the library owns device buffers until *_destroy; the caller owns host
 *     buffers.  Calls that return host values are synchronisation points;
 *     everything else is asynchronous on the context's stream.
 *   - row-partitioned multi-GPU runs: every rank holds a contiguous block of
 *     rows of A, V, AV, B; small (k x k, p x k) objects are replicated.  All
 *     reductions over rows go through the all-reduce hook (sum of doubles).
 * ==========================================================================*/
#ifndef RAILS_HIP_H
#define RAILS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RAILS_OK 0
#define RAILS_EINVAL -1   /* bad argument / shape mismatch                      */
#define RAILS_EHIP -2     /* a HIP runtime call failed                          */
#define RAILS_ENOMEM -3   /* device or host allocation failed                   */
#define RAILS_ELAPACK -4  /* host LAPACK missing or returned an error           */
#define RAILS_ECOMM -5    /* all-reduce / halo hook failed                      */
#define RAILS_ENODEV -6   /* no usable gfx950 device                            */

typedef struct rails_ctx rails_ctx;     /* device, stream, workspaces, RNG, collectives */
typedef struct rails_csr rails_csr;     /* device CSR operator (the Matrix role)        */
typedef struct rails_panel rails_panel; /* device row-partitioned panel (MultiVector)   */

const char *rails_last_error(void);
const char *rails_version(void);

/* ---------------------------------------------------------------- context --- */

/* device: HIP device ordinal.  stream: a hipStream_t to run on (e.g. the caller's
 * torch stream), or NULL to let the library create its own. */
int rails_ctx_create(int device, void *stream, rails_ctx **out);
int rails_ctx_destroy(rails_ctx *ctx);
int rails_ctx_sync(rails_ctx *ctx);
void *rails_ctx_stream(rails_ctx *ctx);
/* compute units of the context's device (the one-pass update + second projection launches min(row tiles, 2 x this) workgroups); 0 for NULL */
int rails_ctx_num_cu(const rails_ctx *ctx);
/* call counters of this context as a JSON object (block vs column-wise orthogonalisations, SpMM kernel choice, ...) */
int rails_ctx_stats(rails_ctx *ctx, char *buf, int cap);
/* Busy meter: with on != 0 every kernel launch of this context is bracketed by a pair of events, read at the next synchronisation of
 * its stream; "gpu_busy_ms" of rails_ctx_stats is the sum: the time the GPU was at work for this context.  Costs a few microseconds
 * per launch: for measurement runs. */
int rails_ctx_set_meter(rails_ctx *ctx, int on);

/* Counter-based RNG: value = f(seed, stream id, GLOBAL row, column); every random
 * fill consumes one stream id.  Replaces StlWrapper::random's std::rand()-seeded
 * generator (src/StlWrapper.cpp:414-423) by one that is identical on CPU and GPU
 * and independent of the row partition. */
int rails_ctx_set_seed(rails_ctx *ctx, uint64_t seed, uint64_t first_stream);
/* Current generator position (seed, id of the next stream): lets a caller repeat a draw. */
int rails_ctx_rng_state(rails_ctx *ctx, uint64_t *seed, uint64_t *next_stream);

/* Row partition of this rank: local rows are global rows [row0, row0 + m_local). */
int rails_ctx_set_partition(rails_ctx *ctx, int rank, int nranks, int64_t row0, int64_t m_global);

/* Sum-all-reduce hook over the ranks, in place on a DEVICE buffer of n doubles,
 * ordered on `stream`.  With nranks == 1 no hook is needed.  This is the one
 * collective of the path: Epetra hides it in Multiply('T','N')/Norm2
 * (src/Epetra_MultiVectorWrapper.cpp:238,312,431). */
typedef int (*rails_allreduce_fn)(void *user, double *dev_buf, size_t n, void *stream);
int rails_ctx_set_allreduce(rails_ctx *ctx, rails_allreduce_fn fn, void *user);

/* The same all-reduce (and the ghost-row exchange of rails_spmm) done by the library itself over RCCL -- xGMI inside a node --
 * on the context's stream, with no hook and no Python in the loop.  Either let the library make the communicator: rank 0 calls
 * rails_rccl_unique_id, the application hands the RAILS_RCCL_ID_BYTES bytes to every rank (any way it likes: MPI, files, a
 * torch.distributed broadcast), then EVERY rank calls rails_ctx_init_rccl (collective; device = the context's); or adopt one
 * the application already has (an ncclComm_t; the caller keeps ownership).  A hook installed with rails_ctx_set_allreduce
 * takes precedence.  librccl.so.1 is loaded at run time (RAILS_RCCL_LIB overrides the name). */
#define RAILS_RCCL_ID_BYTES 128
int rails_rccl_unique_id(void *id_out);
int rails_ctx_init_rccl(rails_ctx *ctx, const void *id, int nranks, int rank);
int rails_ctx_set_rccl(rails_ctx *ctx, void *nccl_comm);
int rails_ctx_rccl_size(const rails_ctx *ctx); /* ranks of the communicator, 0 without one */

/* Halo hook for the row-partitioned operator apply: given the packed rows this rank
 * must send (send_buf, concatenated per destination rank as described by the counts
 * passed to rails_csr_set_halo) fill recv_buf with the ghost rows, on `stream`.
 * Replaces the import inside Epetra_CrsMatrix::Apply (src/Epetra_OperatorWrapper.cpp:87). */
typedef int (*rails_halo_fn)(void *user, const double *send_buf, double *recv_buf, int ncols, void *stream);

/* ------------------------------------------------------------ CSR operator --- */

/* Upload a local CSR block: m_local rows, column indices in [0, n_cols_ext) where
 * columns [0, m_local) are the local rows and [m_local, n_cols_ext) are ghost rows
 * (n_cols_ext == m_local on one GPU).  rowptr has m_local+1 entries.
 * Role: the Matrix template parameter (src/LyapunovSolverDecl.hpp:37,
 * Epetra_OperatorWrapper.cpp:75-91; StlWrapper.cpp:168-187 for the dense Stl form). */
int rails_csr_create(rails_ctx *ctx, int64_t m_local, int64_t n_cols_ext, const int64_t *rowptr,
                     const int32_t *col, const double *val, rails_csr **out);
/* An operator given by its action instead of a CSR block (composite operators such as the reference's Schur complement
 * A22 - A21 A11^-1 A12, src/SchurOperator.cpp:181-214; matrix-free operators): rails_spmm on the returned handle calls
 * fn(user, trans, X, xc0, nc, Y, yc0), which must set Y[:, yc0:yc0+nc] = op(A) X[:, xc0:xc0+nc] with the C-ABI panel functions on
 * the context's stream and return 0.  The handle takes the Matrix role everywhere a CSR handle does (single GPU). */
typedef int (*rails_apply_fn)(void *user, int trans, const rails_panel *X, int xc0, int nc, rails_panel *Y, int yc0);
int rails_csr_create_callback(rails_ctx *ctx, int64_t m_local, rails_apply_fn fn, void *user, rails_csr **out);
int rails_csr_destroy(rails_csr *A);
int64_t rails_csr_rows(const rails_csr *A);
int64_t rails_csr_nnz(const rails_csr *A);

/* Ghost-row plan for multi-GPU: send_rows[0..n_send) are LOCAL row indices to pack (in
 * the order the halo hook expects), n_ghost rows are received. */
int rails_csr_set_halo(rails_csr *A, int64_t n_send, const int64_t *send_rows, int64_t n_ghost,
                       rails_halo_fn fn, void *user);

/* Rows per neighbour rank of that plan: send_rows is grouped by destination rank (ranks ascending, send_counts[r] rows to rank r) and
 * the ghost rows by owning rank (recv_counts[r] from rank r).  With these and an RCCL communicator on the context the exchange
 * is one group of ncclSend / ncclRecv per product and rails_csr_set_halo may be called with fn = NULL. */
int rails_csr_set_halo_counts(rails_csr *A, int nranks, const int64_t *send_counts, const int64_t *recv_counts);

/* Y[:, yc0:yc0+nc] = op(A) * X[:, xc0:xc0+nc]; trans != 0 applies A^T (single GPU only).
 * Replaces `A_ * W` (src/LyapunovSolver.hpp:146).  X and Y must not alias. */
int rails_spmm(rails_ctx *ctx, rails_csr *A, int trans, const rails_panel *X, int xc0, int nc,
               rails_panel *Y, int yc0);

/* Kernel variant control for benchmarking and tests: 0 = auto, 1 = row-gather kernel (column chunking by the window
 * heuristic), 2 = LDS-staged footprint kernel, 3 = row-gather over the whole width, 4 / 5 = row-gather in 32 / 64 column
 * chunks inside one launch, 6 = LDS-staged footprint kernel with 16-column chunks (whole 128-B lines per staged row),
 * 7 = sweep kernel (banded patterns: X streamed once per XCD through LDS rings, partial sums in registers; fails when the
 * pattern or the column count does not fit), 8 = never the sweep kernel (auto otherwise). */
int rails_csr_set_variant(rails_csr *A, int variant);
/* Set-up for products of nc columns with A (trans != 0: with its transpose): builds now what the automatic kernel choice would
 * otherwise put off -- the sweep kernel's schedule (banded patterns, 64 to 256 columns) costs about a third of a second of host time per
 * million rows, a few hundred times what it saves one product, so without this call an operator only builds it after it has been asked for
 * RAILS_SWEEP_AFTER (default 16) products of that width.  *kernel_ready (may be null) = 1 when the sweep kernel will take them.  A
 * no-op for operators and widths the kernel does not apply to.  The reference has no counterpart: Epetra's FillComplete is the
 * nearest (set-up work of the matrix class before `A_ * W`, src/LyapunovSolver.hpp:146). */
int rails_csr_prepare(rails_ctx *ctx, rails_csr *A, int trans, int nc, int *kernel_ready);
/* Statistics of the sweep kernel's schedule for nc columns, once it has been built:
 * out[0] slot efficiency, [1] X rows staged per matrix row and chunk, [2] lock-step trips, [3] 1 if the schedule exists. */
int rails_csr_sweep_stats(rails_csr *A, int nc, double *out);
/* The LDS-staged footprint kernel's tile plan and its most recent launch (out has room for 16):
 * out[0] 1 once the plan has been looked at, [1] 1 if it was accepted, [2] 1 for boxes of a structured grid (0: runs of consecutive rows),
 * [3] tiles, [4] rows of the largest tile, [5] largest column footprint, [6] most LDS rows a footprint is spread over, [7] most nonzeros
 * of a row, [8] nonzeros per staged X row; the launch: [9] 0 none yet, 1 k_spmm_tiled, 2 k_spmm_tiled_pipe, 3 k_spmm_tiled_reg,
 * [10] columns per chunk KC, [11] register slots per row NNZ, [12] staging slots per thread NL, [13] 16-byte vectors per lane V2,
 * [14] chunks in flight NS (zeros where a kernel has no such parameter); [15] 0. */
int rails_csr_tile_stats(rails_csr *A, double *out);
/* The plane-sweep kernel's plan and its most recent launch on this operator (out has room for 16):
 * out[0] 1 once the plan has been looked at, [1] 1 if it was accepted (a complete 7- or 27-point grid stencil), [2] 1 for the 7-point form,
 * [3..5] the grid gx, gy, gz (of a z-slab: its own planes), [6], [7] the output planes [z_lo, z_hi) the plan covers (all of them, or a
 * z-slab's planes without ghost columns); the launch of k_spmm_planes<LPR, RW, WX, WY>: [8] lanes per row LPR (0: none yet), [9] rows per
 * wave RW, [10], [11] waves WX x WY, [12] planes per z segment, [13] z segments, [14] column chunks, [15] 1 if Y's rows took one 16-byte
 * store per lane (0: a window on an odd column, two 8-byte stores) + 2 if the launch was the interior planes of a row-partitioned product. */
int rails_csr_planes_stats(rails_csr *A, double *out);
/* A rectangular operator, n_rows x n_cols, all columns local: in rails_spmm X has n_cols rows and Y n_rows; no transposed apply, no
 * ghost rows.  Role: the off-diagonal blocks A12, A21 of the reference's Schur complement operator (src/SchurOperator.cpp:181-214). */
int rails_csr_create_rect(rails_ctx *ctx, int64_t n_rows, int64_t n_cols, const int64_t *rowptr, const int32_t *col, const double *val,
                          rails_csr **out);
/* name of the kernel the last rails_spmm on A launched */
const char *rails_csr_last_kernel(const rails_csr *A);

/* Host-side schedule of the sweep kernel (rails_amd/csrc/sweep_plan.h), exposed for tests and diagnostics: no device is
 * touched.  params = {waves, groups, rows per step, ring segments, parts, phases, segments being filled at any time, trips per
 * schedule entry (4 or 2; 0 = the library's choice)} (8 entries) or NULL for the kernel's own geometry.
 * info (iinfo has room for 16): iinfo[0..5] = params, [6] entries per step record, [7] lock-step trips, [8] nnz, [9] batches,
 * [10] entries in the busiest (wave, step), [11] slots per wave, [12] segments being filled, [13] trips per entry; dinfo[0] = slot efficiency
 * nnz / (slots x trips), dinfo[1] = X rows staged per matrix row and column chunk.  rails_sweep_plan_array lends the
 * arrays of the plan (which = 0 part_row0 i64, 1 sweep0 i64, 2 nsteps i32, 3 hdr_off i64, 4 batch_off i64, 5 flush_off i64,
 * 6 codes u32, 7 vals f64, 8 offs u16, 9 flush_rows i32); they live until rails_sweep_plan_destroy. */
/* ---- sparse triangular solves on device panels (rails_amd/csrc/sptrsv.hip) -----------------------------------------------------------
 * The A11 systems of the Schur-complement operator: the reference factorises A11 with Amesos KLU and solves on the host inside every
 * product (src/SchurOperator.cpp:171-176 set-up, :181-214 Apply); here a host factorisation's L and U are applied on the device by level
 * scheduling, so that the blocks of a product stay where the SpMM kernels left them.  A triangle comes in CSR (columns of a row in any
 * order); `lower` != 0: entries on or below the diagonal; `unit_diag` != 0: ones on the diagonal, not stored. */
typedef struct rails_sptrsv rails_sptrsv;
int rails_sptrsv_create(rails_ctx *ctx, int64_t n, const int64_t *rowptr, const int32_t *col, const double *val, int lower, int unit_diag,
                        rails_sptrsv **out);
void rails_sptrsv_destroy(rails_sptrsv *T);
int64_t rails_sptrsv_levels(const rails_sptrsv *T); /* number of levels of the dependency graph (diagnostics) */
/* X[:, c0:c0+nc] <- T^-1 X[:, c0:c0+nc] in place, queued on the context's stream */
int rails_sptrsv_solve(rails_ctx *ctx, const rails_sptrsv *T, rails_panel *X, int c0, int nc);
/* row permutations of a factorisation: Y row i <- X row perm[i] (scatter == 0) or Y row perm[i] <- X row i (scatter != 0); perm lives in
 * device memory (rails_index_upload / rails_index_free) */
int rails_panel_permute_rows(rails_ctx *ctx, const rails_panel *X, int xc0, int nc, const int32_t *perm_dev, int scatter, rails_panel *Y, int yc0);
int rails_index_upload(rails_ctx *ctx, const int32_t *host, int64_t n, int32_t **out_dev);
void rails_index_free(rails_ctx *ctx, int32_t *dev);

/* ---- sparse LU solve as a library object (rails_amd/csrc/splu.hip) --------------------------------------------------------------------
 * The operator A^-1 of RAILS' inverse and extended Krylov projections (matlab/RAILSsolver.m:7-24, opts.projection_method and
 * opts.Ainv) from the factors of a host LU, Pr A Pc = L U, as scipy's SuperLU gives them: Pr has ones at (perm_r[i], i), Pc at
 * (i, perm_c[i]); L and U in CSR, L unit lower (its diagonal may be stored, as ones, or left out), U upper with its diagonal.
 * rows (optional, m_sub distinct indices) restricts the operator to a subsystem, x -> (A^-1 E x)[rows] with E putting x on those rows
 * and zeros elsewhere: the inverse of a Schur complement from an LU of the full matrix (Sinv, matlab/RAILSschur.m:60-64).  rows = NULL:
 * the operator is A^-1 itself (m_sub is ignored).  The level analysis runs on the host, here.  Single GPU only. */
typedef struct rails_lu rails_lu;
int rails_lu_create(rails_ctx *ctx, int64_t n, const int64_t *L_rowptr, const int32_t *L_col, const double *L_val, const int64_t *U_rowptr,
                    const int32_t *U_col, const double *U_val, const int32_t *perm_r, const int32_t *perm_c, const int32_t *rows, int64_t m_sub,
                    rails_lu **out);
void rails_lu_destroy(rails_lu *lu);
/* Y[:, yc0:yc0+nc] = A^-1 X[:, xc0:xc0+nc] (trans != 0: A^-T), both panels of m_sub rows, out of place; X is left unchanged.  The
 * object owns its workspace and grows it only when a wider nc arrives. */
int rails_lu_solve(rails_ctx *ctx, rails_lu *lu, int trans, const rails_panel *X, int xc0, int nc, rails_panel *Y, int yc0);
/* info[0..3] levels of L, U, U', L'; [4] nnz of L below its diagonal; [5] nnz of U; [6] kernel launches of the last solve; [7] n;
 * [8] m_sub; [9] workspace columns.  Returns the number of entries written (at most cap), or a negative code. */
int rails_lu_stats(const rails_lu *lu, int64_t *info, int cap);
/* An operator handle whose rails_spmm is rails_lu_solve (both trans values): it takes the Matrix role wherever a CSR handle does
 * (HipOperatorWrapper, rails_solver_create, rails_solver_set_inverse).  The caller keeps the rails_lu alive while the handle is used. */
int rails_csr_create_lu(rails_ctx *ctx, rails_lu *lu, rails_csr **out);

/* ---- iterative solve as a library object (rails_amd/csrc/itsolve.hip, iter_setup.hip, iter_hierarchy.hip, iter_precond.h, iter_scalars.h) --------------------------------------------------
 * The same operator A^-1 without a factorisation: the reference asks for no more than an approximate inverse (matlab/RAILSsolver.m:19-23,
 * opts.Ainv: "This can be approximate"), and at the sizes where the fill of L and U rules a sparse LU out an iteration on the device is
 * the only A^-1 there is.  A is any square operator handle rails_spmm accepts (a CSR matrix, a callback operator such as the Schur
 * complement; a rectangular handle is refused); the caller keeps A and the rails_iter alive, as with rails_csr_create_lu.  method:
 * RAILS_ITER_CG for a definite A of either sign, RAILS_ITER_BICGSTAB (right-preconditioned) for a general one.  The Jacobi preconditioner
 * comes from diag_host (m entries, none zero); with diag_host = NULL from the CSR diagonal when A is a CSR matrix and every diagonal
 * entry is stored and nonzero; otherwise there is none.  Every column is a system of its own (start value zero, tolerance relative to
 * its own ||b||); all scalars stay on the device and the host reads one number back every `check_every` iterations.  No floating-point
 * atomics: two solves of the same input give the same bits, whatever check_every is.
 * On a row partition.  A context reduces when it has more than one rank, an all-reduce hook or an RCCL communicator.  On such a context
 * A may be a stored CSR row block with ghost columns whose halo plan is set (rails_csr_set_halo; "square" then means globally), the
 * inner products are summed over the ranks (an all-reduce of at most 64 doubles between the kernel that sums this rank's partial sums and
 * the kernel that computes the scalars), and every rank holds the same scalars, flags and counts bit for bit.  rails_iter_create,
 * rails_iter_set, rails_iter_solve and rails_iter_precondition are then collective calls: every rank makes them in the same order with
 * the same nc and settings.  rails_iter_create makes one all-reduce, through which the ranks agree on whether the Jacobi diagonal exists
 * (on every rank, or on none), on the sign of the diagonal (negative only when it is on every rank) and on the two Gershgorin bounds (the
 * largest).  The hook or the communicator has to be installed before the object is made: a context with more than one rank and neither
 * is refused (RAILS_EINVAL), since the first inner product would fail.  A transposed solve (trans != 0) on an operator with ghost rows is
 * refused with RAILS_EINVAL before any collective: the transposed product of a row block is single GPU.  A right-hand side that is not
 * finite on any rank gives RAILS_EINVAL on every rank.  On a context that does not reduce nothing of this runs.
 * Settings (rails_iter_set): "tolerance" 1e-10, "max_iterations" 1000, "jacobi" 1, "check_every" 8, "strict" 0, and those of the polynomial
 * preconditioner below: "poly_degree" 0, "poly_ratio" 10, "eig_max" 0, "poly_fused" 1; those of the multigrid preconditioner: "amg" 0,
 * "amg_degree" 1, "amg_ratio" 4, "amg_theta" 0.08, "amg_coarse" 256; block Jacobi: "block_jacobi" 0; block multigrid: "block_amg" 0.
 * Chebyshev polynomial preconditioner (CG only; rails_amd/csrc/cheb_coef.h): with "poly_degree" K in 1 .. 64 the
 * solve preconditions with z = p_K(G A) G r, K products with A in a row without an inner product, a scalar kernel or a read-back between
 * them; G is the Jacobi diagonal's inverse when Jacobi is in effect and otherwise +-I, the sign of the operator's diagonal.  The
 * polynomial is fitted to [hi / "poly_ratio", hi]; hi is a Gershgorin bound on the spectrum of G A taken at create time from the CSR
 * arrays a stored operator keeps on the host, or "eig_max" when that is above 0 (an operator without host arrays -- a callback, an LU
 * handle -- needs it).  For a stored CSR operator without ghost rows, of fewer than 2^24 rows and with work panels below 4 GiB each
 * product is fused with its recurrence update in one kernel ("poly_fused" 0: never); a row block with ghost rows (fewer than 2^24 of
 * them) takes the same kernel in a ghost-row form, behind a ghost-row exchange the object issues itself -- one exchange per product
 * either way, and no all-reduce inside the polynomial.  Degree 0, the default, is the solve without any
 * of this, bit for bit.  RAILS_EINVAL: a degree above 0 on a BiCGStab object, a degree outside 0 .. 64, a ratio of at most 1, and a
 * solve with a degree above 0 and no bound.
 * Smoothed-aggregation multigrid preconditioner (CG only, single GPU; rails_amd/csrc/amg_host.h): with "amg" 1
 * the solve preconditions with one V-cycle, z = M r: per level a Chebyshev smoother of degree "amg_degree" (1; 0 .. 8) in the
 * Jacobi-scaled level matrix on [hi / "amg_ratio", hi] ("amg_ratio" 4, above 1; hi the level's Gershgorin bound) before and, as its
 * adjoint, after the coarse correction, and the dense inverse of the last matrix at the bottom; M is symmetric and definite with the
 * operator's sign.  The hierarchy is built on the host from the CSR arrays of a stored square operator whose diagonal is stored, nonzero
 * and of one sign (strength threshold "amg_theta" 0.08, in [0, 1), halved per level; levels until at most "amg_coarse" 256 rows are
 * left, 1 .. 1024) by rails_iter_amg_setup, which the first solve or rails_iter_precondition with "amg" on calls when there is no
 * hierarchy; a changed "amg_theta" or "amg_coarse" drops it.  "poly_fused" 0 keeps the cycle off the fused kernels too.  "amg" 0, the
 * default, is the solve without any of this: the same kernels, bits and launch counts.  RAILS_EINVAL, before any device work: "amg" on
 * a BiCGStab object; together with a "poly_degree" above 0, in whichever order the two are set; a callback, LU or iterative-solve
 * operator (a sparse right-hand side or a rectangular handle is refused by rails_iter_create already); a context that reduces; 2^24 rows or more; and from the set-up a matrix with unsorted
 * or repeated columns in a row, a zero, missing or non-finite diagonal entry, one that is not definite, or one that does not coarsen
 * below 1025 rows (there is no huge dense block).
 * Block-Jacobi preconditioner (both methods, single GPU; rails_amd/csrc/block_jacobi_host.h): for an operator with b
 * unknowns per cell, G is the inverse of the b x b diagonal blocks instead of the inverse of the diagonal, 2 <= b <= 8 and b divides m.
 * rails_iter_block_jacobi installs the blocks -- given on the host, or taken from a block-CSR handle's host copy or from the CSR arrays
 * a stored handle keeps on the host -- inverts them on the host in long double (Gauss-Jordan with partial pivoting, rounded once) and
 * sets "block_jacobi" to 1; rails_iter_set(it, "block_jacobi", 0 | 1) toggles it.  With "block_jacobi" 1 the preconditioner in effect
 * is block Jacobi; otherwise "jacobi" decides, as before.  The passes that apply G walk block rows, z_i = sum_j G[i][j] r_j with one
 * fused multiply-add per j, j ascending; a transposed BiCGStab solve applies the transposed inverse blocks.  "block_jacobi" 0, the
 * default, is the solve without any of this: the same kernels, bits and launch counts.  RAILS_EINVAL, before any device work: b outside
 * 2 .. 8 or not dividing m; a block with a zero or non-finite pivot or a non-finite inverse (the message names the block); no blocks
 * given on a callback, LU or iterative-solve operator, or on a stored handle without host arrays; b different from a block-CSR
 * handle's block size; a context that reduces; "block_jacobi" 1 without blocks; and "block_jacobi" 1 together with a "poly_degree"
 * above 0 or "amg" 1, in whichever order they are set (one preconditioner at a time).  Not available: block Jacobi as the G of the
 * Chebyshev polynomial, and on a row partition.
 * Block multigrid preconditioner (CG only, single GPU, block-CSR handles only; rails_amd/csrc/block_amg_host.h):
 * with "block_amg" 1 the solve preconditions with one V-cycle of smoothed aggregation on the cells of a block-CSR operator: the cycle of
 * "amg" with G the inverses of the b x b diagonal blocks of every level matrix (block-CSR on every level, the same b), aggregation by
 * the Frobenius norms of the blocks, every unknown of a cell going to the same component of its aggregate.  "amg_degree", "amg_ratio",
 * "amg_theta" and "amg_coarse" keep their meaning, ranges and defaults and serve both multigrids; "poly_fused" 0 keeps this cycle off
 * its fused kernels too.  rails_iter_block_amg_setup builds the hierarchy; the first solve or rails_iter_precondition with "block_amg"
 * on calls it when there is none.  "block_amg" 0, the default, is the solve without any of this: the same kernels, bits and launch
 * counts.  RAILS_EINVAL, before any device work: a BiCGStab object; an operator that is not a block-CSR handle with a host copy;
 * "block_amg" 1 together with "block_jacobi" 1, "amg" 1 or a "poly_degree" above 0, in whichever order they are set (one
 * preconditioner at a time); a context that reduces; 2^24 rows or more; and from the set-up a block row without a stored diagonal
 * block, block columns of a block row that are not strictly increasing, a non-finite entry, a diagonal block whose scalar diagonal has
 * a zero or entries of both signs (or a sign that differs between blocks), a singular diagonal block (the block is named), a hierarchy
 * that does not coarsen below 1025 rows, and a last matrix that is not definite.
 * Outcomes: a zero right-hand-side column gives x = 0 after 0 iterations; a column that stops at max_iterations or breaks down (a
 * vanishing denominator; CG: p'Ap of the wrong sign, the operator is not definite) keeps its last iterate and is flagged, and the call
 * still returns RAILS_OK unless "strict" is set (RAILS_ENOCONV); a right-hand side that is not finite gives RAILS_EINVAL. */
typedef struct rails_iter rails_iter;
#define RAILS_ENOCONV -7 /* strict mode only: a column did not reach the tolerance */
#define RAILS_ITER_CG 1
#define RAILS_ITER_BICGSTAB 2
int rails_iter_create(rails_ctx *ctx, rails_csr *A, int method, const double *diag_host, rails_iter **out);
int rails_iter_set(rails_iter *it, const char *name, double value);
/* Y[:, yc0:yc0+nc] = A^-1 X[:, xc0:xc0+nc] (trans != 0: A^-T; CG ignores it), out of place, any nc (groups of 32 columns); X is left
 * unchanged and columns of Y outside the window are not touched.  The object owns its work panels and grows them only for a wider nc.
 * Synchronises. */
int rails_iter_solve(rails_ctx *ctx, rails_iter *it, int trans, const rails_panel *X, int xc0, int nc, rails_panel *Y, int yc0);
/* Y[:, yc0:yc0+nc] = p_K(G A) G X[:, xc0:xc0+nc]: the preconditioner of the solve on its own, a fixed linear approximate inverse (K = 0:
 * G X).  Same window rules and groups of 32 columns as rails_iter_solve.  Queues its work and does not synchronise; the counters [1], [2],
 * [7], [13] and [14] of rails_iter_stats then count this call. */
int rails_iter_precondition(rails_ctx *ctx, rails_iter *it, const rails_panel *X, int xc0, int nc, rails_panel *Y, int yc0);
/* Builds or rebuilds the multigrid hierarchy of "amg" and uploads it, from the CSR arrays the operator's handle keeps on the host (every
 * handle of rails_csr_create does).  With "amg" on, rails_iter_precondition applies one cycle.  Synchronises. */
int rails_iter_amg_setup(rails_ctx *ctx, rails_iter *it);
/* The hierarchy by its matrices, the last (dense) one included: rows[l], nnz[l] and hi[l] (the Gershgorin bound of the smoother's
 * interval; 0 for the last matrix) for l < n.  Where cap allows, two more entries: [n] the last call's cycles, the products inside them
 * (with the level matrices, P and R) and, in hi[n], the launches of the object's own kernels inside them; [n + 1] the set-up's host time
 * and upload time in microseconds and, in hi[n + 1], the operator complexity.  Any pointer may be NULL.  Returns n (0: no hierarchy has
 * been built) or a negative code; at most cap entries are written.  rails_iter_stats keeps its 19 entries. */
int rails_iter_amg_info(const rails_iter *it, int64_t *rows, int64_t *nnz, double *hi, int cap);
/* Builds or rebuilds the block hierarchy of "block_amg" from the host copy a block-CSR handle keeps, and uploads it.  With "block_amg" on,
 * rails_iter_precondition applies one cycle.  Synchronises. */
int rails_iter_block_amg_setup(rails_ctx *ctx, rails_iter *it);
/* rails_iter_amg_info on the block hierarchy, with its conventions: per matrix the rows, the scalar entries (blocks times b^2) and the
 * smoother's bound (max_i sum_j |(G A)_ij|; 0 for the last matrix), then the two trailing entries.  Returns 0 when no block hierarchy has
 * been built (rails_iter_amg_info returns 0 on a block hierarchy, and this on a scalar one). */
int rails_iter_block_amg_info(const rails_iter *it, int64_t *rows, int64_t *nnz, double *hi, int cap);
/* Installs the block-Jacobi preconditioner and sets "block_jacobi" to 1.  blocks_host != NULL: the m / b diagonal blocks themselves, each
 * row-major b x b (the library inverts them, as it does diag_host), on any square operator.  blocks_host == NULL on a block-CSR handle: the
 * blocks of its host copy, b 0 or the handle's block size, a diagonal block stored more than once in a block row summed in stored order;
 * on a stored CSR handle with host arrays: the entries of row i whose column lies in i's block range, absent entries 0, duplicates added
 * in stored order.  blocks_host == NULL and b == 0 on anything but a block-CSR handle clears the blocks and turns the setting off.
 * Synchronises. */
int rails_iter_block_jacobi(rails_ctx *ctx, rails_iter *it, int b, const double *blocks_host);
/* Returns the number of blocks installed (0: none) and their size in *b (may be NULL); copies the first cap_blocks inverse blocks,
 * row-major, exactly as they were uploaded (inv_blocks_host may be NULL). */
int64_t rails_iter_block_jacobi_info(const rails_iter *it, int *b, double *inv_blocks_host, int64_t cap_blocks);
/* Last solve: info[0] most iterations of a column, [1] inner products, [2] launches of the library's own passes, [3] columns that did not
 * converge, [4] of those, broken down, [5] worst relative residual of the recurrence, [6] work-panel columns, [7] products with A;
 * totals since creation: [8] solves, [9] columns, [10] iterations summed over columns, [11] flagged columns, [12] products; the polynomial
 * preconditioner: [13] its applications in the last solve, [14] launches of the fused step kernel, [15] hi and [16] lo of the interval in
 * use (0 with degree 0); on a context that reduces: [17] all-reduces issued in the last call (per group of 32 columns, conjugate gradients
 * 1 at the start and 2 per queued iteration, BiCGStab 1 and 3; the polynomial adds none), [18] ghost-row exchanges the object issued
 * itself (before fused steps; those inside rails_spmm are not counted).  [7] counts every product with A, those inside fused steps
 * included.  Returns the number of entries written (at
 * most cap: a caller that passes 13 sees what it always saw), or a negative code. */
int rails_iter_stats(const rails_iter *it, double *info, int cap);
/* Per column of the last solve (any pointer may be NULL): iterations, relative residual of the recurrence, flags (2 converged, 4 stopped at
 * max_iterations, 8 breakdown, 16 non-finite).  Returns the number of columns of the last solve; at most cap are written. */
int rails_iter_columns(const rails_iter *it, int32_t *iterations, double *relres, int32_t *flags, int cap);
/* An operator handle whose rails_spmm is rails_iter_solve: it goes wherever the LU handle goes (rails_solver_set_inverse, ...). */
int rails_csr_create_iter(rails_ctx *ctx, rails_iter *it, rails_csr **out);
void rails_iter_destroy(rails_iter *it);

/* ---- sparse right-hand side (rails_amd/csrc/sprhs_host.cpp, sprhs.hip, lanczos.hip) ------------------------------------------------------
 * B of A X M' + M X A' + B B' = 0 as a sparse m x p matrix instead of a panel: the operator form of the reference's
 * MatrixOrMultiVectorWrapper (src/MatrixOrMultiVectorWrapper.hpp; src/main.cpp:67 reads B.mtx as a CrsMatrix and :98 hands it to the
 * solver).  p is not limited by the fused Lanczos' 128 panel columns and B costs its nonzeros, not 8 m p bytes. */

/* Host only (no device is touched).  Transpose of an n_rows x n_cols CSR matrix into t_rowptr (n_cols + 1), t_col, t_val (rowptr[n_rows]
 * each).  Stable: the entries of a transposed row come in increasing original row and duplicates keep their order.  RAILS_EINVAL for a
 * rowptr that does not start at 0 or decreases and for a column outside [0, n_cols); nothing is read out of range. */
int rails_csr_transpose_host(int64_t n_rows, int64_t n_cols, const int64_t *rowptr, const int32_t *col, const double *val, int64_t *t_rowptr,
                             int32_t *t_col, double *t_val);
/* Host only.  *out = ||B'B||_F^2 from B (n_rows x n_cols) and its transpose, with a sparse accumulator over the columns of B: no
 * n_cols x n_cols array.  Both forms are validated as above. */
int rails_csr_gram_norm2_host(int64_t n_rows, int64_t n_cols, const int64_t *rowptr, const int32_t *col, const double *val,
                              const int64_t *t_rowptr, const int32_t *t_col, const double *t_val, double *out);

/* Uploads B (m_local x p, CSR, p >= 0, any number of entries per row) and its transpose.  Single GPU only: B'W of a row-partitioned B
 * would need an all-reduce of p x w, so a context with more than one rank gets RAILS_EINVAL. */
typedef struct rails_sprhs rails_sprhs;
int rails_sprhs_create(rails_ctx *ctx, int64_t m_local, int p, const int64_t *rowptr, const int32_t *col, const double *val, rails_sprhs **out);
void rails_sprhs_destroy(rails_sprhs *S);
int64_t rails_sprhs_rows(const rails_sprhs *S);
int64_t rails_sprhs_cols(const rails_sprhs *S);
int64_t rails_sprhs_nnz(const rails_sprhs *S);
double rails_sprhs_gram_norm2(const rails_sprhs *S); /* ||B'B||_F^2, computed on the host at creation */
/* trans == 0: Y[:, yc0:yc0+nc] = B X[:, xc0:xc0+nc], X of p rows and Y of m; trans != 0: Y = B' X, X of m rows and Y of p. */
int rails_sprhs_apply(rails_ctx *ctx, rails_sprhs *S, int trans, const rails_panel *X, int xc0, int nc, rails_panel *Y, int yc0);
/* An operator handle whose rails_spmm is rails_sprhs_apply (both trans values), as rails_csr_create_lu makes one for an LU solve.  The
 * caller keeps the rails_sprhs alive while the handle is used. */
int rails_csr_create_sprhs(rails_ctx *ctx, rails_sprhs *S, rails_csr **out);
/* rows of X in a product with A (trans == 0): the columns of a rectangular operator or of a sparse right-hand side, the rows of any other */
int64_t rails_csr_cols(const rails_csr *A);
/* the sparse right-hand side behind a handle made by rails_csr_create_sprhs, NULL for any other operator */
rails_sprhs *rails_csr_sprhs(const rails_csr *A);

/* ---- block-CSR operators (rails_amd/csrc/bsr_host.cpp, bsr_choice.h, spmm_bsr.hip) -------------------------------------------------------
 * A sparse matrix of dense b x b blocks, 2 <= b <= 8 (the Jacobian of a PDE system with b unknowns per cell).  Block rows in CSR form:
 * browptr (int64, mb + 1), bcol (int32 block-column indices), bval (nnzb * b * b doubles, every block row-major) -- the layout of scipy's
 * bsr_matrix (indptr, indices, data[nnzb, b, b]).  A gathered row of X serves the b scalar rows of a block row from registers, and an
 * index costs 4 / b^2 bytes per scalar entry.  The product is bit for bit the row-gather product (rails_csr_set_variant 3) of the
 * expanded CSR matrix: every Y[i, j] one accumulator from +0, one fused multiply-add per stored entry of scalar row i in stored order,
 * the zeros inside a block included. */

/* Host only.  *nnzb = the number of b x b blocks that the entries of a CSR matrix (m x n_cols, both multiples of b) touch.  RAILS_EINVAL
 * with a text for a b outside 2 .. 8, sizes that are no multiples of b, a rowptr that does not start at 0 or decreases and a column
 * outside [0, n_cols); nothing is read out of range (this holds for the three functions). */
int rails_bsr_count_host(int64_t m, int64_t n_cols, int b, const int64_t *rowptr, const int32_t *col, int64_t *nnzb);
/* Host only.  Fills browptr (m / b + 1), bcol and bval (as many blocks as rails_bsr_count_host counts; zeros where a touched block has
 * no entry).  Block columns ascend within a block row; the CSR columns may come in any order; duplicate entries are added in stored order. */
int rails_bsr_fill_host(int64_t m, int64_t n_cols, int b, const int64_t *rowptr, const int32_t *col, const double *val, int64_t *browptr,
                        int32_t *bcol, double *bval);
/* Host only.  The transposed block matrix (nb block rows, mb block columns): a stable counting sort by block column, as
 * rails_csr_transpose_host, with every block transposed. */
int rails_bsr_transpose_host(int64_t mb, int64_t nb, int b, const int64_t *browptr, const int32_t *bcol, const double *bval,
                             int64_t *t_browptr, int32_t *t_bcol, double *t_bval);
/* An operator handle over a block-CSR matrix of mb block rows: rails_spmm multiplies by it (both trans values; the transposed copy is
 * made on the host at the first transposed product), rails_csr_rows is mb * b and rails_csr_nnz nnzb * b * b, rails_csr_prepare and
 * rails_csr_set_variant are accepted and change nothing.  Square only (nb_ext == mb) and single GPU only: RAILS_EINVAL on a context with
 * a partition, an all-reduce hook or a communicator, and from rails_csr_set_halo.  rails_iter_create takes the handle as it takes a
 * callback operator (no Jacobi diagonal unless one is given); "amg" over it is refused, and "poly_degree" without "eig_max" fails the
 * solve, both with RAILS_EINVAL: they read scalar CSR arrays, which the handle does not keep. */
int rails_csr_create_bsr(rails_ctx *ctx, int64_t mb, int64_t nb_ext, int b, const int64_t *browptr, const int32_t *bcol, const double *bval,
                         rails_csr **out);
/* b of a block-CSR handle, 1 for every other kind of handle */
int rails_csr_block_size(const rails_csr *A);
/* info[0 .. cap): nnzb, b, blocks of the longest block row, bytes on the device (the transposed copy included once it exists), then of the
 * last launch (zeros before the first): b, lanes per block row, threads per workgroup, block rows per lane group, whether every
 * workgroup's run of blocks fits the LDS buffer, grid: 10 values, the first min(cap, 10) are written.  RAILS_EINVAL for another kind of
 * handle. */
int rails_csr_bsr_stats(const rails_csr *A, int64_t *info, int cap);

typedef struct rails_sweep_plan rails_sweep_plan;
int rails_sweep_plan_create(int64_t m, int64_t ncols, const int64_t *rowptr, const int32_t *col, const double *val,
                            const int *params, rails_sweep_plan **out);
int rails_sweep_plan_destroy(rails_sweep_plan *plan);
int rails_sweep_plan_info(const rails_sweep_plan *plan, int64_t *iinfo, double *dinfo);
int rails_sweep_plan_array(const rails_sweep_plan *plan, int which, const void **ptr, int64_t *count);

/* ------------------------------------------------------------------ panels --- */

/* A panel holds m_local rows x capacity columns (ld >= capacity, padded).
 * Role: the MultiVector template parameter's storage (StlWrapper m_max x n_max buffer,
 * src/StlWrapper.hpp:13-21). */
int rails_panel_create(rails_ctx *ctx, int64_t m_local, int capacity, rails_panel **out);
/* The same with rows exactly ld >= capacity doubles apart (no padding to 16 columns): for a narrow block that is swept whole several
 * times in a row, where padded rows would only add cache lines.  Kernels that load 16 bytes at a time want ld even. */
int rails_panel_create_ld(rails_ctx *ctx, int64_t m_local, int capacity, int ld, rails_panel **out);
int rails_panel_destroy(rails_panel *P);
int64_t rails_panel_rows(const rails_panel *P);
int rails_panel_capacity(const rails_panel *P);
int rails_panel_ld(const rails_panel *P);
void *rails_panel_device_ptr(const rails_panel *P);
/* grow capacity preserving contents (StlWrapper::resize re-allocation, src/StlWrapper.cpp:238-248) */
int rails_panel_reserve(rails_ctx *ctx, rails_panel *P, int capacity);

/* host (column-major, ldh) <-> device columns [c0, c0+nc) */
int rails_panel_upload(rails_ctx *ctx, rails_panel *P, int c0, int nc, const double *host, int64_t ldh);
int rails_panel_download(rails_ctx *ctx, const rails_panel *P, int c0, int nc, double *host, int64_t ldh);

int rails_panel_fill(rails_ctx *ctx, rails_panel *P, int c0, int nc, double value);     /* operator=(double) :123 */
int rails_panel_scale(rails_ctx *ctx, rails_panel *P, int c0, int nc, double s);        /* operator*=  :131      */
int rails_panel_copy(rails_ctx *ctx, const rails_panel *X, int xc0, int nc, rails_panel *Y, int yc0); /* = / push_back :65,:367 */
int rails_panel_axpy(rails_ctx *ctx, double alpha, const rails_panel *X, int xc0, int nc, rails_panel *Y,
                     int yc0);                                                            /* += -=  :145-158        */
int rails_panel_random(rails_ctx *ctx, rails_panel *P, int c0, int nc);                  /* random() :414         */

/* C (a x b, host, column-major ldc) = X[:, xc0:+a]^T * Y[:, yc0:+b], summed over all ranks.
 * Replaces MultiVector::dot (src/StlWrapper.cpp:394-412; call sites
 * src/LyapunovSolver.hpp:173,187,394,400,406).  Synchronises. */
int rails_gram(rails_ctx *ctx, const rails_panel *X, int xc0, int a, const rails_panel *Y, int yc0, int b,
               double *C_host, int ldc);

/* Y[:, yc0:+r] = beta * Y[:, yc0:+r] + alpha * X[:, xc0:+k] * C   (C host, k x r column-major).
 * Replaces MultiVector * DenseMatrix (src/StlWrapper.cpp:168-187; call sites
 * src/LyapunovSolver.hpp:265,290,396,402,443).  X and Y may be the same panel only if the
 * column windows coincide exactly (in-place, row-local) or are disjoint. */
int rails_panel_gemm(rails_ctx *ctx, double alpha, const rails_panel *X, int xc0, int k, const double *C_host,
                     int ldc, int r, double beta, rails_panel *Y, int yc0);

/* Opt-in since round 3 (the library's own one-pass MFMA kernel, k_panel_gemm_wide, is the default and the faster one: 49 against 43-46
 * TFLOP/s at k = 324, r = 268): with RAILS_WIDE_GEMM=rocblas in the environment this call creates a rocBLAS handle (resolved with dlopen;
 * ~0.3 s in a warm process, seconds in a cold one, once per process, for the calling context's device, on the CALLING thread) and
 * rails_panel_gemm_wide with k, r >= 64 goes through rocblas_dgemm from then on (rails_ctx_library_gemm_ready).  Without the variable
 * the call does nothing. */
int rails_ctx_enable_library_gemm(rails_ctx *ctx);
int rails_ctx_library_gemm_ready(const rails_ctx *ctx);

/* Deferred small results: a chain Gram -> update -> Gram -> Cholesky -> update on the device without the host in between (the block
 * orthogonalisation of the coordinate-space back end behind the host's projected solve).  An arena of `nslots` slots of
 * `doubles_per_slot` doubles on the device with a pinned mirror; rails_gram_deferred leaves X'Y (a x b, leading dimension a, summed
 * over the ranks) in a slot and sends it on its way to the mirror; rails_panel_gemm_deferred takes the coefficient matrix of
 * Y = beta Y + alpha X C from a slot (rows [0, k) of its r columns, leading dimension ld); rails_chol_inverse_deferred turns the w x w
 * Gram matrix G of a slot (w <= 48) into D^-1 R^-1 (D = sqrt(diag G), R'R = D^-1 G D^-1) in another slot.  None of them synchronises;
 * rails_deferred_fetch copies from the mirror and is valid after a rails_ctx_sync that follows the call which filled the slot. */
int rails_deferred_reserve(rails_ctx *ctx, int nslots, int64_t doubles_per_slot);
int rails_gram_deferred(rails_ctx *ctx, const rails_panel *X, int xc0, int a, const rails_panel *Y, int yc0, int b, int slot);
int rails_panel_gemm_deferred(rails_ctx *ctx, double alpha, const rails_panel *X, int xc0, int k, int slot, int ld, int r, double beta,
                              rails_panel *Y, int yc0);
int rails_chol_inverse_deferred(rails_ctx *ctx, int slot_in, int w, int slot_out);
/* First update and second projection of a block in one pass over the basis (the second sweep of the reference's block
 * Gram-Schmidt, src/StlWrapper.cpp:314-344): Y[:, yc0:yc0+r] += alpha X[:, xc0:xc0+k] C with C on the host (k x r, leading dimension
 * ldc), then slot <- X[:, xc0:xc0+k]' Y[:, yc0:yc0+r2] for the leading r2 <= r updated columns (k x r2, leading dimension k, summed
 * over the ranks, on its way to the mirror).  Fused for r <= 17, r2 <= 16, 32 <= k <= 512; the two separate kernels otherwise. */
int rails_update_gram_deferred(rails_ctx *ctx, double alpha, const rails_panel *X, int xc0, int k, const double *C_host, int ldc, int r,
                               rails_panel *Y, int yc0, int r2, int slot);
/* The same with the updated columns written to Yout[:, oc0:oc0+r] and Y left as it was (Yout = Y, oc0 = yc0: the call above).  The
 * arithmetic is that of the call above, operation for operation: the r columns of Yout and the slot hold the same bits whichever way
 * it is called.  Where the two separate kernels run (k > 512, r > 17, r2 > 16, k < 32 or fewer than 4096 rows) Y is copied to Yout first.  Columns
 * of Yout outside the window are not touched; no alignment of Yout is assumed.  X's window must not overlap Y's or Yout's; Y's and
 * Yout's coincide or are disjoint. */
int rails_update_gram_deferred_out(rails_ctx *ctx, double alpha, const rails_panel *X, int xc0, int k, const double *C_host, int ldc, int r,
                                   const rails_panel *Y, int yc0, rails_panel *Yout, int oc0, int r2, int slot);
int rails_deferred_fetch(rails_ctx *ctx, int slot, int64_t n, double *host_out);

/* The same product for any number r of output columns: one upload of C, launches in slices of 128 columns with no host wait in
 * between (the basis rotation of the coordinate-space back end).  X and Y: different panels or disjoint windows. */
int rails_panel_gemm_wide(rails_ctx *ctx, double alpha, const rails_panel *X, int xc0, int k, const double *C_host, int ldc, int r,
                          double beta, rails_panel *Y, int yc0);

/* Tile counts of the dense kernels fitted to the widths a solve runs at: rails_update_gram_deferred[_out] with five column blocks per
 * wave for 256 < k <= 320, the wide-X Gram form with five tiles per wave instead of six where the same waves cover it (289 to 320 columns),
 * rails_panel_gemm_wide with 13, 15 or 17 output tiles where that is the exact count, and without the second half of its last chunk
 * of 32 where that lies past k.  All of it leaves out work on zero padding only: results are the same bits either way.  On by default;
 * RAILS_DENSE_TILE_FIT=0 in the environment (read at the first use) or this process-wide setter (on = 0; it wins over the variable)
 * restores the choices before the fit. */
void rails_dense_set_tile_fit(int on);
int rails_dense_tile_fit(void);
/* Template parameter of the context's last launch of k_update_gram<NBW, .>, of the wide-X Gram form k_gram_cols[2]<TI, ., .> and of
 * k_panel_gemm_wide<TR> (its last slice); 0 where there has been none.  Any of the three pointers may be NULL.  Read-only. */
int rails_dense_last_tiles(const rails_ctx *ctx, int *update_gram_nbw, int *gram_cols_ti, int *gemm_wide_tr);

/* The schedule of the one-pass form of rails_update_gram_deferred[_out]: the pipelined kernel (C in registers, one register set of X
 * refilled block by block, one conflict-free turn-around per tile) or the kernel as it was.  Both form the same
 * partial sums and add them in the same order: results are the same bits either way, and which shapes take the one-pass form does
 * not depend on it.  On by default; RAILS_UPDATE_GRAM_PIPELINE=0 in the environment (read at the first use) or this process-wide
 * setter (on = 0; it wins over the variable) restores the earlier kernel. */
void rails_dense_set_update_gram_pipeline(int on);
int rails_dense_update_gram_pipeline(void);
/* *form = which kernel the context's last one-pass update + second projection launched: 1 the earlier kernel, 2 the pipelined one;
 * 0 where there has been none.  Read-only. */
int rails_dense_last_update_gram_form(const rails_ctx *ctx, int *form);

/* Orthonormalise columns [k_old, k_old+w) of V against columns [0, k_old) and among themselves,
 * equivalent to the reference's column-wise CGS2 with pre/post normalisation
 * (src/StlWrapper.cpp:305-321): block CGS2 + CholQR2 on MFMA, falling back to the column-wise
 * form when the block Gram matrix is numerically rank deficient.  method: 0 = auto,
 * 1 = force column-wise, 2 = force block.  *used (may be NULL) receives the method used (1 column-wise, 2 block,
 * 3 block after one repair round: dependent columns replaced by their normalised residuals, see orth.hip). */
int rails_orthogonalize(rails_ctx *ctx, rails_panel *V, int k_old, int w, int method, int *used);
/* The same with a nullspace (opts.nullspace of matlab/RAILSsolver.m:538-616): columns [nc0, nc0+q) of the panel N (V's rows, not V
 * itself; [N, V_old] orthonormal, as the solver keeps them) are projected out in every projection round of every path -- block, repair round, column-wise -- together with V's
 * columns [0, k_old): one Gram pass [N V_old]'W, one all-reduce and one update W -= N D + V_old C per round (fused for q, w <= 32).
 * q = 0 is rails_orthogonalize. */
int rails_orthogonalize_deflated(rails_ctx *ctx, rails_panel *V, int k_old, int w, const rails_panel *N, int nc0, int q, int method, int *used);

/* Column sums of squares of X[:, c0:c0+nc), all-reduced over the ranks, to the host.  One pass over the window for any nc
 * (a kernel of its own, 16-byte loads along the rows, every order of summation fixed: two calls agree bit for bit).  Synchronises. */
int rails_panel_colnorms2(rails_ctx *ctx, const rails_panel *X, int c0, int nc, double *out_host);

/* An orthonormal basis of the range of columns that may be rank deficient: the reference's Morth for a start space
 * (matlab/RAILSsolver.m:567-580), in column order.  Column i of W = V[:, k_old:k_old+w) is scaled to unit length, projected twice
 * against N[:, nc0:nc0+q), V[:, 0:k_old) and the columns kept before it, and kept, normalised, when at least `tol` of its unit length
 * survives; otherwise it is dropped.  A column whose own norm is zero or not finite is dropped.  [N, V_old] must be orthonormal.
 * On return V[:, k_old:k_old+*kept) holds the kept directions and V[:, k_old+*kept : k_old+w) is zero; kept_idx (may be NULL, room for w)
 * receives the original column index (0 .. w-1) of each kept direction, in increasing order.  tol <= 0 means 1e-8.  Any w with
 * k_old + w <= capacity; q = 0 means no nullspace (N may then be NULL).  Works in blocks of 128 columns with block operations only:
 * the number of synchronisations grows with the number of blocks, not of columns (orth.hip). */
int rails_orthogonalize_range(rails_ctx *ctx, rails_panel *V, int k_old, int w, const rails_panel *N, int nc0, int q, double tol, int *kept,
                              int32_t *kept_idx);

/* Fused residual Lanczos (src/LyapunovSolver.hpp:367-447): L steps of Lanczos on the implicit
 *   R = AV*T*MV^T + MV*T*AV^T + B*B^T      (MV == V for M = I)
 * started from a fresh random unit vector (one RNG stream is consumed, as Q.random() does at :374).
 * One pass over [AV MV B] per step; alpha, beta and the breakdown test stay on the device.
 *   T_host: k x k column-major (ldt).  H_host: out, (L+1) x (L+1) column-major (ldh >= L+1),
 *   zero-filled then the tridiagonal entries set exactly where the reference sets them.
 *   *steps: Lanczos steps done (< L on breakdown, beta < 1e-14, :419-426).
 * The orthonormal Lanczos vectors q_0..q_{steps-1} stay in a device side buffer of the library until the
 * next call on the same context.  Column windows must start at even columns; k <= 512, p <= 128.  Synchronises. */
int rails_resid_lanczos(rails_ctx *ctx, const rails_panel *AV, int avc0, const rails_panel *MV, int mvc0, int k,
                        const double *T_host, int ldt, const rails_panel *B, int bc0, int p, int L,
                        double *H_host, int ldh, int *steps);

/* The same run with B a sparse right-hand side S (m x p, any p >= 0): per step one pass over [AV MV] that takes B's part of each row
 * from the CSR form, r = [AV MV]_row . g + sum_q B_val[q] g_B[B_col[q]] - alpha q_i - beta q_{i-1}, then c_B = B'r over the transposed
 * form, balanced by nonzeros and summed in a fixed order (two runs from one seed give the same bits).  Everything else -- the RNG
 * stream, H, the breakdown test, the stored vectors, rails_lanczos_last_launch, k <= 512, even window starts -- as above.  Single GPU. */
int rails_resid_lanczos_sparse(rails_ctx *ctx, const rails_panel *AV, int avc0, const rails_panel *MV, int mvc0, int k, const double *T_host,
                               int ldt, const rails_sprhs *S, int L, double *H_host, int ldh, int *steps);

/* Start of a residual Lanczos run only: draws the random start vector q0 (one RNG stream, as Q.random() at :374), and
 * returns sums_host = [AV^T q0 (k) | MV^T q0 (k) | B^T q0 (p) | q0^T q0] (summed over the ranks) in ONE pass over the
 * panels.  q0 (un-normalised) becomes Lanczos vector 0 for rails_lanczos_vectors.  Used by the projected-space Lanczos
 * of rails/HipSolverOps.hpp, which carries the recurrence itself in the (2k+p+1)-dimensional coefficient space. */
int rails_lanczos_start(rails_ctx *ctx, const rails_panel *AV, int avc0, const rails_panel *MV, int mvc0, int k,
                        const rails_panel *B, int bc0, int p, double *sums_host);

/* Out[:, oc0:oc0+w] = Q * S with Q the Lanczos vectors of the last rails_resid_lanczos and S (steps x w,
 * host column-major, lds).  Replaces `eigenvectors = Q * v` (src/LyapunovSolver.hpp:443); passing only the
 * selected columns of v writes the expansion vectors straight into V's tail (:338-339). */
int rails_lanczos_vectors(rails_ctx *ctx, const double *S_host, int lds, int w, rails_panel *Out, int oc0);
/* Which pass kernel the context's last rails_resid_lanczos / rails_lanczos_start launched: k_lanczos_pass<nch, unroll> (nch = 128-column
 * pair chunks per lane, unroll = rows in flight per wave) on nblocks blocks.  Read-only; an error before the first run. */
int rails_lanczos_last_launch(rails_ctx *ctx, int *nch, int *unroll, int *nblocks);
int rails_lanczos_release(rails_ctx *ctx); /* frees the Lanczos vectors kept by the context (also done by rails_ctx_destroy) */

/* ---------------------------------------------------------- timing helpers --- */
/* HIP-event timing on the context's stream (bench.py's roofline leg). */
/* Make room for `bytes` of coefficient uploads / small results now (pinned staging buffer and its device counterpart) instead
 * of at the call that first needs it. */
int rails_ctx_reserve_staging(rails_ctx *ctx, size_t bytes);
int rails_timer_start(rails_ctx *ctx);
int rails_timer_stop(rails_ctx *ctx, double *ms);

/* ------------------------------------------------------ host numerics (C ABI) --- */
/* Kept on the host per the north star; thin C ABI with the argument meaning of the reference's
 * shims.  LAPACK is resolved at run time (env RAILS_LAPACK_LIB, scipy's OpenBLAS, MKL, system). */

/* src/SlicotWrapper.hpp:14-16.  Only (dico,job,fact) = ('C','X','N') is supported (the only use,
 * src/LyapunovSolver.hpp:357).  trans='T' solves A*X + X*A^T = scale*C, trans='N' A^T*X + X*A.
 * SLICOT itself is not available: Bartels-Stewart on dgees + dtrsyl; info = n+1 when the
 * triangular solve had to perturb (SLICOT's convention).  Two faster routes to the same X are tried first
 * where they apply, each checked before it is accepted: the eigen-decomposition for a symmetric A, and a
 * squared Smith iteration (level-3 BLAS, residual-verified to the level Bartels-Stewart reaches) for a
 * nonsymmetric A whose spectrum is clustered.  A holds its Schur form afterwards only
 * on the Bartels-Stewart route. */
void rails_sb03md(char dico, char job, char fact, char trans, int n, double *A, int lda, double *X, int ldx,
                  double *scale, int *info);
/* how many calls of this process took the squared-Smith route and the Bartels-Stewart route (diagnostics) */
void rails_sb03md_counts(long *smith, long *schur);
/* calls of the factored ADI form that built on the call before (a bordered extension of its matrix: shifts kept, LU factors extended)
 * and calls that started from scratch */
void rails_sb03md_adi_counts(long *extended, long *fresh);
/* after an attempt of the squared-Smith route that did not apply, the calling thread skips the attempt for the next 30 calls;
 * this sets that counter (0: try again at the next call) */
void rails_sb03md_set_pause(int calls);
/* src/LapackWrapper.hpp:21-22 */
void rails_dsyev(char jobz, char uplo, int n, double *a, int lda, double *w, int *info);
/* src/LapackWrapper.hpp:18-19 */
void rails_dsteqr(char compz, int n, double *d, double *e, double *z, int ldz, double *work, int *info);
/* src/BlasWrapper.hpp:34-42 (DGEMM), for the small host products of the restart (X' (VAV X), src/LyapunovSolver.hpp:286) */
void rails_dgemm(char transa, char transb, int m, int n, int k, double alpha, const double *A, int lda, const double *B,
                 int ldb, double beta, double *C, int ldc);
/* Triangular solve with many right-hand sides (BLAS DTRSM; src/BlasWrapper.hpp has no counterpart -- the generalized projected
 * solve, matlab/mex/lyap.c:125-133, reduces with the Cholesky factor of V'MV through it) */
void rails_dtrsm(char side, char uplo, char transa, char diag, int m, int n, double alpha, const double *A, int lda, double *B, int ldb);
/* Cholesky (generalized projected solve, block orthogonalisation) */
void rails_dpotrf(char uplo, int n, double *a, int lda, int *info);
/* Cholesky with complete pivoting of a positive semi-definite matrix (LAPACK dpstrf): P'AP = R'R, stops at the first pivot
 * <= tol; *rank = pivots taken, piv 0-based (column j of the factor belongs to column piv[j] of A); info 1 = rank < n. */
void rails_dpstrf(char uplo, int n, double *a, int lda, int *piv, int *rank, double tol, int *info);
/* Orthonormal basis of the column space of A (m x n, overwritten): pivoted Householder QR (dgeqp3 + dorgqr), rank = pivots with
 * |r_ii| > tol*|r_11|; q (m x rank, ldq >= m).  info = -100 when the host LAPACK lacks dgeqp3/dorgqr. */
void rails_range_basis(int m, int n, double *a, int lda, double tol, double *q, int ldq, int *rank, int *info);
int rails_host_lapack_init(const char *path);
const char *rails_host_lapack_path(void);

#ifdef __cplusplus
}
#endif
#endif /* RAILS_HIP_H */
