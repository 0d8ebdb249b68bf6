/* ============================================================================
 * rails_solver.h -- C ABI of the RAILS solver instantiated on the HIP backend:
 *   rails::Solver<HipOperatorWrapper, HipMultiVectorWrapper, HostDenseMatrix>
 * (rails_amd/include/rails/), the drop-in counterpart of the reference's
 *   RAILS::Solver<Matrix, MultiVector, DenseMatrix>   (src/LyapunovSolverDecl.hpp:9-51).
 * This is what a non-C++ host (Python via ctypes, see rails_amd/solver.py) binds.
 * Return conventions as in rails_hip.h.
 * ==========================================================================*/
#ifndef RAILS_SOLVER_H
#define RAILS_SOLVER_H

#include "rails_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rails_solver rails_solver;

/* Solver(A, B, M) -- src/LyapunovSolverDecl.hpp:13-16.  A, M: operators created with rails_csr_create
 * (M may be NULL = identity; the caller keeps ownership).  B: host column-major block of the LOCAL rows,
 * m_local x p with leading dimension ldb.  m_global: global row count (= m_local on one GPU). */
int rails_solver_create(rails_ctx *ctx, rails_csr *A, rails_csr *M, const double *B_host, int64_t ldb, int p,
                        int64_t m_global, rails_solver **out);
/* The same with B a sparse right-hand side (rails_sprhs_create; the caller keeps S alive): B takes the operator form of the reference's
 * B adaptor (src/MatrixOrMultiVectorWrapper.hpp; src/main.cpp:67,98).  Single GPU.  Such a solver always runs the direct back end
 * (rails_amd/csrc/solve_choice.h), so rails_solver_backend_stats is "{}" and the options "subspace" and "projected_lanczos" are accepted
 * and ignored.  The projection methods that start from B (1.2, 2.2) are refused (*code = -2), as for
 * any operator B. */
int rails_solver_create_sparse(rails_ctx *ctx, rails_csr *A, rails_csr *M, rails_sprhs *S, int64_t m_global, rails_solver **out);
int rails_solver_destroy(rails_solver *s);

/* set_parameters -- src/LyapunovSolver.hpp:72-98.  Names are the reference's ("Maximum iterations",
 * "Tolerance", "Expand size", "Lanczos iterations", "Restart size", "Reduced size", "Restart iterations",
 * "Restart tolerance", "Minimize solution space", "Restart from solution", "Restart upon start" (opts.restart_upon_start of
 * matlab/RAILSsolver.m:53-57: shrink the space right after the first projected solve of a warm start); any capitalisation the
 * reference accepts).  Values are stored until rails_solver_apply_parameters, which returns the
 * reference's code (0 ok, 1 = Lanczos iterations <= Expand size). */
int rails_solver_set_parameter(rails_solver *s, const char *name, double value);
int rails_solver_apply_parameters(rails_solver *s, int *code);

/* extensions: "mass" (use M, generalized equation), "mass_orthogonalisation" (with mass: keep V M-orthonormal, V'MV = I, so that the
 * projected equation is the standard one -- `opts.ortho = 'M'` of matlab/RAILSsolver.m:38-41,384,583-597; default 0: orthonormal V and the
 * generalized projected equation by Cholesky reduction), "verbose", "max_trips", "projected_lanczos" (M = I only: carry the
 * residual Lanczos recurrence in coefficient space, see rails/HipSolverOps.hpp), "subspace" (default 1: run the solver template on the
 * coordinate-space back end of rails/SubspaceWrappers.hpp -- all multivectors as coordinates in one orthonormal device basis;
 * 0: the direct back end of rails/HipWrappers.hpp; which solves the coordinate-space back end takes, and why the others go to the direct
 * one, is the one rule of rails_amd/csrc/solve_choice.h) */
int rails_solver_set_option(rails_solver *s, const char *name, double value);
/* opts.Ainv of matlab/RAILSsolver.m:18-22: the operator the projection methods other than 1 apply as A^-1 ("Projection method" =
 * 1.1, 1.2, 1.3: expand with A^-1 r instead of r; 2.1, 2.2, 2.3: with [r, A^-1 r]; the decimal picks the start space -- .1 A^-1 V0
 * (2.x: [V0, A^-1 V0]), .2 A^-1 B ([B, A^-1 B]), .3 V0 -- matlab/RAILSsolver.m:7-16).  Any operator handle of A's row count: a
 * sparse LU solve (rails_csr_create_lu), a callback, a CSR matrix.  The caller keeps ownership, as for A and M.  "Projection method"
 * itself is a parameter (rails_solver_set_parameter); rails_solver_apply_parameters returns code 2 for a value that is no method, and
 * rails_solver_solve refuses a method other than 1 without an inverse (RAILS_EINVAL). */
int rails_solver_set_inverse(rails_solver *s, rails_csr *Ainv);
/* opts.nullspace of matlab/RAILSsolver.m:33-34,221-222,538-616: N (host column-major, the LOCAL rows x q, leading dimension ldn, like B)
 * spans a space that is projected out of every space that joins V -- the start space (cold, warm or A^-1 start) and every expansion --
 * for a singular A with a known kernel.  The solve orthonormalises N (M-orthonormalises it with "mass_orthogonalisation", a deliberate
 * deviation from the reference, whose Euclidean basis makes its M-projection no projector) and drops dependent columns; it is refused
 * (*code = -2, V and T unchanged) when none is left or the rank reaches the problem size.  q = 0 clears it.  Both back ends. */
int rails_solver_set_nullspace(rails_solver *s, const double *N_host, int64_t ldn, int q);
/* columns of the nullspace the last solve kept after orthonormalisation (0 without one) */
int rails_solver_nullspace_rank(rails_solver *s);

/* called at the start of every loop trip with the index of that trip, and once after the last */
typedef void (*rails_trip_fn)(void *user, int trip);
int rails_solver_set_trip_callback(rails_solver *s, rails_trip_fn fn, void *user);

/* warm start: set V (host column-major, local rows x k); assumed orthonormal ("Restart from solution") */
int rails_solver_set_V(rails_solver *s, const double *V_host, int64_t ldv, int k);

/* opts.space of matlab/RAILSsolver.m:25-28: columns [c0, c0+k) of a device panel of the solver's local rows (a previous solution's
 * rails_solution_panel, [V_prev, B], the union of two earlier solutions) become the start space of the NEXT solve, copied device to
 * device.  They need not be orthonormal or independent: the solve orthonormalises them (rails_orthogonalize_range), drops every column
 * of which less than 1e-8 survives and projects the nullspace out.  The next solve is a warm start whatever "Restart from solution"
 * says; one solve consumes the space, as rails_solver_set_V is consumed.  The solve is refused (*code = -2, V and T unchanged) when no
 * column survives.  Both back ends (with a nullspace set as well: the direct one, rails_amd/csrc/solve_choice.h).  (On the direct back end such a solve applies the
 * parameters set so far, as rails_solver_apply_parameters does.)  A panel with another row count, or k < 1: RAILS_EINVAL. */
int rails_solver_set_start_space(rails_solver *s, const rails_panel *P, int c0, int k);
/* columns the last solve kept of its start space; 1 after a cold start */
int rails_solver_start_rank(rails_solver *s);

/* solve(V, T) -- src/LyapunovSolver.hpp:100-346.  *code = 0 converged, -1 not converged, 1 loop exhausted,
 * 2 stopped by max_trips; *k = V.N(). */
int rails_solver_solve(rails_solver *s, int *code, int *k);

int rails_solver_get_V(rails_solver *s, double *V_host, int64_t ldv); /* local rows x k */
int rails_solver_get_T(rails_solver *s, double *T_host, int ldt);     /* k x k */
int rails_solver_trips(rails_solver *s);
/* ||B||_2^2 as the last solve computed it on either back end, the scale of its stopping test (src/LyapunovSolver.hpp:134); 0 before the
 * first solve */
int rails_solver_scale(rails_solver *s, double *scale);
int rails_solver_history(rails_solver *s, double *res, int cap);      /* Lanczos estimates per trip; returns count */

/* host wall-clock seconds per solver section of the last solve (JSON object; names follow the reference's profile
 * sections, src/Timer.hpp:101-106: "Apply A", "Apply B", "Compute VAV", "dense_solve", "Residual Lanczos", ...) */
int rails_solver_profile(rails_solver *s, char *buf, int cap);
/* JSON counters of the coordinate-space back end for the last solve ("{}" when the direct back end ran). */
const char *rails_solver_backend_stats(rails_solver *s);

/* ||A X + X A' + B B'||_F / ||B B'||_F for X = V T V' evaluated on the device without forming X
 * (uses R = [AV V B] G [AV V B]'; test / reporting helper).  The norm comes out of a trace of Gram products, i.e. as the
 * square root of a difference of O(||X||^2 ||A||^2) terms: it bottoms out near 1e-8 relative.  Below that use products with R
 * itself (tests/test_gpu_fullsize.py does a power iteration on R). */
/* With a sparse B (rails_solver_create_sparse): P = [AV MV], K = [[0 T],[T 0]], Z = B'P (a p-row panel), and
 * ||R||_F^2 = tr((P'P K)^2) + 2 tr(K Z'Z) + ||B'B||_F^2 with the last term from rails_sprhs_gram_norm2: no m x p or p x p array. */
int rails_solver_relative_residual(rails_solver *s, double *rel);

#ifdef __cplusplus
}
#endif
#endif
