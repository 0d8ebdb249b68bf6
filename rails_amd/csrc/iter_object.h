// iter_object.h -- the iterative A^-1 operator as an object: what itsolve.hip (the calls, everything that launches a kernel),
// iter_setup.hip (lifetime, settings, work panels, statistics) and iter_hierarchy.hip (the multigrid hierarchies, the block-Jacobi
// blocks) share.  Which preconditioner is in effect is never read off the fields below directly: rails_iter_facts and iter_precond.h.
#ifndef RAILS_ITER_OBJECT_H
#define RAILS_ITER_OBJECT_H

#include "rails_internal.h"

#include <vector>

#include "amg_host.h"
#include "iter_precond.h"
#include "iter_scalars.h"

constexpr int RAILS_ITER_GROUP = 32; // columns per group: the widest panel every SpMM kernel takes in one chunk
// default of "poly_ratio" (hi / lo): the smallest worst case of products relative to plain CG over the table of DESIGN.md section 15
constexpr double RAILS_ITER_POLY_RATIO = 10.0;

// The multigrid hierarchy on the device (amg_host.h and block_amg_host.h build it on the host).  Level 0 works in the object's own work
// panels (r = W_R, z = W_Z / W_Z2, d = W_D, q = W_Q) on the object's operator; the levels below own their operators and five panels of
// the same row stride; the last matrix is its dense inverse with two panels (none when there is no level: W_R and W_Z then).  A call
// reaches every level's panels through its Sweep (itsolve.hip: plan_call), level 0's like the others.
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

// iter_setup.hip
// whether a stored operator keeps its scalar CSR arrays on the host (every handle of rails_csr_create does)
bool rails_iter_host_csr(const rails_csr *A, int64_t m);
// the facts iter_precond.h decides on, read off the object as it stands
rails_precond_facts rails_iter_facts(const rails_iter *it);
// RAILS_EINVAL with the refusal's text where iter_precond.h does not grant the request
int rails_iter_grant(const rails_iter *it, int request, int v, const char *who);
// the upper end of the polynomial's interval where the passes apply `pass` (RAILS_PC_PASS_*): "eig_max", else the Gershgorin bound (0: none)
double rails_iter_poly_hi(const rails_iter *it, int pass);
// the work panels `want` (bits 1 << W_...) beside those there are, at `cols` columns or more; the columns' scalars and the pinned block
int rails_iter_grow_work(rails_ctx *c, rails_iter *it, int cols, unsigned want);
int rails_iter_grow_cols(rails_ctx *c, rails_iter *it, int nc);
// iter_hierarchy.hip
// drops the hierarchy (a changed "amg_theta" or "amg_coarse", a rebuild, the end of the object)
void rails_iter_amg_release(rails_iter *it);
// before a call with a cycle in effect: the hierarchy of that kind when there is none yet, the level panels at the work panels' width
int rails_iter_amg_prepare(rails_ctx *c, rails_iter *it, bool block);

#endif
