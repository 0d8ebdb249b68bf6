// amg_host.h -- the host set-up of the smoothed-aggregation multigrid preconditioner of the iterative A^-1 operator (iter_hierarchy.hip: rails_iter_amg_setup, "amg";
// DESIGN.md section 16).  No HIP in here: the library compiles amg_host.cpp for the host, tests/cpp/amg_host.cpp stands alone on it, and
// tests/amg_reference.py restates it in numpy/scipy.
//
// Per level l, from A_l (CSR, n_l rows, columns of a row strictly increasing, diagonal d stored, nonzero and finite):
//   strength   entry j != i is strong when |a_ij| >= theta_l sqrt(|a_ii| |a_jj|), theta_l = theta 0.5^l
//   aggregates three passes in row order: (1) an unaggregated row with strong neighbours, all of them unaggregated, founds an aggregate
//              with them; (2) a remaining row joins the aggregate of its strongest strong neighbour that pass 1 aggregated (the largest
//              |a_ij|, ties to the lower column); (3) what is left founds aggregates with its unaggregated strong neighbours, a row
//              with none is a singleton
//   T          n_l x aggregates, a one per row
//   P          (I - (4 / (3 hi)) D^-1 A_l) T with hi = rails_cheb_gershgorin(A_l, 1 / d), the bound the smoother uses
//   R          P' (rails_csr_transpose_host: stable)
//   A_{l+1}    R A_l P by two Gustavson products (R A_l, then times P); columns sorted, structural entries kept where they cancel
// Stop: n_l <= coarse, RAILS_AMG_MAX_LEVELS matrices, or a level that would keep more than 0.8 of its rows.  The last matrix has at
// most RAILS_AMG_MAX_COARSE rows (else RAILS_EINVAL, "does not coarsen") and is inverted densely: Cholesky of defsign A_L
// (rails_dpotrf), two triangular solves against the identity (rails_dtrsm), column-major.  Every traversal and every sum has one fixed
// order: two builds from the same arrays give the same bytes.
#ifndef RAILS_AMG_HOST_H
#define RAILS_AMG_HOST_H

#include <cstdint>
#include <vector>

constexpr int RAILS_AMG_MAX_LEVELS = 16;    // matrices of a hierarchy, the coarsest included
constexpr int RAILS_AMG_MAX_COARSE = 1024;  // rows of the dense coarsest block
constexpr double RAILS_AMG_THETA = 0.08;    // default of "amg_theta"
constexpr int RAILS_AMG_COARSE = 256;       // default of "amg_coarse"

struct rails_amg_csr {
    int64_t n_rows = 0, n_cols = 0;
    std::vector<int64_t> rowptr;
    std::vector<int32_t> col;
    std::vector<double> val;
    int64_t nnz() const { return rowptr.empty() ? 0 : rowptr.back(); }
};

struct rails_amg_level {
    rails_amg_csr A, P, R;      // A_l (n_l x n_l), P (n_l x n_{l+1}), R = P'
    std::vector<double> dinv;   // 1 / diagonal of A_l
    double hi = 0.0;            // Gershgorin bound on D^-1 A_l
    std::vector<int32_t> agg;   // aggregate of every row
};

struct rails_amg_hierarchy {
    std::vector<rails_amg_level> levels; // the multigrid levels; none for a matrix of at most `coarse` rows
    rails_amg_csr coarse;                // the last matrix A_L
    std::vector<double> coarse_inv;      // its dense inverse, column-major, n_L x n_L
    double defsign = 1.0;                // -1: negative definite
};

// RAILS_OK or RAILS_EINVAL (the message names the reason; nothing is read out of range of a matrix that is refused)
int rails_amg_build_host(int64_t n, const int64_t *rowptr, const int32_t *col, const double *val, double theta, int coarse,
                         rails_amg_hierarchy *out);

// The pieces the block form of the set-up (block_amg_host.cpp) takes from here, so that each rule is written once:
// the three aggregation passes on a matrix with its diagonal (returns the number of aggregates),
int64_t rails_amg_aggregate(const rails_amg_csr &A, const std::vector<double> &diag, double theta_l, std::vector<int32_t> &agg);
// C = A B by Gustavson's row-wise product, the columns of a row sorted, every structural entry kept,
void rails_amg_spgemm(const rails_amg_csr &A, const rails_amg_csr &B, rails_amg_csr &C);
// and the dense inverse (column-major) of the last matrix through the Cholesky factorisation of defsign A.
int rails_amg_dense_inverse(const rails_amg_csr &A, double defsign, std::vector<double> &inv);

#endif
