// block_amg_host.h -- the host set-up of the block multigrid preconditioner of the iterative A^-1 operator (iter_hierarchy.hip: rails_iter_block_amg_setup, "block_amg";
// DESIGN.md section 19): smoothed aggregation on the cells of a block-CSR operator with b unknowns per cell.  No HIP in here: the library
// compiles block_amg_host.cpp for the host, tests/cpp/block_amg_host.cpp stands alone on it, and tests/block_amg_reference.py restates it
// in numpy/scipy.
//
// Per level l, from A_l in block-CSR form (mb_l block rows of b x b row-major blocks, the block columns of a block row strictly
// increasing, every diagonal block stored, the same b on every level):
//   N_l        the condensed node matrix: scalar CSR, mb_l x mb_l, the block pattern; entry (I, J) is the Frobenius norm of block (I, J),
//              the sum of its squares in stored order, then the square root
//   aggregates amg_host.h's strength rule and three passes on N_l (rails_amg_aggregate), theta_l = theta 0.5^l
//   T          T_nodes (x) I_b: unknown r of cell I goes to component r of I's aggregate
//   G_l        the inverses of the diagonal blocks (rails_bj_invert: long double, rounded once)
//   hi_l       max_i sum_j |(G_l A_l)_ij|: per block row the products G_I A_IJ in stored order, entry (r, s) of a product one sum over k
//              ascending of G_I[r][k] A_IJ[k][s] (a product, then an addition), the row sums over the blocks in stored order, s ascending
//   P          T - (4 / (3 hi_l)) (G_l A_l) T, the product with T by rails_amg_spgemm on the expanded G_l A_l
//   R          P' (rails_csr_transpose_host: stable)
//   A_{l+1}    R A_l P by two Gustavson products on the expanded A_l (zeros inside blocks kept), columns sorted, then blocked by
//              rails_bsr_count_host / rails_bsr_fill_host: block-aligned by construction
// Stop: at most `coarse` rows left, RAILS_AMG_MAX_LEVELS matrices, or a level that would keep more than 0.8 of its block rows.  The last
// matrix has at most RAILS_AMG_MAX_COARSE rows (else "does not coarsen") and is inverted densely as amg_host.h's is.  Every traversal and
// every sum has one fixed order: two builds from the same arrays give the same bytes.
#ifndef RAILS_BLOCK_AMG_HOST_H
#define RAILS_BLOCK_AMG_HOST_H

#include "amg_host.h"

struct rails_bamg_bsr {
    int b = 0;
    int64_t mb = 0;
    std::vector<int64_t> browptr;
    std::vector<int32_t> bcol;
    std::vector<double> bval; // nnzb blocks, row-major b x b
    int64_t nnzb() const { return browptr.empty() ? 0 : browptr.back(); }
};

struct rails_bamg_level {
    rails_bamg_bsr A;          // A_l
    rails_amg_csr P, R;        // mb_l b x mb_{l+1} b, and its transpose
    std::vector<double> ginv;  // G_l: mb_l inverse diagonal blocks, row-major
    double hi = 0.0;           // the bound on the spectrum of G_l A_l
    std::vector<int32_t> agg;  // aggregate of every cell
};

struct rails_bamg_hierarchy {
    int b = 0;
    std::vector<rails_bamg_level> levels; // none for a matrix of at most `coarse` rows
    rails_bamg_bsr coarse;                // the last matrix A_L
    std::vector<double> coarse_inv;       // its dense inverse, column-major, n_L x n_L
    double defsign = 1.0;                 // -1: negative definite
};

// RAILS_OK or RAILS_EINVAL (the message names the reason; nothing is read out of range of a matrix that is refused)
int rails_bamg_build_host(int64_t mb, int b, const int64_t *browptr, const int32_t *bcol, const double *bval, double theta, int coarse,
                          rails_bamg_hierarchy *out);

#endif
