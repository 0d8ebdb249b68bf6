// block_jacobi_host.h -- the host part of the block-Jacobi preconditioner of the iterative A^-1 operator (iter_hierarchy.hip: rails_iter_block_jacobi; DESIGN.md section
// 18): where the b x b diagonal blocks come from and what is refused (rails_bj_plan), their extraction from block-CSR and CSR arrays, and
// their inverses in long double.  No HIP in here: tests/cpp/block_jacobi_host.cpp stands alone on it.
#ifndef RAILS_BLOCK_JACOBI_HOST_H
#define RAILS_BLOCK_JACOBI_HOST_H

#include <cstddef>
#include <cstdint>

constexpr int RAILS_BJ_MIN_B = 2, RAILS_BJ_MAX_B = 8;

// the operator the object iterates on, as far as the blocks' source depends on it
enum { RAILS_BJ_OP_CSR = 0, RAILS_BJ_OP_CSR_NO_HOST, RAILS_BJ_OP_BSR, RAILS_BJ_OP_CALLBACK, RAILS_BJ_OP_LU, RAILS_BJ_OP_ITER };
// what rails_iter_block_jacobi does
enum { RAILS_BJ_CLEAR = 0, RAILS_BJ_FROM_ARGUMENT, RAILS_BJ_FROM_BSR, RAILS_BJ_FROM_CSR };

// The decision of rails_iter_block_jacobi(ctx, it, b, blocks) on an operator of kind `op` (block size handle_b where it is block-CSR) of
// m rows: *source and the block size in effect *b_eff, or a refusal (nonzero, the reason in err).  Nothing but integers in, so that every
// refusal is tested without a device.
int rails_bj_plan(int op, int handle_b, bool reduces, int64_t m, int b, bool blocks_given, int *source, int *b_eff, char *err, size_t cap);

// The diagonal blocks (mb of them, row-major b x b, zeroed first) of a block-CSR matrix: a diagonal block stored more than once in a
// block row is summed in stored order.
void rails_bj_from_bsr(int64_t mb, int b, const int64_t *browptr, const int32_t *bcol, const double *bval, double *blocks);
// ... and of a CSR matrix of m = mb * b rows: the entries of row i whose column lies in i's block range; absent entries are 0, duplicates
// are added in stored order.  Columns need not be sorted.
void rails_bj_from_csr(int64_t mb, int b, const int64_t *rowptr, const int32_t *col, const double *val, double *blocks);

// inv[k] = blocks[k]^-1 for k < nblocks by Gauss-Jordan elimination with partial pivoting in long double, rounded to double once at the
// end.  Nonzero with the block named in err: a zero or non-finite pivot, a non-finite entry of the inverse.
int rails_bj_invert(int64_t nblocks, int b, const double *blocks, double *inv, char *err, size_t cap);

#endif
