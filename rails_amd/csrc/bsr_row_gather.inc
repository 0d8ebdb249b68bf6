// bsr_row_gather.inc -- the block-row product the block-CSR kernels share: t = (A X) of the block rows of one workgroup by k_spmm_bsr's
// scheme (spmm_bsr.hip's head comment), then epilogue(block row, the lane's first column, its B x 2 accumulators, full, one) in the same
// thread.  Included by spmm_bsr.hip (k_spmm_bsr: a storing epilogue) and by iter_kernels.inc (k_cheb_step_bsr, the fused Chebyshev step
// with the block-Jacobi factor, and k_amg_residual_bsr, the multigrid cycle's residual), inside the anonymous namespace of either.
//
// LPR lanes own a block row; a lane owns two adjacent columns of the panel and holds B x 2 accumulators.  The arithmetic is fixed: every
// (A X)[i, j] is one accumulator, from +0, updated by one __builtin_fma per stored entry of scalar row i in stored order.  The epilogue
// runs once per live (block row, pair).  full: both columns of the pair are columns of the panel, and the accumulators hold them; else the
// lane owns the last column alone and its value is acc[r].x when `one` (a panel of one column) and acc[r].y otherwise (the lane loaded the
// last pair instead of its own, never past column nc of the window).
#ifndef RAILS_BSR_ROW_GATHER_INC
#define RAILS_BSR_ROW_GATHER_INC

typedef double bsr_v2 __attribute__((ext_vector_type(2)));
typedef bsr_v2 bsr_v2_a8 __attribute__((aligned(8))); // 16-byte accesses of two doubles that are only 8-byte aligned (windows on odd columns)

// The multiply-adds of one block into the B x 2 accumulators: row r of the block times the lane's two columns of the block's B rows of X,
// columns of the block ascending.  a: the block's B * B values, in LDS (staged) or in global memory (every lane of the group reads the
// same address).
template <int B>
__device__ __forceinline__ void block_fma(const double *a, const bsr_v2 (&x)[B], bsr_v2 (&acc)[B])
{
#pragma unroll
    for (int r = 0; r < B; ++r)
#pragma unroll
        for (int j = 0; j < B; ++j) {
            const double v = a[r * B + j];
            acc[r].x = __builtin_fma(v, x[j].x, acc[r].x);
            acc[r].y = __builtin_fma(v, x[j].y, acc[r].y);
        }
}

// One block row for one lane: its n blocks at cols / vals (a block row without blocks is given the first block of the workgroup's run,
// which exists whenever nmax > 0); every lane of the wave makes nmax steps (wave-uniform bound) and issues its loads unconditionally -- a
// lane past its own end re-reads the first block and skips the arithmetic -- so that no vector-memory load of X sits under a divergent
// branch (see lanczos_pass.inc's row loads).
template <int B>
__device__ __forceinline__ void block_row(int n, int nmax, const int32_t *__restrict__ cols, const double *__restrict__ vals, const char *__restrict__ Xb,
                                          int64_t ldx8, bool one, bsr_v2 (&acc)[B])
{
    constexpr int U = rails_bsr_unroll(B), BB = B * B;
    for (int k = 0; k < nmax; k += U) {
        bsr_v2 x[U][B];
        int at[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            at[u] = (k + u < n) ? k + u : 0;
            const char *src = Xb + (int64_t)cols[at[u]] * B * ldx8;
#pragma unroll
            for (int r = 0; r < B; ++r) {
                if (one) { // a panel of one column: 8 bytes
                    const double v = *reinterpret_cast<const double *>(src + r * ldx8);
                    x[u][r] = (bsr_v2){v, v};
                } else
                    x[u][r] = *reinterpret_cast<const bsr_v2_a8 *>(src + r * ldx8);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (k + u < n) block_fma<B>(vals + (int64_t)at[u] * BB, x[u], acc);
    }
}

// LPR lanes per block row, threads / LPR block rows in flight, rpg rounds of them per workgroup (bsr_choice.h decides all three).
template <int B, int LPR, class Epilogue>
__device__ __forceinline__ void bsr_row_gather(int64_t mb, const int64_t *browptr, const int32_t *bcol, const double *bval, const double *X, int ldx, int nc, int rpg,
                                               int64_t blocks_per_xcd, Epilogue epilogue)
{
    constexpr int NT = rails_bsr_threads(B), GROUPS = NT / LPR, CAP = rails_bsr_lds_blocks(B), BB = B * B;
    __shared__ double s_val[CAP * BB];
    __shared__ int32_t s_col[CAP];
    const int g = threadIdx.x / LPR;
    const int l = threadIdx.x % LPR;
    // the XCD-aware block -> row-range map of the row kernels (spmm.hip): XCD x gets the contiguous workgroups [x * bpx, (x + 1) * bpx)
    const int64_t lb = (int64_t)(blockIdx.x & 7) * blocks_per_xcd + (blockIdx.x >> 3);
    const int64_t rows = (int64_t)GROUPS * rpg;
    const int64_t r0 = lb * rows;
    if (r0 >= mb) return; // (the whole workgroup)
    const int64_t r1 = (r0 + rows < mb) ? r0 + rows : mb;
    const int64_t q0 = browptr[r0], q1 = browptr[r1];
    const bool staged = (q1 - q0) <= CAP; // workgroup-uniform
    if (staged) {
        for (int q = threadIdx.x; q < (int)(q1 - q0); q += NT) s_col[q] = bcol[q0 + q];
        for (int q = threadIdx.x; q < (int)(q1 - q0) * BB; q += NT) s_val[q] = bval[q0 * BB + q];
        __syncthreads();
    }
    const bool one = nc == 1;
    const int64_t ldx8 = (int64_t)ldx * 8;
    for (int rr = 0; rr < rpg; ++rr) {
        if (r0 + (int64_t)rr * GROUPS >= r1) break; // (uniform)
        const int64_t brow = r0 + (int64_t)rr * GROUPS + g; // the block rows in flight are consecutive
        int64_t i = 0; // where the block row starts in the workgroup's run
        int n = 0;
        if (brow < r1) {
            n = (int)(browptr[brow + 1] - browptr[brow]);
            if (n > 0) i = browptr[brow] - q0;
        }
        int nmax = n; // the longest block row among the wave's
#pragma unroll
        for (int off = LPR; off < 64; off *= 2) nmax = max(nmax, __shfl_xor(nmax, off, 64));
        nmax = __builtin_amdgcn_readfirstlane(nmax);
        for (int cb0 = 0; cb0 < nc; cb0 += 2 * LPR) {
            // this lane's two columns.  A lane whose columns start at or behind the last one loads the last pair instead -- never past column
            // nc of the window --; the lane of an odd last column then keeps the second accumulator of each row, lanes behind it keep nothing
            const int cb = cb0 + 2 * l;
            const int xo = one ? 0 : (cb + 2 <= nc ? cb : nc - 2);
            bsr_v2 acc[B];
#pragma unroll
            for (int r = 0; r < B; ++r) acc[r] = (bsr_v2){0.0, 0.0};
            const char *Xb = reinterpret_cast<const char *>(X + xo);
            if (staged) // the values as LDS broadcasts
                block_row<B>(n, nmax, s_col + i, s_val + i * BB, Xb, ldx8, one, acc);
            else // a run longer than the buffer: from global memory, the lanes of a group at one address
                block_row<B>(n, nmax, bcol + q0 + i, bval + (q0 + i) * BB, Xb, ldx8, one, acc);
            if (brow >= r1 || cb >= nc) continue;
            epilogue(brow, cb, acc, cb + 2 <= nc, one);
        }
    }
}

#endif
