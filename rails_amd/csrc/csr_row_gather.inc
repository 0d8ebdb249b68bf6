// csr_row_gather.inc -- the row gather the kernels of itsolve.hip share (included by iter_kernels.inc, so inside itsolve.hip's anonymous namespace, after it_v2, ld2
// and st2): t = (A Zin)_row for the rows of one block by k_spmm_narrow's scheme (spmm.hip), then epilogue(row, offset of the thread's
// pair in a work panel, t, full) in the same thread.  k_cheb_step_csr (the fused Chebyshev step) and k_amg_residual_csr (the multigrid
// cycle's residual) differ in their epilogues only.
//
// LPR lanes own a row and two adjacent columns each, 64 rows per block, the block's (col, val) run staged in LDS, 32-bit byte offsets;
// one entry at a time for a block whose run is longer than the LDS buffer and for the lane of an odd last column.  Zin is a work panel:
// window at column 0, row stride ld, rows 16-byte aligned.  GHOST, a row-partitioned operator: column c >= m is row c - m of the
// operator's ghost buffer Zg (row stride ldg doubles) -- the select between two bases and two strides k_spmm_narrow<RPG, true, LPR> makes.
// The epilogue runs for local rows only, once per (row, pair); the pad column beside an odd last column may be read, never written.
template <int RPG, int LPR, bool GHOST, class Epilogue>
__device__ __forceinline__ void csr_row_gather(int64_t m, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, const double *__restrict__ val,
                                               const double *__restrict__ Zin, int ld, int nc, int64_t blocks_per_xcd, const double *__restrict__ Zg, int ldg,
                                               Epilogue epilogue)
{
    constexpr int GROUPS = 256 / LPR, ROWS = GROUPS * RPG, CAP = 2048;
    __shared__ double s_val[CAP];
    __shared__ int32_t s_col[CAP];
    const int g = threadIdx.x / LPR;
    const int l = threadIdx.x % LPR;
    const int64_t lb = (int64_t)(blockIdx.x & 7) * blocks_per_xcd + (blockIdx.x >> 3);
    const int64_t r0 = lb * ROWS;
    if (r0 >= m) return;
    const int64_t r1 = (r0 + ROWS < m) ? r0 + ROWS : m;
    const int64_t nz0 = rowptr[r0], nz1 = rowptr[r1];
    const bool staged = (nz1 - nz0) <= CAP; // block-uniform
    if (staged) {
        for (int q = threadIdx.x; q < (int)(nz1 - nz0); q += 256) {
            s_col[q] = col[nz0 + q];
            s_val[q] = val[nz0 + q];
        }
        __syncthreads();
    }
    const int cb = l * 2;
    if (cb >= nc) return;
    const bool full = (cb + 2 <= nc);
    const uint32_t cb8 = (uint32_t)cb * 8u, ld8 = (uint32_t)ld * 8u;
    const uint32_t ldg8 = (uint32_t)ldg * 8u, m32 = (uint32_t)m;
    const char *Zb = reinterpret_cast<const char *>(Zin), *Gb = reinterpret_cast<const char *>(Zg);
    auto zrow = [&](uint32_t c) -> const char * {
        if (!GHOST) return Zb + (__umul24(c, ld8) + cb8);
        const bool local = c < m32;
        return (local ? Zb : Gb) + ((local ? __umul24(c, ld8) : __umul24(c - m32, ldg8)) + cb8);
    };
    for (int rr = 0; rr < RPG; ++rr) {
        const int64_t row = r0 + (int64_t)rr * GROUPS + g; // the rows in flight are consecutive
        if (row >= m) break;
        it_v2 acc = (it_v2){0.0, 0.0};
        if (staged && full) {
            int i = (int)(rowptr[row] - nz0);
            const int i1 = (int)(rowptr[row + 1] - nz0);
            for (; i + 8 <= i1; i += 8) {
                it_v2 x[8];
                double av[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    x[u] = *reinterpret_cast<const it_v2 *>(zrow((uint32_t)s_col[i + u]));
                    av[u] = s_val[i + u];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    acc.x = __builtin_fma(av[u], x[u].x, acc.x);
                    acc.y = __builtin_fma(av[u], x[u].y, acc.y);
                }
            }
            for (; i < i1; i += 4) { // the last one to seven: groups of four, the slots past the end repeat the last entry with a zero
                it_v2 x[4];
                double av[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int q = i + u < i1 ? i + u : i1 - 1;
                    x[u] = *reinterpret_cast<const it_v2 *>(zrow((uint32_t)s_col[q]));
                    av[u] = i + u < i1 ? s_val[q] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    acc.x = __builtin_fma(av[u], x[u].x, acc.x);
                    acc.y = __builtin_fma(av[u], x[u].y, acc.y);
                }
            }
        } else {
            for (int64_t p = rowptr[row]; p < rowptr[row + 1]; ++p) {
                const double av = val[p];
                const double *src = reinterpret_cast<const double *>(zrow((uint32_t)col[p]));
                acc.x = __builtin_fma(av, src[0], acc.x);
                if (full) acc.y = __builtin_fma(av, src[1], acc.y);
            }
        }
        epilogue(row, row * ld + cb, acc, full);
    }
}
