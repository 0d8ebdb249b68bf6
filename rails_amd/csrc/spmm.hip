// spmm.hip -- CSR x tall-skinny panel product Y = op(A) X for gfx950.
//
// Replaces `A_ * W` of the reference (src/LyapunovSolver.hpp:146), i.e.
// Epetra_CrsMatrix::Apply (src/Epetra_OperatorWrapper.cpp:87) / the dense DGEMM of the Stl
// path (src/StlWrapper.cpp:181).  HBM-bound integer/fp64 streaming work: no MFMA here.
//
// Data layout: panels are row-major (ld padded to 128 B), so one nonzero a_ij gathers ONE
// contiguous row segment X[j, c0:c0+nc] -- a single 1 KiB wave-wide dwordx4 load at nc = 128.
//
// In this file: the operator object (create, destroy, halo set-up, transpose), the row kernels with their launchers, and the dispatcher
// rails_spmm in stages: check_windows, apply_delegate, exchange_halo / overlapped_product for a row-partitioned operator, local_product.
// Which whole-operator kernel (sweep, planes, LDS-staged) a product tries before the row kernels, whether a row-partitioned product
// overlaps its exchange, and what rails_csr_prepare builds ahead are decided in one place, op_choice.h.
// Kernel 1 (row-gather): LPR lanes own one row; (col,val) of the row are group-uniform
// (scalar loads when LPR == 64), U = 8 X-row loads are kept in flight per lane.  1b / 1c: its chunked and lean forms, see there.
// Which of the three computes a product is decided in one place, row_choice.h.
// Kernel 2 (LDS-staged footprint, spmm_tiled.hip over the host plan of tile_plan.cpp): for matrices whose row blocks share columns
// (stencils, banded), the union of X rows a row block touches is staged once in LDS per
// column chunk and re-used by all rows of the block.
// The sweep kernel for banded patterns is in spmm_sweep.hip, the plane-sweep kernel for grid stencils in spmm_planes.hip.
#include "rails_internal.h"
#include "op_choice.h"
#include "row_choice.h"
#include "tile_plan.h"

#include <algorithm>

namespace {

typedef double double2_t __attribute__((ext_vector_type(2)));
typedef double2_t double2_a8_t __attribute__((aligned(8))); // 16-byte loads of two doubles that are only 8-byte aligned (odd column offsets)

template <int VEC>
struct Acc;
template <>
struct Acc<1> {
    double v;
    __device__ __forceinline__ void zero() { v = 0.0; }
    __device__ __forceinline__ void fma(double a, const double *x) { v = __builtin_fma(a, *x, v); }
    __device__ __forceinline__ void store(double *y) { *y = v; }
};
template <>
struct Acc<2> {
    double2_t v;
    __device__ __forceinline__ void zero() { v = (double2_t){0.0, 0.0}; }
    __device__ __forceinline__ void fma(double a, const double *x)
    {
        // (16-byte accesses that may be only 8-byte aligned -- windows on odd columns, odd panel strides: global memory asks for dword
        // alignment, and the instructions are the same ones)
        double2_t t = *reinterpret_cast<const double2_a8_t *>(x);
        v.x = __builtin_fma(a, t.x, v.x);
        v.y = __builtin_fma(a, t.y, v.y);
    }
    __device__ __forceinline__ void store(double *y) { *reinterpret_cast<double2_a8_t *>(y) = v; }
};

// One group of LPR lanes per row, RPG consecutive rows per group.
// Xg/ldg: ghost rows (column index >= m_local) for row-partitioned runs, else unused.
template <int LPR, int VEC, int RPG>
__global__ __launch_bounds__(256) void k_spmm_rowgather(int64_t m, const int64_t *__restrict__ rowptr,
                                                        const int32_t *__restrict__ col, const double *__restrict__ val,
                                                        const double *__restrict__ X, int ldx, const double *__restrict__ Xg,
                                                        int ldg, double *__restrict__ Y, int ldy, int nc, int64_t blocks_per_xcd, int64_t mc)
{
    // m rows (of this launch: the operator's, or a range of them -- rowptr and Y then start at the range); mc local columns: column
    // indices from mc on are ghost rows, taken from Xg
    constexpr int GROUPS = 256 / LPR;
    constexpr int U = 8;
    const int g = threadIdx.x / LPR;
    const int l = threadIdx.x % LPR;
    // XCD-aware block -> row-range map: blocks are dealt round-robin over the 8 XCDs (b and b+8 share one), so giving
    // XCD x the contiguous logical blocks [x*bpx, (x+1)*bpx) keeps the sliding window of gathered X rows of each XCD
    // inside its own 4 MiB L2 (speed only: any placement computes the same rows).
    int64_t lb = blockIdx.x;
    if (blocks_per_xcd > 0) lb = (int64_t)(blockIdx.x & 7) * blocks_per_xcd + (blockIdx.x >> 3);
    int64_t row_base = (lb * GROUPS + g) * RPG;
    if (LPR == 64) row_base = (lb * GROUPS + __builtin_amdgcn_readfirstlane(g)) * RPG;

    for (int rr = 0; rr < RPG; ++rr) {
        const int64_t row = row_base + rr;
        if (row >= m) break;
        const int64_t p0 = rowptr[row], p1 = rowptr[row + 1];
        for (int cb = l * VEC; cb < nc; cb += LPR * VEC) {
            const bool full = (cb + VEC <= nc);
            Acc<VEC> acc;
            acc.zero();
            double tail = 0.0; // VEC == 2 and only one valid column
            for (int64_t p = p0; p < p1; p += U) {
                int32_t c[U];
                double a[U];
                const int cnt = (int)((p1 - p) < U ? (p1 - p) : U);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const bool ok = u < cnt;
                    c[u] = col[ok ? p + u : p0];
                    a[u] = ok ? val[p + u] : 0.0;
                }
                const double *src[U];
#pragma unroll
                for (int u = 0; u < U; ++u)
                    src[u] = (c[u] < mc) ? (X + (int64_t)c[u] * ldx + cb) : (Xg + ((int64_t)c[u] - mc) * ldg + cb);
                if (full) {
#pragma unroll
                    for (int u = 0; u < U; ++u) acc.fma(a[u], src[u]);
                } else {
#pragma unroll
                    for (int u = 0; u < U; ++u) tail = __builtin_fma(a[u], *src[u], tail);
                }
            }
            double *dst = Y + row * ldy + cb;
            if (full)
                acc.store(dst);
            else
                *dst = tail;
        }
    }
}

__global__ void k_pack_rows(const int64_t *__restrict__ rows, int64_t n, const double *__restrict__ X, int ldx, int nc,
                            double *__restrict__ out)
{
    int64_t total = n * nc;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        int64_t i = idx / nc;
        int cidx = (int)(idx - i * nc);
        out[idx] = X[rows[i] * ldx + cidx];
    }
}

// rows [r0, r0 + nrows) of the operator on stream st (defaults: all rows, the context's stream).  A span is how the row-partitioned
// product overlaps its halo exchange: interior rows on a second stream while the ghost rows travel, boundary rows afterwards.
struct RowSpan {
    int64_t r0 = 0, nrows = -1;
    hipStream_t st = nullptr;
};
// (the busy meter brackets launches on the context's stream only)
#define RAILS_LAUNCH_ON(st__, kern__, grid__, block__, lds__, ...)                           \
    do {                                                                                     \
        if ((st__) == c->stream)                                                             \
            RAILS_LAUNCH(kern__, grid__, block__, lds__, c->stream, __VA_ARGS__);            \
        else                                                                                 \
            hipLaunchKernelGGL(kern__, grid__, block__, lds__, (st__), __VA_ARGS__);        \
    } while (0)

template <int LPR, int VEC>
int launch_rg(rails_ctx *c, const rails_csr *A, const double *X, int ldx, const double *Xg, int ldg, double *Y, int ldy, int nc, const RowSpan &sp)
{
    const int64_t m_rows = sp.nrows < 0 ? A->m : sp.nrows;
    hipStream_t st = sp.st ? sp.st : c->stream;
    constexpr int GROUPS = 256 / LPR;
    constexpr int RPG = (LPR >= 32) ? 4 : 2;
    int64_t rows_per_block = (int64_t)GROUPS * RPG;
    int64_t grid = (m_rows + rows_per_block - 1) / rows_per_block;
    static const int xcd_aware = spmm_env("RAILS_SPMM_XCD", 1);
    int64_t bpx = 0;
    if (xcd_aware && grid >= 64) {
        bpx = (grid + 7) / 8;
        grid = bpx * 8;
    }
    RAILS_REQUIRE(grid <= 0x7fffffffLL, "rails_spmm: grid too large");
    RAILS_LAUNCH_ON(st, (k_spmm_rowgather<LPR, VEC, RPG>), dim3((unsigned)grid), dim3(256), 0, m_rows, A->rowptr + sp.r0, A->col,
                    A->val, X, ldx, Xg, ldg, Y + sp.r0 * ldy, ldy, nc, bpx, A->m);
    return RAILS_OK;
}


// Kernel 1b (row-gather, column chunks inside one launch): for wide X (nc = 128) the sliding window of X rows that the
// row blocks of one XCD gather from (window_rows x nc x 8 B: 8 MiB for |j-i| <= 4096) does not fit the XCD's 4 MiB L2 and
// two thirds of the gathers miss it.  Here the panel is cut into chunks of CC = 2*LPR columns and every XCD walks its
// row range once per chunk (blocks are dealt to the XCDs round-robin and, per XCD, in launch order: chunk-major), so the
// window is window_rows x CC x 8 B and the gathers hit L2.  LPR lanes own a row (4 rows per wave at CC = 32); the block's
// (col, val) run is staged in LDS once so that the per-nonzero loads are LDS broadcasts instead of vector-memory loads.
template <int LPR, int RPG>
__global__ __launch_bounds__(256) void k_spmm_rowgather_cc(int64_t m, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                           const double *__restrict__ val, const double *__restrict__ X, int ldx,
                                                           const double *__restrict__ Xg, int ldg, double *__restrict__ Y, int ldy, int nc,
                                                           int64_t blocks_per_xcd, int lds_cap, int y_vec, int64_t mc)
{
    constexpr int GROUPS = 256 / LPR;
    constexpr int ROWS = GROUPS * RPG;
    constexpr int CC = 2 * LPR;
    constexpr int U = 8;
    extern __shared__ double smem[];
    double *s_val = smem;
    int32_t *s_col = reinterpret_cast<int32_t *>(smem + lds_cap);
    const int g = threadIdx.x / LPR;
    const int l = threadIdx.x % LPR;
    const int64_t s = blockIdx.x >> 3;
    const int chunk = (int)(s / blocks_per_xcd);
    const int64_t lb = (int64_t)(blockIdx.x & 7) * blocks_per_xcd + (s - (int64_t)chunk * blocks_per_xcd);
    const int64_t r0 = lb * ROWS;
    if (r0 >= m) return;
    const int64_t r1 = (r0 + ROWS < m) ? r0 + ROWS : m;
    const int64_t nz0 = rowptr[r0], nz1 = rowptr[r1];
    const bool staged = (nz1 - nz0) <= lds_cap; // block-uniform
    if (staged) {
        for (int64_t q = nz0 + threadIdx.x; q < nz1; q += 256) {
            s_col[q - nz0] = col[q];
            s_val[q - nz0] = val[q];
        }
        __syncthreads();
    }
    const int cb = chunk * CC + l * 2;
    if (cb >= nc) return;
    const bool full = (cb + 2 <= nc);
    for (int rr = 0; rr < RPG; ++rr) {
        const int64_t row = r0 + (int64_t)rr * GROUPS + g; // the 256/LPR rows in flight are consecutive
        if (row >= m) break;
        const int64_t p0 = rowptr[row], p1 = rowptr[row + 1];
        double2_t acc = (double2_t){0.0, 0.0};
        for (int64_t p = p0; p < p1; p += U) {
            int32_t c[U];
            double a[U];
            const int cnt = (int)((p1 - p) < U ? (p1 - p) : U);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool ok = u < cnt;
                const int64_t q = ok ? p + u : p0;
                c[u] = staged ? s_col[q - nz0] : col[q];
                const double av = staged ? s_val[q - nz0] : val[q];
                a[u] = ok ? av : 0.0;
            }
            if (full) {
                double2_t x[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const double *src = (c[u] < mc) ? (X + (int64_t)c[u] * ldx + cb) : (Xg + ((int64_t)c[u] - mc) * ldg + cb);
                    x[u] = *reinterpret_cast<const double2_t *>(src);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    acc.x = __builtin_fma(a[u], x[u].x, acc.x);
                    acc.y = __builtin_fma(a[u], x[u].y, acc.y);
                }
            } else {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const double *src = (c[u] < mc) ? (X + (int64_t)c[u] * ldx + cb) : (Xg + ((int64_t)c[u] - mc) * ldg + cb);
                    acc.x = __builtin_fma(a[u], *src, acc.x);
                }
            }
        }
        double *dst = Y + row * ldy + cb;
        if (full && y_vec)
            *reinterpret_cast<double2_t *>(dst) = acc;
        else if (full) { // Y window starts on an odd column: two 8-byte stores
            dst[0] = acc.x;
            dst[1] = acc.y;
        } else
            *dst = acc.x;
    }
}

// Kernel 1c: the in-loop product A * W at Expand size <= 16 on operators whose X rows are all addressable as X + c * ldx with 32-bit
// byte offsets (no ghost rows, panel below 4 GiB, fewer than 2^24 rows).  Same scheme as kernel 1b with one chunk -- 8 lanes own a row,
// the block's (col, val) run staged in LDS -- but the per-nonzero work is cut to what the product needs: two LDS broadcasts, one
// 24-bit multiply-add for the byte offset, one 16-byte load with a scalar base, two multiply-adds.  Kernel 1b spends ~37 vector
// instructions per nonzero on 64-bit addresses, the ghost-row select and the masks of its tail and ran at the instruction rate
// (rocprofv3 --pmc: 2000 VALU instructions per wave of 16 rows, TA and L2 far from busy): 0.40 ms at 16 columns, 18 % of the HBM rate.
template <int RPG, bool GHOST, int LPR = 8>
__global__ __launch_bounds__(256) void k_spmm_narrow(int64_t m, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                     const double *__restrict__ val, const double *__restrict__ X, uint32_t ldx8,
                                                     const double *__restrict__ Xg, uint32_t ldg8, double *__restrict__ Y, int ldy, int nc,
                                                     int64_t blocks_per_xcd, int y_vec, int64_t mc)
{
    constexpr int GROUPS = 256 / LPR, ROWS = GROUPS * RPG, CAP = 2048; // LPR lanes own a row: 16 columns with 8, 32 with 16
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
    const uint32_t cb8 = (uint32_t)cb * 8u, m32 = (uint32_t)mc;
    const char *Xb = reinterpret_cast<const char *>(X), *Gb = reinterpret_cast<const char *>(Xg);
    // the address of this lane's two columns of X row c: local rows from the panel, ghost rows (c >= m, row-partitioned runs) from the
    // buffer the halo exchange filled -- a select between two bases and two strides, still 32-bit offsets
    auto xrow = [&](uint32_t c) -> const char * {
        if (!GHOST) return Xb + (__umul24(c, ldx8) + cb8);
        const bool local = c < m32;
        return (local ? Xb : Gb) + ((local ? __umul24(c, ldx8) : __umul24(c - m32, ldg8)) + cb8);
    };
    for (int rr = 0; rr < RPG; ++rr) {
        const int64_t row = r0 + (int64_t)rr * GROUPS + g; // the 32 rows in flight are consecutive
        if (row >= m) break;
        double2_t acc = (double2_t){0.0, 0.0};
        if (staged && full) {
            int i = (int)(rowptr[row] - nz0);
            const int i1 = (int)(rowptr[row + 1] - nz0);
            for (; i + 8 <= i1; i += 8) {
                double2_t x[8];
                double a[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    x[u] = *reinterpret_cast<const double2_a8_t *>(xrow((uint32_t)s_col[i + u]));
                    a[u] = s_val[i + u];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    acc.x = __builtin_fma(a[u], x[u].x, acc.x);
                    acc.y = __builtin_fma(a[u], x[u].y, acc.y);
                }
            }
            for (; i < i1; i += 4) { // the last one to seven: groups of four, the slots past the end repeat the last entry with a zero
                double2_t x[4];
                double a[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int q = i + u < i1 ? i + u : i1 - 1;
                    x[u] = *reinterpret_cast<const double2_a8_t *>(xrow((uint32_t)s_col[q]));
                    a[u] = i + u < i1 ? s_val[q] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    acc.x = __builtin_fma(a[u], x[u].x, acc.x);
                    acc.y = __builtin_fma(a[u], x[u].y, acc.y);
                }
            }
        } else {
            // (a block with more nonzeros than the LDS buffer holds, or the lane of an odd last column: one entry at a time)
            for (int64_t p = rowptr[row]; p < rowptr[row + 1]; ++p) {
                const double a = val[p];
                const double *src = reinterpret_cast<const double *>(xrow((uint32_t)col[p]));
                acc.x = __builtin_fma(a, src[0], acc.x);
                if (full) acc.y = __builtin_fma(a, src[1], acc.y);
            }
        }
        double *dst = Y + row * ldy + cb;
        if (full && y_vec)
            *reinterpret_cast<double2_t *>(dst) = acc;
        else if (full) { // Y window starts on an odd column: two 8-byte stores
            dst[0] = acc.x;
            dst[1] = acc.y;
        } else
            *dst = acc.x;
    }
}

// the kernels that give a block of 64 consecutive rows to a workgroup: the chunked one (1b), or -- where the choice says that its one
// chunk can have it -- the lean one (1c); LPR = 8 / 16 / 32 lanes per row for chunks of 16 / 32 / 64 columns (the lean kernel: 8 or 16)
template <int LPR>
int launch_rg_cc(rails_ctx *c, const rails_csr *A, const RowChoice &ch, const double *X, int ldx, const double *Xg, int ldg, double *Y, int ldy, int nc,
                 const RowSpan &sp)
{
    const int64_t m_rows = sp.nrows < 0 ? A->m : sp.nrows;
    hipStream_t st = sp.st ? sp.st : c->stream;
    const int64_t *rowptr = A->rowptr + sp.r0;
    Y += sp.r0 * ldy;
    constexpr int GROUPS = 256 / LPR;
    constexpr int RPG = (LPR >= 32) ? 8 : (LPR >= 16 ? 4 : 2);
    constexpr int ROWS = GROUPS * RPG; // 64 rows per block
    constexpr int CC = 2 * LPR;
    constexpr int NLPR = LPR == 16 ? 16 : 8;
    const int nchunks = (nc + CC - 1) / CC;
    const int64_t blocks = (m_rows + ROWS - 1) / ROWS;
    const int64_t bpx = (blocks + 7) / 8;
    const int64_t grid = bpx * 8 * nchunks;
    RAILS_REQUIRE(grid <= 0x7fffffffLL, "rails_spmm: grid too large");
    const int y_vec = ch.y_vec ? 1 : 0;
    if (ch.kind == RowChoice::NARROW && !ch.ghost)
        RAILS_LAUNCH_ON(st, (k_spmm_narrow<RPG, false, NLPR>), dim3((unsigned)grid), dim3(256), 0, m_rows, rowptr, A->col, A->val, X, (uint32_t)ldx * 8u, X, 0u, Y, ldy, nc,
                        bpx, y_vec, A->m);
    else if (ch.kind == RowChoice::NARROW) // row-partitioned runs: columns >= m are ghost rows in the halo buffer (16-byte aligned rows there too)
        RAILS_LAUNCH_ON(st, (k_spmm_narrow<RPG, true, NLPR>), dim3((unsigned)grid), dim3(256), 0, m_rows, rowptr, A->col, A->val, X, (uint32_t)ldx * 8u, Xg,
                        (uint32_t)ldg * 8u, Y, ldy, nc, bpx, y_vec, A->m);
    else {
        const int lds_cap = 2048; // nonzeros of one block staged in LDS (24 KiB); longer runs read (col, val) from global memory
        RAILS_LAUNCH_ON(st, (k_spmm_rowgather_cc<LPR, RPG>), dim3((unsigned)grid), dim3(256), (size_t)lds_cap * 12, m_rows, rowptr, A->col, A->val, X, ldx, Xg, ldg, Y,
                        ldy, nc, bpx, lds_cap, y_vec, A->m);
    }
    return RAILS_OK;
}

template <int VEC>
int dispatch_rg(rails_ctx *c, const rails_csr *A, int lpr, const double *X, int ldx, const double *Xg, int ldg, double *Y, int ldy, int nc, const RowSpan &sp)
{
    switch (lpr) {
    case 64: return launch_rg<64, VEC>(c, A, X, ldx, Xg, ldg, Y, ldy, nc, sp);
    case 32: return launch_rg<32, VEC>(c, A, X, ldx, Xg, ldg, Y, ldy, nc, sp);
    case 16: return launch_rg<16, VEC>(c, A, X, ldx, Xg, ldg, Y, ldy, nc, sp);
    case 8: return launch_rg<8, VEC>(c, A, X, ldx, Xg, ldg, Y, ldy, nc, sp);
    case 4: return launch_rg<4, VEC>(c, A, X, ldx, Xg, ldg, Y, ldy, nc, sp);
    case 2: return launch_rg<2, VEC>(c, A, X, ldx, Xg, ldg, Y, ldy, nc, sp);
    default: return launch_rg<1, VEC>(c, A, X, ldx, Xg, ldg, Y, ldy, nc, sp);
    }
}

// The facts rails_row_choice (row_choice.h) decides on.  Whole width is the automatic choice at every panel width: measured on MI355X
// at nc = 128 (profiles/r01_spmm_chunked.md), chunking removes the L2 misses as intended (banded |j-i| <= 4096: 18.7 GB -> 3.1 GB of L2
// fills per product) but the product does not get faster (2.34 -> 2.6 ms): the 27.6 GB of gathered row segments are bounded by
// L2 -> L1 throughput (~12 TB/s), not by the fabric.  The chunked kernel stays selectable (variants 4/5, RAILS_SPMM_CHUNK).  Narrow
// panels: (col, val) of a 64-row block staged in LDS instead of per-lane vector-memory loads -- kernel 1c where every X row is within
// 32-bit byte offsets (0.24 vs 0.45 ms at 16 columns, 0.44 vs 0.71 ms at 32, banded pattern), kernel 1b otherwise
// (RAILS_SPMM_NARROW_CC=0 disables both).
struct NarrowEnv {
    bool cc, fast;
};
const NarrowEnv &narrow_env() // (read once)
{
    static const NarrowEnv e = {spmm_env("RAILS_SPMM_NARROW_CC", 1) != 0, spmm_env("RAILS_SPMM_NARROW_FAST", 1) != 0};
    return e;
}

RowFacts row_facts(const rails_csr *A, int nc, bool x_vec2, bool y_vec2, bool vec2, const double *X, int ldx, const double *Xg, int ldg, int span_ghost)
{
    static const int chunk_env = spmm_env("RAILS_SPMM_CHUNK", 0);
    RowFacts f;
    f.variant = A->variant; f.max_row_nnz = A->max_row_nnz; f.m = A->m; f.ncols_ext = A->ncols_ext; f.n_ghost = A->n_ghost; f.rect = A->rect;
    f.nc = nc; f.x_vec2 = x_vec2; f.y_vec2 = y_vec2; f.vec2 = vec2; f.ldx = ldx; f.ldg = ldg;
    f.xg_is_tail = Xg == X + (int64_t)A->m * ldx;
    f.span_ghost = span_ghost;
    f.narrow_cc = narrow_env().cc; f.narrow_fast = narrow_env().fast; f.chunk_env = chunk_env;
    return f;
}

const char *const ROW_KERNEL[3] = {"k_spmm_rowgather", "k_spmm_rowgather_cc", "k_spmm_narrow"}; // by RowChoice::Kind

// Launches what was chosen (ROW_KERNEL[ch.kind] is its name) for the rows of a span (default: all rows, the context's stream).
int launch_rows(rails_ctx *c, const rails_csr *A, const RowChoice &ch, const double *X, int ldx, const double *Xg, int ldg, double *Y, int ldy, int nc,
                const RowSpan &sp = RowSpan())
{
    if (ch.kind == RowChoice::PLAIN)
        return ch.vec == 2 ? dispatch_rg<2>(c, A, ch.lpr, X, ldx, Xg, ldg, Y, ldy, nc, sp) : dispatch_rg<1>(c, A, ch.lpr, X, ldx, Xg, ldg, Y, ldy, nc, sp);
    if (ch.lpr == 8) return launch_rg_cc<8>(c, A, ch, X, ldx, Xg, ldg, Y, ldy, nc, sp);
    if (ch.lpr == 16) return launch_rg_cc<16>(c, A, ch, X, ldx, Xg, ldg, Y, ldy, nc, sp);
    return launch_rg_cc<32>(c, A, ch, X, ldx, Xg, ldg, Y, ldy, nc, sp);
}

// The rows of a span of the halo-overlapped product (an empty span launches nothing).
int spmm_span(rails_ctx *c, const rails_csr *A, const RowChoice &ch, const double *X, int ldx, const double *Xg, int ldg, double *Y, int ldy, int nc,
              const RowSpan &sp)
{
    return sp.nrows <= 0 ? RAILS_OK : launch_rows(c, A, ch, X, ldx, Xg, ldg, Y, ldy, nc, sp);
}

// mean of (max col - min col + 1) over a sample of about 4096 of the rows [r0, r1) (rows without entries aside): the sliding window of
// X rows a row block gathers from
int64_t mean_row_window(const int64_t *rowptr, const int32_t *col, int64_t r0, int64_t r1)
{
    const int64_t stride = std::max<int64_t>(1, (r1 - r0) / 4096);
    int64_t sum = 0, cnt = 0;
    for (int64_t i = r0; i < r1; i += stride) {
        if (rowptr[i + 1] == rowptr[i]) continue;
        int32_t lo = col[rowptr[i]], hi = lo;
        for (int64_t q = rowptr[i]; q < rowptr[i + 1]; ++q) {
            lo = std::min(lo, col[q]);
            hi = std::max(hi, col[q]);
        }
        sum += (int64_t)hi - lo + 1;
        cnt++;
    }
    return cnt ? sum / cnt : 0;
}

int build_transpose(rails_csr *A)
{
    if (A->AT) return RAILS_OK;
    RAILS_REQUIRE(A->n_ghost == 0 && A->ncols_ext == A->m, "rails_spmm: transposed apply is single-GPU only");
    const int64_t m = A->m, nnz = A->nnz;
    std::vector<int64_t> rp(m + 1, 0);
    for (int64_t p = 0; p < nnz; ++p) rp[A->h_col[p] + 1]++;
    for (int64_t i = 0; i < m; ++i) rp[i + 1] += rp[i];
    std::vector<int32_t> ci(nnz);
    std::vector<double> va(nnz);
    std::vector<int64_t> next(rp.begin(), rp.end() - 1);
    for (int64_t i = 0; i < m; ++i)
        for (int64_t p = A->h_rowptr[i]; p < A->h_rowptr[i + 1]; ++p) {
            int64_t q = next[A->h_col[p]]++;
            ci[q] = (int32_t)i;
            va[q] = A->h_val[p];
        }
    return rails_csr_create(A->ctx, m, m, rp.data(), ci.data(), va.data(), &A->AT);
}

} // namespace

extern "C" int rails_csr_create(rails_ctx *c, int64_t m_local, int64_t n_cols_ext, const int64_t *rowptr, const int32_t *col,
                                const double *val, rails_csr **out)
{
    if (c) hipSetDevice(c->device); // allocations and launches go to the context's device whatever the caller's current device is
    RAILS_REQUIRE(c && out && rowptr, "rails_csr_create: null argument");
    RAILS_REQUIRE(m_local >= 0 && n_cols_ext >= 0 && n_cols_ext <= 0x7fffffffLL, "rails_csr_create: bad shape %lld x %lld",
                  (long long)m_local, (long long)n_cols_ext);
    RAILS_REQUIRE(rowptr[0] == 0, "rails_csr_create: rowptr[0] != 0");
    int64_t nnz = rowptr[m_local];
    RAILS_REQUIRE(nnz >= 0 && (nnz == 0 || (col && val)), "rails_csr_create: bad nnz / null arrays");
    int maxrow = 0;
    for (int64_t i = 0; i < m_local; ++i) {
        int64_t d = rowptr[i + 1] - rowptr[i];
        RAILS_REQUIRE(d >= 0 && d <= 0x7fffffffLL, "rails_csr_create: rowptr not monotone at row %lld", (long long)i);
        if (d > maxrow) maxrow = (int)d;
    }
    // host-side index validation: an out-of-range column would fault the kernel
    for (int64_t p = 0; p < nnz; ++p)
        RAILS_REQUIRE(col[p] >= 0 && col[p] < n_cols_ext, "rails_csr_create: column %d out of range at nz %lld", col[p], (long long)p);
    rails_csr *A = new rails_csr();
    A->ctx = c;
    A->m = m_local;
    A->ncols_ext = n_cols_ext;
    A->nnz = nnz;
    A->max_row_nnz = maxrow;
    A->window_rows = mean_row_window(rowptr, col, 0, m_local);
    A->h_rowptr.assign(rowptr, rowptr + m_local + 1);
    if (nnz) {
        A->h_col.assign(col, col + nnz);
        A->h_val.assign(val, val + nnz);
    }
    hipError_t e1 = hipMalloc((void **)&A->rowptr, (size_t)(m_local + 1) * sizeof(int64_t));
    hipError_t e2 = hipMalloc((void **)&A->col, (size_t)(nnz ? nnz : 1) * sizeof(int32_t));
    hipError_t e3 = hipMalloc((void **)&A->val, (size_t)(nnz ? nnz : 1) * sizeof(double));
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) {
        rails_set_error("rails_csr_create: device allocation failed");
        rails_csr_destroy(A);
        return RAILS_ENOMEM;
    }
    hipError_t ce = hipMemcpyAsync(A->rowptr, rowptr, (size_t)(m_local + 1) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream);
    if (ce == hipSuccess && nnz) ce = hipMemcpyAsync(A->col, col, (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice, c->stream);
    if (ce == hipSuccess && nnz) ce = hipMemcpyAsync(A->val, val, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice, c->stream);
    if (ce == hipSuccess) ce = rails_stream_sync(c);
    if (ce != hipSuccess) { // the half-made operator is released, not leaked
        rails_set_error("rails_csr_create: upload failed: %s", hipGetErrorString(ce));
        rails_csr_destroy(A);
        return RAILS_EHIP;
    }
    *out = A;
    return RAILS_OK;
}

extern "C" int rails_csr_create_callback(rails_ctx *c, int64_t m_local, rails_apply_fn fn, void *user, rails_csr **out)
{
    RAILS_REQUIRE(c && out && fn && m_local >= 0, "rails_csr_create_callback: bad argument");
    rails_csr *A = new rails_csr();
    A->ctx = c;
    A->m = m_local;
    A->ncols_ext = m_local;
    A->kind = rails_csr::CALLBACK;
    A->apply_fn = fn;
    A->delegate = user;
    A->last_kernel = "callback";
    *out = A;
    return RAILS_OK;
}

extern "C" int rails_csr_destroy(rails_csr *A)
{
    if (!A) return RAILS_OK;
    hipStreamSynchronize(A->ctx->stream);
    if (A->AT) rails_csr_destroy(A->AT);
    rails_sweep_release(A);
    rails_planes_release(A);
    rails_tiled_release(A);
    rails_bsr_release(A);
    if (A->rowptr) hipFree(A->rowptr);
    if (A->col) hipFree(A->col);
    if (A->val) hipFree(A->val);
    if (A->send_rows) hipFree(A->send_rows);
    if (A->send_buf) hipFree(A->send_buf);
    if (A->ext) hipFree(A->ext);
    delete A;
    return RAILS_OK;
}

extern "C" int64_t rails_csr_rows(const rails_csr *A) { return A ? A->m : -1; }
extern "C" int64_t rails_csr_nnz(const rails_csr *A) { return A ? A->nnz : -1; }
extern "C" const char *rails_csr_last_kernel(const rails_csr *A) { return A ? A->last_kernel : ""; }

// n_rows x n_cols with all columns local: X of a product has n_cols rows, Y n_rows.  The blocks A12, A21 of a Schur complement
// (src/SchurOperator.cpp:181-214) are of this kind.  Plain row-gather kernels only (the tile and sweep plans assume a square operator).
extern "C" int rails_csr_create_rect(rails_ctx *c, int64_t n_rows, int64_t n_cols, const int64_t *rowptr, const int32_t *col, const double *val,
                                     rails_csr **out)
{
    RAILS_REQUIRE(n_cols >= 1, "rails_csr_create_rect: no columns");
    RAILS_TRY(rails_csr_create(c, n_rows, n_cols, rowptr, col, val, out));
    (*out)->rect = true;
    (*out)->variant = 1;
    return RAILS_OK;
}

extern "C" int rails_csr_set_variant(rails_csr *A, int variant)
{
    RAILS_REQUIRE(A && variant >= 0 && variant <= 9, "rails_csr_set_variant: bad argument");
    if (A->rect) return RAILS_OK; // rectangular operators stay on the plain row-gather kernel
    A->variant = variant;
    return RAILS_OK;
}

extern "C" int rails_csr_set_halo_counts(rails_csr *A, int nranks, const int64_t *send_counts, const int64_t *recv_counts)
{
    RAILS_REQUIRE(A && nranks >= 1 && send_counts && recv_counts, "rails_csr_set_halo_counts: bad argument");
    int64_t ns = 0, nr = 0;
    for (int r = 0; r < nranks; ++r) {
        RAILS_REQUIRE(send_counts[r] >= 0 && recv_counts[r] >= 0, "rails_csr_set_halo_counts: negative count");
        ns += send_counts[r];
        nr += recv_counts[r];
    }
    RAILS_REQUIRE(ns == A->n_send && nr == A->n_ghost, "rails_csr_set_halo_counts: counts add up to %lld sent / %lld received rows, the plan has %lld / %lld",
                  (long long)ns, (long long)nr, (long long)A->n_send, (long long)A->n_ghost);
    A->send_counts.assign(send_counts, send_counts + nranks);
    A->recv_counts.assign(recv_counts, recv_counts + nranks);
    return RAILS_OK;
}

extern "C" int rails_csr_set_halo(rails_csr *A, int64_t n_send, const int64_t *send_rows, int64_t n_ghost, rails_halo_fn fn,
                                  void *user)
{
    RAILS_REQUIRE(A, "null operator");
    static const char *const single_gpu_only[] = {nullptr, nullptr, "an LU solve operator", "a sparse right-hand side", "an iterative solve operator", "a block-CSR operator"}; // by rails_csr::Kind
    RAILS_REQUIRE(!single_gpu_only[A->kind], "rails_csr_set_halo: %s is single GPU only", single_gpu_only[A->kind]);
    RAILS_REQUIRE(n_send >= 0 && n_ghost >= 0 && A->m + n_ghost == A->ncols_ext,
                  "rails_csr_set_halo: m_local %lld + ghosts %lld != extended columns %lld", (long long)A->m, (long long)n_ghost,
                  (long long)A->ncols_ext);
    RAILS_REQUIRE((n_send == 0 && n_ghost == 0) || fn || A->ctx->rccl,
                  "rails_csr_set_halo: neither a halo hook nor an RCCL communicator on the context (rails_ctx_init_rccl)");
    for (int64_t i = 0; i < n_send; ++i)
        RAILS_REQUIRE(send_rows[i] >= 0 && send_rows[i] < A->m, "rails_csr_set_halo: send row %lld out of range", (long long)send_rows[i]);
    rails_ctx *c = A->ctx;
    if (A->send_rows) {
        RAILS_HIP_CHECK(rails_stream_sync(c));
        RAILS_HIP_CHECK(hipFree(A->send_rows));
        A->send_rows = nullptr;
    }
    A->n_send = n_send;
    A->n_ghost = n_ghost;
    A->halo = fn;
    A->halo_user = user;
    // the interior rows: the contiguous range in the middle of the block whose rows reference no ghost column (row blocks of banded and
    // grid operators keep their boundary rows at the two ends).  Their product does not wait for the exchange (rails_spmm).
    A->int_lo = 0;
    A->int_hi = A->m;
    if (n_ghost > 0) {
        const int64_t m = A->m, mid = m / 2;
        for (int64_t r = 0; r < m; ++r) {
            bool boundary = false;
            for (int64_t p2 = A->h_rowptr[r]; p2 < A->h_rowptr[r + 1] && !boundary; ++p2) boundary = A->h_col[p2] >= m;
            if (!boundary) continue;
            if (r < mid)
                A->int_lo = r + 1;
            else {
                A->int_hi = r;
                break;
            }
        }
        // the sliding window of the interior rows alone (the boundary rows' ghost columns sit behind the local ones: they would inflate it)
        A->window_rows_int = mean_row_window(A->h_rowptr.data(), A->h_col.data(), A->int_lo, A->int_hi);
    }
    if (n_send) {
        RAILS_HIP_CHECK(hipMalloc((void **)&A->send_rows, (size_t)n_send * sizeof(int64_t)));
        RAILS_HIP_CHECK(hipMemcpy(A->send_rows, send_rows, (size_t)n_send * sizeof(int64_t), hipMemcpyHostToDevice));
    }
    return RAILS_OK;
}

// structured-grid stencil (the territory of the plane-sweep and LDS-staged box kernels)?  Looked at once
static bool rails_csr_is_grid(rails_csr *A)
{
    if (A->is_grid < 0) {
        int64_t gx = 0, gy = 0, gz = 0;
        A->is_grid = (spmm_env("RAILS_SPMM_TILE_BOX", 1) && rails_detect_grid(A->m, A->h_rowptr.data(), A->h_col.data(), &gx, &gy, &gz)) ? 1 : 0;
    }
    return A->is_grid == 1;
}

// The facts op_choice.h decides on.  RAILS_SPMM_HALO_OVERLAP and RAILS_SPMM_PLANES are read per product (the tests switch the first inside
// one process), the other switches once.
OpFacts rails_op_facts(const rails_ctx *c, const rails_csr *A, int nc, bool x_vec2, bool y_vec2)
{
    OpFacts f;
    f.variant = A->variant; f.max_row_nnz = A->max_row_nnz; f.m = A->m; f.ncols_ext = A->ncols_ext; f.n_ghost = A->n_ghost; f.rect = A->rect;
    f.window_rows = A->window_rows; f.window_rows_int = A->window_rows_int; f.int_lo = A->int_lo; f.int_hi = A->int_hi;
    f.nc = nc; f.x_vec2 = x_vec2; f.y_vec2 = y_vec2;
    f.num_cu = c->num_cu;
    f.planes = spmm_env("RAILS_SPMM_PLANES", 1) != 0; f.halo_overlap = spmm_env("RAILS_SPMM_HALO_OVERLAP", 1) != 0;
    f.narrow_cc = narrow_env().cc; f.narrow_fast = narrow_env().fast;
    return f;
}

extern "C" int rails_csr_prepare(rails_ctx *c, rails_csr *A, int trans, int nc, int *kernel_ready)
{
    RAILS_REQUIRE(c && A && nc >= 1, "rails_csr_prepare: bad argument");
    if (kernel_ready) *kernel_ready = 0;
    if (A->kind != rails_csr::STORED) return RAILS_OK;
    if (trans) {
        RAILS_TRY(build_transpose(A));
        A->AT->variant = A->variant;
        return rails_csr_prepare(c, A->AT, 0, nc, kernel_ready);
    }
    // what the products of that width would take, between aligned windows
    bool fits = false;
    switch (rails_prepare_choice(rails_op_facts(c, A, nc, true, true), [&] { return rails_csr_is_grid(A); })) {
    case PrepareChoice::SWEEP: RAILS_TRY(rails_sweep_prepare(c, A, nc, &fits)); break;
    case PrepareChoice::SWEEP_INTERIOR: RAILS_TRY(rails_sweep_prepare_interior(c, A, nc, &fits)); break; // row-partitioned: the schedule of the interior rows
    case PrepareChoice::NONE: break;
    }
    if (kernel_ready) *kernel_ready = fits ? 1 : 0;
    return RAILS_OK;
}

namespace {

// One product's operands: the windows of X and Y, and where the columns beyond the operator's rows come from.
struct Product {
    const rails_panel *X;
    rails_panel *Y;
    int xc0, yc0, nc;
    const double *Xp; // X->d + xc0
    double *Yp;       // Y->d + yc0
    const double *Xg; // ghost rows, leading dimension ldg
    int ldg;
};

int check_windows(const rails_csr *A, int trans, const rails_panel *X, int xc0, int nc, const rails_panel *Y, int yc0)
{
    RAILS_REQUIRE(xc0 >= 0 && nc >= 0 && xc0 + nc <= X->cap, "rails_spmm: X columns [%d,%d) outside capacity %d", xc0, xc0 + nc, X->cap);
    RAILS_REQUIRE(yc0 >= 0 && yc0 + nc <= Y->cap, "rails_spmm: Y columns [%d,%d) outside capacity %d", yc0, yc0 + nc, Y->cap);
    RAILS_REQUIRE(X->m == (A->rect ? A->ncols_ext : A->m) && Y->m == A->m, "rails_spmm: operator is %lld x %lld, X has %lld rows, Y %lld", (long long)A->m,
                  (long long)(A->rect ? A->ncols_ext : A->m), (long long)X->m, (long long)Y->m);
    RAILS_REQUIRE(!(A->rect && trans), "rails_spmm: a rectangular operator has no transposed apply (create the transposed matrix)");
    if (X->d == Y->d) RAILS_REQUIRE(xc0 + nc <= yc0 || yc0 + nc <= xc0, "rails_spmm: X and Y windows alias");
    return RAILS_OK;
}

// An operator that is not a stored matrix: the panels go to its delegate.
int apply_delegate(rails_ctx *c, rails_csr *A, int trans, const rails_panel *X, int xc0, int nc, rails_panel *Y, int yc0)
{
    switch (A->kind) {
    case rails_csr::SPRHS: return rails_sprhs_apply(c, A->sprhs(), trans, X, xc0, nc, Y, yc0);
    case rails_csr::LU: return rails_lu_solve(c, A->lu(), trans, X, xc0, nc, Y, yc0);
    case rails_csr::ITER: return rails_iter_solve(c, A->iter(), trans, X, xc0, nc, Y, yc0);
    case rails_csr::BSR: return rails_bsr_apply(c, A, trans, X, xc0, nc, Y, yc0);
    default: break;
    }
    int rc = A->apply_fn(A->delegate, trans ? 1 : 0, X, xc0, nc, Y, yc0);
    if (rc != 0) {
        rails_set_error("rails_spmm: the operator callback failed with code %d", rc);
        return RAILS_ECOMM;
    }
    c->n_spmm_callback++;
    return RAILS_OK;
}

// a device buffer of the operator that only grows (the stream may still read the old one)
int grow_buffer(rails_ctx *c, double **buf, size_t *cap, size_t bytes)
{
    if (bytes <= *cap) return RAILS_OK;
    RAILS_HIP_CHECK(rails_stream_sync(c));
    if (*buf) RAILS_HIP_CHECK(hipFree(*buf));
    *buf = nullptr;
    RAILS_HIP_CHECK(hipMalloc((void **)buf, bytes));
    *cap = bytes;
    return RAILS_OK;
}

// Packs the rows the neighbours need and exchanges: afterwards (in stream order) A->ext holds the ghost rows, nc columns wide.
int exchange_halo(rails_ctx *c, rails_csr *A, const double *Xp, int ldx, int nc)
{
    if (A->n_send) {
        int64_t total = A->n_send * nc;
        int grid = (int)std::min<int64_t>((total + 255) / 256, (int64_t)c->num_cu * 8);
        RAILS_LAUNCH(k_pack_rows, dim3(grid), dim3(256), 0, c->stream, A->send_rows, A->n_send, Xp, ldx, nc, A->send_buf);
    }
    if (A->halo) {
        int rc = A->halo(A->halo_user, A->send_buf, A->ext, nc, (void *)c->stream);
        if (rc != 0) {
            rails_set_error("rails_spmm: halo hook failed with code %d", rc);
            return RAILS_ECOMM;
        }
        return RAILS_OK;
    }
    RAILS_REQUIRE(c->rccl, "rails_spmm: ghost rows but neither a halo hook nor an RCCL communicator");
    return rails_rccl_halo(c, A, A->send_buf, A->ext, nc);
}

// From the fork on, the second stream may be writing Y: whichever way the product is left, the first stream waits for it, so that the
// stream the caller synchronises covers every write (an error return must not leave the interior product in flight on panels the
// caller is then free to release).  The normal exit has recorded and waited itself and calls joined().
struct JoinGuard {
    rails_ctx *c;
    bool armed = true;
    explicit JoinGuard(rails_ctx *ctx) : c(ctx) {}
    void joined() { armed = false; }
    ~JoinGuard()
    {
        if (!armed) return;
        (void)hipEventRecord(c->ev_join, c->stream2); // (already on the way out with an error, or with one to come from the next call)
        (void)hipStreamWaitEvent(c->stream, c->ev_join, 0);
    }
};

// The row-partitioned product in the overlapped order: the interior rows' product runs on the context's second stream while the ghost rows
// are packed, exchanged and waited for on the first; the boundary rows follow the exchange, and the first stream then waits for the
// interior.  Row by row the same kernels as the serial order (`RAILS_SPMM_HALO_OVERLAP=0`): the result is bitwise the same.
int overlapped_product(rails_ctx *c, rails_csr *A, const OpOrder &interior, const Product &p, bool x_vec2, bool y_vec2)
{
    const rails_panel *X = p.X, *Y = p.Y;
    const int nc = p.nc;
    RAILS_TRY(rails_ctx_second_stream(c));
    RAILS_HIP_CHECK(hipEventRecord(c->ev_fork, c->stream));
    JoinGuard join(c);
    RAILS_HIP_CHECK(hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
    bool planes_done = false, sweep_done = false;
    for (int i = 0; i < interior.n && !planes_done && !sweep_done; ++i) {
        if (interior.step[i].kernel == OpStep::PLANES)
            RAILS_TRY(rails_spmm_planes_interior(c, A, p.Xp, X->ld, p.Yp, Y->ld, nc, x_vec2, c->stream2, &planes_done));
        else if (interior.step[i].kernel == OpStep::SWEEP)
            RAILS_TRY(rails_spmm_sweep_interior(c, A, p.Xp, X->ld, p.Yp, Y->ld, nc, x_vec2 && y_vec2, c->stream2, &sweep_done));
    }
    if (!planes_done && !sweep_done) {
        const RowSpan in = {A->int_lo, A->int_hi - A->int_lo, c->stream2};
        RAILS_TRY(spmm_span(c, A, rails_row_choice(row_facts(A, nc, x_vec2, y_vec2, false, p.Xp, X->ld, p.Xp, X->ld, 0)), p.Xp, X->ld, p.Xp, X->ld, p.Yp, Y->ld, nc, in));
    }
    RAILS_HIP_CHECK(hipEventRecord(c->ev_join, c->stream2));
    c->n_spmm_overlapped++;
    RAILS_TRY(exchange_halo(c, A, p.Xp, X->ld, nc));
    const RowSpan lo = {0, A->int_lo, nullptr}, hi = {A->int_hi, A->m - A->int_hi, nullptr};
    // (ghost rows are packed with ld = nc: even, 16-byte aligned rows when nc is even)
    const RowChoice ch = rails_row_choice(row_facts(A, nc, x_vec2, y_vec2, false, p.Xp, X->ld, A->ext, nc, 1));
    RAILS_TRY(spmm_span(c, A, ch, p.Xp, X->ld, A->ext, nc, p.Yp, Y->ld, nc, lo));
    RAILS_TRY(spmm_span(c, A, ch, p.Xp, X->ld, A->ext, nc, p.Yp, Y->ld, nc, hi));
    RAILS_HIP_CHECK(hipStreamWaitEvent(c->stream, c->ev_join, 0));
    join.joined();
    // what ran: the kernel of the boundary rows (the chunked one counts as row-gather beside another kernel's name), and of the
    // interior rows where that is another one
    static const char *const overlapped[3][3] = {
        {"k_spmm_rowgather (halo overlapped)", "k_spmm_rowgather_cc (halo overlapped)", "k_spmm_narrow (halo overlapped)"},
        {"k_spmm_rowgather + k_spmm_planes (halo overlapped)", "k_spmm_rowgather + k_spmm_planes (halo overlapped)", "k_spmm_narrow + k_spmm_planes (halo overlapped)"},
        {"k_spmm_rowgather + k_spmm_sweep (halo overlapped)", "k_spmm_rowgather + k_spmm_sweep (halo overlapped)", "k_spmm_rowgather + k_spmm_sweep (halo overlapped)"}};
    const RowChoice::Kind boundary = (lo.nrows > 0 || hi.nrows > 0) ? ch.kind : RowChoice::PLAIN;
    A->last_kernel = overlapped[sweep_done ? 2 : planes_last_interior(A) ? 1 : 0][boundary];
    c->n_spmm_rowgather++;
    RAILS_HIP_CHECK(hipGetLastError());
    return RAILS_OK;
}

// All rows on the context's stream: the whole-operator kernels in the order of rails_op_order, then the row kernel of rails_row_choice.
int local_product(rails_ctx *c, rails_csr *A, const OpOrder &order, const Product &p)
{
    const rails_panel *X = p.X, *Y = p.Y;
    const int xc0 = p.xc0, yc0 = p.yc0, nc = p.nc, ldg = p.ldg;
    const bool vec2 = ((xc0 | yc0) & 1) == 0 && (ldg % 2 == 0);
    for (int i = 0; i < order.n; ++i) {
        const bool forced = order.step[i].forced;
        bool done = false;
        switch (order.step[i].kernel) {
        case OpStep::SWEEP: { // banded patterns at panel width (spmm_sweep.hip; forced, it fails itself instead of declining)
            const bool al = vec2 && X->ld % 2 == 0 && Y->ld % 2 == 0;
            RAILS_TRY(rails_spmm_sweep(c, A, p.Xp, X->ld, p.Xg, ldg, p.Yp, Y->ld, nc, al, forced, &done));
            break;
        }
        case OpStep::PLANES: { // structured-grid stencils (complete 7- / 27-point patterns) at every even width (spmm_planes.hip) -- the plan
                               // is one pass over the matrix on the device (a product's worth of time), made by the first product that asks
            const bool al = (xc0 & 1) == 0 && X->ld % 2 == 0; // (16-byte aligned X rows for the LDS-DMA; Y's window may sit on an odd column)
            RAILS_TRY(rails_spmm_planes(c, A, p.Xp, X->ld, p.Yp, Y->ld, nc, al, true, &done));
            if (done) c->n_spmm_planes++;
            RAILS_REQUIRE(done || !forced, "rails_spmm: plane-sweep kernel requested but not applicable to this operator/shape");
            break;
        }
        case OpStep::TILED:
            RAILS_TRY(rails_spmm_tiled(c, A, p.Xp, X->ld, p.Xg, ldg, p.Yp, Y->ld, nc, vec2, X->ld - xc0, &done));
            if (done) c->n_spmm_tiled++;
            RAILS_REQUIRE(done || !forced, "rails_spmm: LDS-staged kernel requested but not applicable to this operator/shape");
            break;
        }
        if (done) {
            RAILS_HIP_CHECK(hipGetLastError());
            return RAILS_OK;
        }
    }
    // (the gathers need 16-byte aligned X rows; a Y window on an odd column -- A*W written behind an odd number of basis columns --
    // only changes the form of the stores)
    const bool x_vec2 = (xc0 & 1) == 0 && (X->ld % 2 == 0) && (ldg % 2 == 0);
    const bool y_vec2 = (yc0 & 1) == 0 && (Y->ld % 2 == 0);
    const RowChoice ch = rails_row_choice(row_facts(A, nc, x_vec2, y_vec2, vec2, p.Xp, X->ld, p.Xg, ldg, -1));
    RAILS_TRY(launch_rows(c, A, ch, p.Xp, X->ld, p.Xg, ldg, p.Yp, Y->ld, nc));
    A->last_kernel = ROW_KERNEL[ch.kind];
    c->n_spmm_rowgather++;
    RAILS_HIP_CHECK(hipGetLastError());
    return RAILS_OK;
}

} // namespace

// The exchange of rails_spmm on its own (itsolve.hip's fused polynomial step gathers from the ghost buffer itself): grows the two buffers
// as rails_spmm does, packs nc columns from Xp and exchanges; afterwards (in stream order) A->ext holds the ghost rows with row stride nc.
// The caller decides whether to exchange by rails_spmm's condition (n_ghost > 0 || n_send > 0); a rank that only sends or only receives
// takes part with an empty buffer on the other side.
int rails_halo_exchange(rails_ctx *c, rails_csr *A, const double *Xp, int ldx, int nc)
{
    RAILS_TRY(grow_buffer(c, &A->send_buf, &A->send_cap, (size_t)(A->n_send ? A->n_send : 1) * nc * sizeof(double)));
    RAILS_TRY(grow_buffer(c, &A->ext, &A->ext_cap, (size_t)(A->n_ghost ? A->n_ghost : 1) * nc * sizeof(double)));
    return exchange_halo(c, A, Xp, ldx, nc);
}

extern "C" int rails_spmm(rails_ctx *c, rails_csr *A, int trans, const rails_panel *X, int xc0, int nc, rails_panel *Y, int yc0)
{
    if (c) hipSetDevice(c->device); // allocations and launches go to the context's device whatever the caller's current device is
    rails_slow_guard slow__(c, "rails_spmm", nc, A ? A->m : 0);
    RAILS_REQUIRE(c && A && X && Y, "rails_spmm: null argument");
    if (A->kind == rails_csr::SPRHS) return apply_delegate(c, A, trans, X, xc0, nc, Y, yc0); // m x p: it checks the shapes of either direction itself
    RAILS_TRY(check_windows(A, trans, X, xc0, nc, Y, yc0));
    if (nc == 0 || A->m == 0) return RAILS_OK;
    if (A->kind != rails_csr::STORED) return apply_delegate(c, A, trans, X, xc0, nc, Y, yc0);
    if (trans) {
        RAILS_TRY(build_transpose(A));
        A->AT->variant = A->variant;
        int rc = rails_spmm(c, A->AT, 0, X, xc0, nc, Y, yc0);
        A->last_kernel = A->AT->last_kernel;
        return rc;
    }
    // columns beyond the operator's rows come from the ghost buffer; for a rectangular operator (more columns than rows, all of them
    // local) that buffer is the rest of X itself
    Product p = {X, Y, xc0, yc0, nc, X->d + xc0, Y->d + yc0, nullptr, X->ld};
    p.Xg = A->rect ? p.Xp + (size_t)std::min(A->m, A->ncols_ext) * X->ld : p.Xp;
    const bool x_vec2 = (xc0 & 1) == 0 && (X->ld % 2 == 0) && (nc % 2 == 0), y_vec2 = (yc0 & 1) == 0 && (Y->ld % 2 == 0);
    const OpFacts facts = rails_op_facts(c, A, nc, x_vec2, y_vec2);
    if (A->n_ghost > 0 || A->n_send > 0) {
        // pack the rows the neighbours need, exchange, gather from [local | ghost]
        RAILS_TRY(grow_buffer(c, &A->send_buf, &A->send_cap, (size_t)(A->n_send ? A->n_send : 1) * nc * sizeof(double)));
        RAILS_TRY(grow_buffer(c, &A->ext, &A->ext_cap, (size_t)(A->n_ghost ? A->n_ghost : 1) * nc * sizeof(double)));
        const HaloOrder halo = rails_halo_order(facts);
        if (halo.overlap) return overlapped_product(c, A, halo.interior, p, x_vec2, y_vec2);
        RAILS_TRY(exchange_halo(c, A, p.Xp, X->ld, nc));
        p.Xg = A->ext;
        p.ldg = nc;
    }
    return local_product(c, A, rails_op_order(facts, [&] { return rails_csr_is_grid(A); }), p);
}
