// dense.hip -- tall-skinny dense kernels on v_mfma_f64_16x16x4_f64 (gfx950):
//   rails_gram        C = X^T Y          (MultiVector::dot,  src/StlWrapper.cpp:394-412)
//   rails_panel_gemm  Y = beta Y + alpha X C   (MultiVector * DenseMatrix, src/StlWrapper.cpp:168-187)
//
// fp64 MFMA on gfx950 runs at the fp64 vector rate; it is used here because it needs ONE operand
// register per lane per 2048 flop (no LDS broadcast of the small operand, no register tiling),
// which leaves the load path free: both kernels are HBM-bound whenever one small dimension is
// <= 32 (every call of the solver) and reach the fp64 ridge only for k x 128 restart products.
//
// MFMA f64 16x16x4 lane maps (cdna_hip_programming.md section 3): lane l supplies A[i=l&15][k=l>>4]
// and B[k=l>>4][j=l&15]; it receives D[row=(l>>4)+4*v][col=l&15] in result register v (0..3).
//
// Reductions over rows are two-stage and deterministic: per-block partial tiles are written to a
// workspace and summed in a fixed order by a second kernel (no float atomics), then all-reduced
// over the ranks through the context hook.
//
// The row-split Gram, the wide-X Gram and the panel GEMM each have ONE body (dense_gram.inc, dense_gram_cols.inc, dense_panel_gemm.inc),
// written against the left operand Xo: a OneSeg, columns of one panel, or a TwoSeg, [X1 | X2] in two panels (the deflated projection of
// orth.hip: the nullspace and the old basis columns).  Every __global__ kernel declares its own parameters and attributes, builds Xo and
// includes the body, so a one-segment kernel has the arguments, the attributes and -- compared per kernel on the assembly when the bodies
// were merged -- the instructions and registers it had with a body of its own.  (The bodies are text, not __forceinline__ functions:
// a function is optimised once on its own and again after inlining, which alone reordered operands in k_gram.)
#include "rails_internal.h"

#include <dlfcn.h>
#include <atomic>
#include <mutex>

#include <algorithm>

namespace {

typedef double v4f64 __attribute__((ext_vector_type(4)));
typedef double v2f64 __attribute__((ext_vector_type(2)));

// Tile counts fitted to the widths a solve runs at: k_update_gram<5, .>, k_gram_cols<5, 1, .>, the odd TR of
// k_panel_gemm_wide and its skipped half chunk.  One process-wide switch for all of them: rails_dense_set_tile_fit, or
// RAILS_DENSE_TILE_FIT=0 in the environment (read at the first use, unless the setter came first).  Off: the choices before the fit.
// Either way the same bits come out: the fitted forms leave out work on zero padding and nothing else.
std::atomic<int> g_tile_fit{-1}; // -1: not decided yet

bool dense_tile_fit()
{
    int v = g_tile_fit.load(std::memory_order_relaxed);
    if (v < 0) {
        const char *e = getenv("RAILS_DENSE_TILE_FIT");
        int undecided = -1;
        g_tile_fit.compare_exchange_strong(undecided, (e ? atoi(e) : 1) ? 1 : 0); // (a setter that got in between wins)
        v = g_tile_fit.load(std::memory_order_relaxed);
    }
    return v != 0;
}

// The schedule of the fused update + second projection: k_update_gram_p, or k_update_gram as it was.  Process-wide
// like the tile fit: rails_dense_set_update_gram_pipeline, or RAILS_UPDATE_GRAM_PIPELINE=0 in the environment (read at the first use,
// unless the setter came first).  The same bits either way.
std::atomic<int> g_update_gram_pipeline{-1}; // -1: not decided yet

bool dense_update_gram_pipeline()
{
    int v = g_update_gram_pipeline.load(std::memory_order_relaxed);
    if (v < 0) {
        const char *e = getenv("RAILS_UPDATE_GRAM_PIPELINE");
        int undecided = -1;
        g_update_gram_pipeline.compare_exchange_strong(undecided, (e ? atoi(e) : 1) ? 1 : 0); // (a setter that got in between wins)
        v = g_update_gram_pipeline.load(std::memory_order_relaxed);
    }
    return v != 0;
}

__device__ __forceinline__ v4f64 mfma_f64(double a, double b, v4f64 c)
{
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// The left operand X of a kernel body: col() turns a column index into the handle a lane keeps per tile, row() a row index into the base
// pointer(s) of that row, at() both into an address.
struct OneSeg {
    const double *X;
    int ld;
    struct Row {
        const double *x;
    };
    __device__ int col(int c) const { return c; }
    __device__ Row row(int64_t r) const { return {X + r * ld}; }
    __device__ static const double *at(Row r, int c) { return r.x + c; }
};
// [X1 | X2]: columns [0, a1) are columns of X1, [a1, a) columns of X2; a lane picks the segment by address
struct TwoSeg {
    const double *X1;
    int ld1, a1;
    const double *X2;
    int ld2;
    struct Col {
        int off;
        bool second;
    };
    struct Row {
        const double *x1, *x2;
    };
    __device__ Col col(int c) const
    {
        const bool second = c >= a1;
        return {second ? c - a1 : c, second};
    }
    __device__ Row row(int64_t r) const { return {X1 + r * ld1, X2 + r * ld2}; }
    __device__ static const double *at(Row r, Col c) { return (c.second ? r.x2 : r.x1) + c.off; }
};

// ------------------------------------------------------------------------------- Gram ---
// grid.x = row slabs, grid.y = tile groups (gi over X column tiles, gj over Y column tiles).
// Each of the 4 waves accumulates TI x TJ output tiles over its share of the slab's rows.
template <int TI, int TJ>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 8))) void k_gram(const double *__restrict__ X, int ldx, int a, const double *__restrict__ Y, int ldy,
                                              int b, int64_t m, int64_t rows_per_slab, int ngj, double *__restrict__ partial)
{
    const OneSeg Xo{X, ldx};
#include "dense_gram.inc"
}

// the same with X = [X1 | X2], a columns in all (no amdgpu_waves_per_eu: these kernels never had one)
template <int TI, int TJ>
__global__ __launch_bounds__(256) void k_gram2(const double *__restrict__ X1, int ldx1, int a1, const double *__restrict__ X2, int ldx2, int a,
                                               const double *__restrict__ Y, int ldy, int b, int64_t m, int64_t rows_per_slab, int ngj,
                                               double *__restrict__ partial)
{
    const TwoSeg Xo{X1, ldx1, a1, X2, ldx2};
#include "dense_gram.inc"
}

// Wide-X / narrow-Y form (the projections [P | X]' X of the coordinate-space back end: a = dim + w >> b = w <= 32): the four waves
// of a block take four ADJACENT 64-column strips of X for the SAME rows, so a block reads whole 2 KiB row segments (the row-split
// form above reads 512 B per row and block; measured 3.0 -> see profiles/r01_kernels.md) and Y's few columns once; every wave owns
// its output tiles, so there is no cross-wave reduction.  Two 4-row steps are in flight per wave.
// NE columns of Y beyond 16 * TJ (the prefetched random vector that rides at the end of an A*W block: b = 17) are done with plain
// multiply-adds on the values the lanes hold anyway: a second MFMA column tile for ONE column doubles the matrix work, and the pass
// took a third longer for it (0.81 against 0.61 ms at 369 x 17 / 369 x 16, 1M rows).  A lane sums its own rows (r + kk, r + 4 + kk, ...) of
// its own column; the four row classes are added at the end (kk = 0 + 1, + 2, + 3: a fixed order).
template <int TI, int TJ, int NE = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 8))) void k_gram_cols(const double *__restrict__ X, int ldx, int a,
                                                                                             const double *__restrict__ Y, int ldy, int b, int64_t m,
                                                                                             int64_t rows_per_slab, double *__restrict__ partial)
{
    const OneSeg Xo{X, ldx};
#include "dense_gram_cols.inc"
}

// the same with X = [X1 | X2], a columns in all (no amdgpu_waves_per_eu: these kernels never had one)
template <int TI, int TJ, int NE>
__global__ __launch_bounds__(256) void k_gram_cols2(const double *__restrict__ X1, int ldx1, int a1, const double *__restrict__ X2, int ldx2, int a,
                                                    const double *__restrict__ Y, int ldy, int b, int64_t m, int64_t rows_per_slab,
                                                    double *__restrict__ partial)
{
    const TwoSeg Xo{X1, ldx1, a1, X2, ldx2};
#include "dense_gram_cols.inc"
}

// out[e] = sum_t partial[t][e] in a fixed order: 16 interleaved strands per element, then the strands 0..15
__global__ __launch_bounds__(1024) void k_reduce_partials(const double *__restrict__ partial, int64_t nslab, int64_t n, double *__restrict__ out)
{
    __shared__ double sh[16][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int64_t e = (int64_t)blockIdx.x * 64 + tx;
    double s = 0.0;
    if (e < n)
        for (int64_t t = ty; t < nslab; t += 16) s += partial[t * n + e];
    sh[ty][tx] = s;
    __syncthreads();
    if (ty == 0 && e < n) {
        double r = 0.0;
#pragma unroll
        for (int g = 0; g < 16; ++g) r += sh[g][tx];
        out[e] = r;
    }
}

template <int TI, int TJ>
void launch_gram(rails_ctx *c, const double *X, int ldx, int a, const double *Y, int ldy, int b, int64_t m, int64_t rps,
                 int64_t nslab, double *partial)
{
    int ngi = (a + 16 * TI - 1) / (16 * TI), ngj = (b + 16 * TJ - 1) / (16 * TJ);
    RAILS_LAUNCH((k_gram<TI, TJ>), dim3((unsigned)nslab, (unsigned)(ngi * ngj)), dim3(256), 0, c->stream, X, ldx, a, Y, ldy, b,
                       m, rps, ngj, partial);
}

template <int TI, int TJ>
void launch_gram2(rails_ctx *c, const double *X1, int ldx1, int a1, const double *X2, int ldx2, int a, const double *Y, int ldy, int b, int64_t m,
                  int64_t rps, int64_t nslab, double *partial)
{
    int ngi = (a + 16 * TI - 1) / (16 * TI), ngj = (b + 16 * TJ - 1) / (16 * TJ);
    RAILS_LAUNCH((k_gram2<TI, TJ>), dim3((unsigned)nslab, (unsigned)(ngi * ngj)), dim3(256), 0, c->stream, X1, ldx1, a1, X2, ldx2, a, Y, ldy, b,
                 m, rps, ngj, partial);
}

// ------------------------------------------------------------------------- panel GEMM ---
// Each wave owns 16 rows and all r (<= 16*TR) output columns; the block streams C through LDS in
// chunks of KC rows.  X is read with the k index permuted inside every 16-column block so that a
// lane reads 4 consecutive doubles: lane (i,kk) holds X[row i][kb + 4*kk + s], s = 0..3, and MFMA
// number s sums over k in {kb + 4*kk + s}; C's rows are fetched from LDS with the same permutation.
template <int TR, int KC>
__global__ __launch_bounds__(256) void k_panel_gemm(double alpha, const double *X, int ldx, int k,
                                                    const double *__restrict__ C, int r, double beta, double *Yp,
                                                    int ldy, int64_t m, int vec_ok)
{
    const OneSeg Xo{X, ldx};
#define RAILS_PG_VEC4(c) (vec_ok && (c) + 4 <= k)
#include "dense_panel_gemm.inc"
}

// the same with X = [X1 | X2], a columns in all; vec1 / vec2: the rows of that segment may be read 16 bytes at a time
template <int TR, int KC>
__global__ __launch_bounds__(256) void k_panel_gemm2(double alpha, const double *X1, int ldx1, int a1, const double *X2, int ldx2, int a,
                                                     const double *__restrict__ C, int r, double beta, double *Yp, int ldy, int64_t m, int vec1,
                                                     int vec2)
{
    const TwoSeg Xo{X1, ldx1, a1, X2, ldx2};
    const int k = a;
#define RAILS_PG_VEC4(c) (((c) + 4 <= a1 && vec1) || ((c) >= a1 && (c) + 4 <= a && vec2))
#include "dense_panel_gemm.inc"
}

template <int TR, int KC>
void launch_pg(rails_ctx *c, double alpha, const double *X, int ldx, int k, const double *C, int r, double beta, double *Y,
               int ldy, int64_t m, int vec_ok)
{
    int64_t grid = (m + 63) / 64;
    RAILS_LAUNCH((k_panel_gemm<TR, KC>), dim3((unsigned)grid), dim3(256), 0, c->stream, alpha, X, ldx, k, C, r, beta, Y,
                       ldy, m, vec_ok);
}

// The restart rotation P2 = P Q (k and r in the hundreds: the one compute-bound product of the solver, src/StlWrapper.cpp:168-187 behind
// src/LyapunovSolver.hpp:265,290) in ONE pass: a wave keeps 16 rows x ALL r <= 288 output columns in registers (TR tiles of 16 x 16, 8
// VGPRs each), so X is read once (k_panel_gemm in 128-column slices read it once per slice and padded r = 268 to 384 columns of MFMA
// work) and the matrix pipe does exactly ceil(r / 16) tiles per step.  C comes packed (k_pack_ct: transposed, rows of 16 TR + 4 doubles
// -- the two k-groups a ds_read_b64 serves together fall on disjoint bank halves -- zero padded to whole chunks of 32 rows) and streams
// through a double buffer in LDS by LDS-DMA: chunk i + 1 lands while chunk i is multiplied, one barrier per chunk, no staging loop in
// the waves (a first form staged C with plain loads and LDS stores, 36 round trips per thread and chunk: 28 TFLOP/s).  8 waves x 16
// rows per workgroup, one workgroup per CU (2 x 73 KiB of LDS).  X and Y must not alias.
__global__ void k_pack_ct(const double *__restrict__ C, int k, int r, int kpad, int RL, double *__restrict__ out)
{
    const int64_t n = (int64_t)kpad * RL;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
        const int kl = (int)(q / RL), j = (int)(q % RL);
        out[q] = (kl < k && j < r) ? C[kl + (int64_t)j * k] : 0.0;
    }
}

template <int TR>
__global__ __launch_bounds__(512) void k_panel_gemm_wide(double alpha, const double *__restrict__ X, int ldx, int k, const double *__restrict__ Ct /* packed, kpad x RL */,
                                                         int r, double beta, double *__restrict__ Yp, int ldy, int64_t m, int vec_ok, int skip_tail)
{
    constexpr int KC = 32, RL = 16 * TR + 4, CHUNK_B = KC * RL * 8, PIECES = CHUNK_B / 1024; // (KC * RL * 8 is a multiple of 1024 for every TR)
    static_assert(CHUNK_B % 1024 == 0, "whole LDS-DMA pieces per chunk");
    extern __shared__ double Cs[]; // 2 x KC x RL
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int li = lane & 15, kk = lane >> 4;
    const int64_t r0 = ((int64_t)blockIdx.x * 8 + wave) * 16;
    const int64_t myrow = r0 + li;
    const bool rowok = myrow < m;
    const int nchunks = (k + KC - 1) / KC;
    const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)Cs;
    const uint32_t lane16 = (uint32_t)lane * 16u;
    auto stage = [&](int chunk) { // this wave's pieces of a chunk: piece p goes to wave p % 8
        const char *src = reinterpret_cast<const char *>(Ct) + (size_t)chunk * CHUNK_B;
        const uint32_t dst = lds_base + (uint32_t)((chunk & 1) * CHUNK_B);
        for (int p = wave; p < PIECES; p += 8) {
            uint32_t keep;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(lane16), "s"(src + (size_t)p * 1024), "s"(dst + (uint32_t)(p * 1024)) : "memory");
        }
    };
    v4f64 acc[TR];
#pragma unroll
    for (int t = 0; t < TR; ++t) acc[t] = (v4f64){0.0, 0.0, 0.0, 0.0};
    const double *xrow = X + (rowok ? myrow : m - 1) * ldx;
    auto fetch = [&](int kcol, double *xs) {
        if (vec_ok && kcol + 4 <= k) {
            v2f64 t0 = *reinterpret_cast<const v2f64 *>(xrow + kcol);
            v2f64 t1 = *reinterpret_cast<const v2f64 *>(xrow + kcol + 2);
            xs[0] = t0.x;
            xs[1] = t0.y;
            xs[2] = t1.x;
            xs[3] = t1.y;
        } else {
#pragma unroll
            for (int s = 0; s < 4; ++s) xs[s] = (kcol + s < k) ? xrow[kcol + s] : 0.0;
        }
    };
    double xa[4], xb[4];
    stage(0);
    fetch(4 * kk, xa);
    fetch(16 + 4 * kk, xb);
    asm volatile("s_waitcnt vmcnt(0)" : : : "memory");
    __builtin_amdgcn_s_barrier();
    for (int ci = 0; ci < nchunks; ++ci) {
        if (ci + 1 < nchunks) stage(ci + 1); // into the buffer every wave left at the barrier above
        double xc[4], xd[4];
        fetch((ci + 1) * KC + 4 * kk, xc);
        fetch((ci + 1) * KC + 16 + 4 * kk, xd);
        const double *cb = Cs + (size_t)(ci & 1) * (KC * RL);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const double *crow = &cb[(4 * kk + s) * RL + li];
#pragma unroll
            for (int t = 0; t < TR; ++t) acc[t] = mfma_f64(xa[s], crow[16 * t], acc[t]);
        }
        // (skip_tail: the second half of the last chunk is left out where it lies past k altogether -- sixteen k-steps of zeros times
        // zeros.  The same for every wave of every block; the fetches above stay, so the loads keep their order.)
        if (!skip_tail || ci * KC + 16 < k) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const double *crow = &cb[(16 + 4 * kk + s) * RL + li];
#pragma unroll
                for (int t = 0; t < TR; ++t) acc[t] = mfma_f64(xb[s], crow[16 * t], acc[t]);
            }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            xa[s] = xc[s];
            xb[s] = xd[s];
        }
        // the next chunk has landed (this wave's pieces; then everybody's) and nobody reads this chunk's buffer any more
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" : : : "memory");
        __builtin_amdgcn_s_barrier();
    }
#pragma unroll
    for (int t = 0; t < TR; ++t) {
        const int j = 16 * t + li;
        if (j >= r) continue;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int64_t row = r0 + kk + 4 * v;
            if (row >= m) continue;
            double *dst = Yp + row * ldy + j;
            double val = alpha * acc[t][v];
            if (beta != 0.0) val += beta * (*dst);
            *dst = val;
        }
    }
}

// C (k x r, column-major, on the device) -> packed in `ct`; then the product
template <int TR>
int launch_pg_wide(rails_ctx *c, double alpha, const double *X, int ldx, int k, const double *C, int r, double beta, double *Y, int ldy, int64_t m, int vec_ok, double *ct)
{
    constexpr int RL = 16 * TR + 4;
    const int kpad = (k + 31) / 32 * 32;
    RAILS_LAUNCH(k_pack_ct, dim3((unsigned)std::min<int64_t>(512, ((int64_t)kpad * RL + 255) / 256)), dim3(256), 0, c->stream, C, k, r, kpad, RL, ct);
    const size_t lds = (size_t)2 * 32 * RL * sizeof(double);
    RAILS_HIP_CHECK(hipFuncSetAttribute((const void *)k_panel_gemm_wide<TR>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    RAILS_LAUNCH((k_panel_gemm_wide<TR>), dim3((unsigned)((m + 127) / 128)), dim3(512), lds, c->stream, alpha, X, ldx, k, ct, r, beta, Y, ldy, m, vec_ok,
                 dense_tile_fit() ? 1 : 0);
    c->last_gemm_wide_tr = TR;
    return RAILS_OK;
}

// row slabs of a Gram product (a x b): enough blocks to fill the chip, partial-tile traffic bounded to ~4% of the input
void gram_slabs(int64_t m, int a, int b, int64_t *nslab_out, int64_t *rps_out)
{
    double bound = 0.02 * (double)m * (double)(a + b) / ((double)a * (double)b);
    int64_t nslab = (int64_t)std::min<double>(1024.0, std::max<double>(1.0, bound));
    int64_t maxslab = (m + 15) / 16;
    if (nslab > maxslab) nslab = std::max<int64_t>(1, maxslab);
    int64_t rps = (m + nslab - 1) / nslab;
    rps = (rps + 15) / 16 * 16;
    if (rps < 16) rps = 16;
    *nslab_out = std::max<int64_t>(1, (m + rps - 1) / rps);
    *rps_out = rps;
}

// wide-X form: tiles of 16 X-columns per wave, the choice that leaves the fewest idle tile slots in blocks of four waves
// (one_tile: Y is one MFMA column tile, b <= 16 or the 17th column on the vector unit).  With the tile fit a one-tile form of six
// tiles per wave becomes one of five where five cover the columns with the same number of waves (19 and 20 tiles, 289 to 320
// columns: 20 slots instead of 24).  Not where five need a wave more: at 17 and 18 tiles six tiles keep three waves busy, the fourth
// leaves at once and costs nothing, and four waves of five measured 16 us slower (profiles/r11_tile_fit_kernels.md).
int gram_cols_tiles(int ntiles, bool one_tile)
{
    const int cand2[3] = {3, 4, 5}, cand1[3] = {4, 6, 8};
    const int *cand = one_tile ? cand1 : cand2;
    int best = cand[1], best_cost = 1 << 30;
    for (int q = 0; q < 3; ++q) {
        int ti = cand[q], strips = (ntiles + ti - 1) / ti, cost = (strips + 3) / 4 * 4 * ti;
        if (cost < best_cost) best = ti, best_cost = cost;
    }
    if (one_tile && best == 6 && (ntiles + 4) / 5 == (ntiles + 5) / 6 && dense_tile_fit()) best = 5;
    return best;
}

// the eleven instantiations of the wide-X form; K is k_gram_cols or k_gram_cols2, the variadic part its operand arguments
#define RAILS_GRAM_COLS_CASE(K, TI, TJ, NE, ...) RAILS_LAUNCH((K<TI, TJ, NE>), grid, dim3(256), 0, c->stream, __VA_ARGS__, Y, ldy, b, m, rps, c->ws)
#define RAILS_GRAM_COLS(K, ...)                                                                                                            \
    do {                                                                                                                                   \
        const int ntiles = (a + 15) / 16, best = gram_cols_tiles(ntiles, b <= 16 || extra);                                                \
        const dim3 grid((unsigned)nslab, (unsigned)(((ntiles + best - 1) / best + 3) / 4));                                                \
        c->last_gram_cols_ti = best;                                                                                                       \
        if (extra) {                                                                                                                       \
            if (best == 4)                                                                                                                 \
                RAILS_GRAM_COLS_CASE(K, 4, 1, 1, __VA_ARGS__);                                                                             \
            else if (best == 5)                                                                                                            \
                RAILS_GRAM_COLS_CASE(K, 5, 1, 1, __VA_ARGS__);                                                                             \
            else if (best == 6)                                                                                                            \
                RAILS_GRAM_COLS_CASE(K, 6, 1, 1, __VA_ARGS__);                                                                             \
            else                                                                                                                           \
                RAILS_GRAM_COLS_CASE(K, 8, 1, 1, __VA_ARGS__);                                                                             \
        } else if (b <= 16) {                                                                                                              \
            if (best == 4)                                                                                                                 \
                RAILS_GRAM_COLS_CASE(K, 4, 1, 0, __VA_ARGS__);                                                                             \
            else if (best == 5)                                                                                                            \
                RAILS_GRAM_COLS_CASE(K, 5, 1, 0, __VA_ARGS__);                                                                             \
            else if (best == 6)                                                                                                            \
                RAILS_GRAM_COLS_CASE(K, 6, 1, 0, __VA_ARGS__);                                                                             \
            else                                                                                                                           \
                RAILS_GRAM_COLS_CASE(K, 8, 1, 0, __VA_ARGS__);                                                                             \
        } else if (best == 3)                                                                                                              \
            RAILS_GRAM_COLS_CASE(K, 3, 2, 0, __VA_ARGS__);                                                                                 \
        else if (best == 4)                                                                                                                \
            RAILS_GRAM_COLS_CASE(K, 4, 2, 0, __VA_ARGS__);                                                                                 \
        else                                                                                                                               \
            RAILS_GRAM_COLS_CASE(K, 5, 2, 0, __VA_ARGS__);                                                                                 \
    } while (0)

} // namespace

extern "C" void rails_dense_set_tile_fit(int on) { g_tile_fit.store(on ? 1 : 0); }

extern "C" int rails_dense_tile_fit(void) { return dense_tile_fit() ? 1 : 0; }

extern "C" int rails_dense_last_tiles(const rails_ctx *c, int *update_gram_nbw, int *gram_cols_ti, int *gemm_wide_tr)
{
    RAILS_REQUIRE(c, "rails_dense_last_tiles: null context");
    if (update_gram_nbw) *update_gram_nbw = c->last_update_gram_nbw;
    if (gram_cols_ti) *gram_cols_ti = c->last_gram_cols_ti;
    if (gemm_wide_tr) *gemm_wide_tr = c->last_gemm_wide_tr;
    return RAILS_OK;
}

extern "C" void rails_dense_set_update_gram_pipeline(int on) { g_update_gram_pipeline.store(on ? 1 : 0); }

extern "C" int rails_dense_update_gram_pipeline(void) { return dense_update_gram_pipeline() ? 1 : 0; }

extern "C" int rails_dense_last_update_gram_form(const rails_ctx *c, int *form)
{
    RAILS_REQUIRE(c && form, "rails_dense_last_update_gram_form: null argument");
    *form = c->last_update_gram_form;
    return RAILS_OK;
}

int rails_gram_dev(rails_ctx *c, const double *X, int ldx, const double *Y, int ldy, int64_t m, int a, int b, double *C_dev)
{
    if (a <= 0 || b <= 0) return RAILS_OK;
    int64_t nslab, rps;
    gram_slabs(m, a, b, &nslab, &rps);
    size_t n = (size_t)a * b;
    RAILS_TRY(rails_ws_reserve(c, (size_t)nslab * n * sizeof(double)));
    if (b <= 16 && a <= 16)
        launch_gram<1, 1>(c, X, ldx, a, Y, ldy, b, m, rps, nslab, c->ws);
    else if (b <= 32 && a >= 128) {
        static const int cols_form = getenv("RAILS_GRAM_COLS") ? atoi(getenv("RAILS_GRAM_COLS")) : 1;
        if (cols_form) {
            // b = 17: one MFMA column tile and the 17th column on the vector unit (see gram_cols_body)
            static const int extra_env = getenv("RAILS_GRAM_EXTRA_COLUMN") ? atoi(getenv("RAILS_GRAM_EXTRA_COLUMN")) : 1;
            const bool extra = extra_env && b == 17;
            RAILS_GRAM_COLS(k_gram_cols, X, ldx, a);
        } else if (b <= 16)
            launch_gram<8, 1>(c, X, ldx, a, Y, ldy, b, m, rps, nslab, c->ws);
        else
            launch_gram<4, 2>(c, X, ldx, a, Y, ldy, b, m, rps, nslab, c->ws);
    } else if (b <= 16)
        launch_gram<8, 1>(c, X, ldx, a, Y, ldy, b, m, rps, nslab, c->ws);
    else if (a <= 16)
        launch_gram<1, 8>(c, X, ldx, a, Y, ldy, b, m, rps, nslab, c->ws);
    else if (a <= 32 && b <= 32) // the block's own 17 x 17 Gram matrices of CholQR2
        launch_gram<2, 2>(c, X, ldx, a, Y, ldy, b, m, rps, nslab, c->ws);
    else if (b <= 32)
        launch_gram<4, 2>(c, X, ldx, a, Y, ldy, b, m, rps, nslab, c->ws);
    else if (a <= 32)
        launch_gram<2, 4>(c, X, ldx, a, Y, ldy, b, m, rps, nslab, c->ws);
    else
        launch_gram<2, 4>(c, X, ldx, a, Y, ldy, b, m, rps, nslab, c->ws);
    RAILS_LAUNCH(k_reduce_partials, dim3((unsigned)((n + 63) / 64)), dim3(1024), 0, c->stream, c->ws, nslab, (int64_t)n, C_dev);
    RAILS_HIP_CHECK(hipGetLastError());
    return RAILS_OK;
}

// the same for a left operand in two panels, [X1 X2]' Y with a = a1 + a2 columns (the deflated projection of orth.hip); b <= 32
int rails_gram2_dev(rails_ctx *c, const double *X1, int ldx1, int a1, const double *X2, int ldx2, int a2, const double *Y, int ldy, int64_t m, int b,
                    double *C_dev)
{
    const int a = a1 + a2;
    if (a <= 0 || b <= 0) return RAILS_OK;
    int64_t nslab, rps;
    gram_slabs(m, a, b, &nslab, &rps);
    const size_t n = (size_t)a * b;
    RAILS_TRY(rails_ws_reserve(c, (size_t)nslab * n * sizeof(double)));
    if (a >= 128 && b <= 32) {
        const bool extra = b == 17;
        RAILS_GRAM_COLS(k_gram_cols2, X1, ldx1, a1, X2, ldx2, a);
    } else if (a <= 16 && b <= 16)
        launch_gram2<1, 1>(c, X1, ldx1, a1, X2, ldx2, a, Y, ldy, b, m, rps, nslab, c->ws);
    else if (b <= 16)
        launch_gram2<8, 1>(c, X1, ldx1, a1, X2, ldx2, a, Y, ldy, b, m, rps, nslab, c->ws);
    else
        launch_gram2<4, 2>(c, X1, ldx1, a1, X2, ldx2, a, Y, ldy, b, m, rps, nslab, c->ws);
    RAILS_LAUNCH(k_reduce_partials, dim3((unsigned)((n + 63) / 64)), dim3(1024), 0, c->stream, c->ws, nslab, (int64_t)n, C_dev);
    RAILS_HIP_CHECK(hipGetLastError());
    return RAILS_OK;
}

extern "C" int rails_gram(rails_ctx *c, const rails_panel *X, int xc0, int a, const rails_panel *Y, int yc0, int b, double *C_host,
                          int ldc)
{
    if (c) hipSetDevice(c->device); // allocations and launches go to the context's device whatever the caller's current device is
    rails_slow_guard slow__(c, "rails_gram", a, b);
    RAILS_REQUIRE(c && X && Y, "rails_gram: null argument");
    RAILS_REQUIRE(a >= 0 && b >= 0 && xc0 >= 0 && yc0 >= 0 && xc0 + a <= X->cap && yc0 + b <= Y->cap,
                  "rails_gram: windows [%d,%d) / [%d,%d) outside capacities %d / %d", xc0, xc0 + a, yc0, yc0 + b, X->cap, Y->cap);
    RAILS_REQUIRE(X->m == Y->m, "rails_gram: row mismatch %lld vs %lld", (long long)X->m, (long long)Y->m);
    RAILS_REQUIRE(a == 0 || b == 0 || (C_host && ldc >= a), "rails_gram: bad output buffer (ldc %d < %d)", ldc, a);
    if (a == 0 || b == 0) return RAILS_OK;
    size_t n = (size_t)a * b;
    RAILS_TRY(rails_small_reserve(c, n * sizeof(double)));
    RAILS_TRY(rails_pinned_reserve(c, n * sizeof(double)));
    if (X->m > 0)
        RAILS_TRY(rails_gram_dev(c, X->d + xc0, X->ld, Y->d + yc0, Y->ld, X->m, a, b, c->small));
    else
        RAILS_HIP_CHECK(hipMemsetAsync(c->small, 0, n * sizeof(double), c->stream));
    RAILS_TRY(rails_allreduce_dev(c, c->small, n));
    RAILS_HIP_CHECK(hipMemcpyAsync(c->pinned, c->small, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    RAILS_HIP_CHECK(rails_stream_sync(c));
    for (int j = 0; j < b; ++j) memcpy(C_host + (size_t)j * ldc, c->pinned + (size_t)j * a, sizeof(double) * a);
    return RAILS_OK;
}

// ---- column sums of squares ------------------------------------------------------------------------------------------------------
// The column norms of a wide window (the pre-scaling and the second stage of the rank decision of rails_orthogonalize_range, orth.hip)
// are the diagonal of its Gram matrix, but a 512 x 512 Gram product computed for its diagonal does 2 m 512^2 flops where reading the
// 8 m 512 bytes once suffices.  k_colnorms2: thread (tx, ty) of a block owns the column pair 2 tx, 2 tx + 1 of the window and every
// TY-th row of the block's slab, TX * TY = 256 with TX the next power of two above the number of pairs -- so a wave reads up to 1 KiB of
// one row with 16-byte loads (a window that starts at an odd column is read 8 bytes at a time, same sums).  A thread adds its rows in
// increasing order into four interleaved strands, the strands 0..3, then the TY row classes through LDS in a tree of fixed shape, then
// the slabs in k_reduce_partials: every order is fixed by (m, nc) alone, so two runs agree bit for bit.  nc <= 512.
namespace {

__global__ __launch_bounds__(256) void k_colnorms2(const double *__restrict__ X, int ldx, int nc, int64_t m, int64_t rows_per_slab, int tx_bits,
                                                   int vec_ok, double *__restrict__ partial)
{
    __shared__ double sh[256][2];
    const int TX = 1 << tx_bits, TY = 256 >> tx_bits;
    const int tx = threadIdx.x & (TX - 1), ty = threadIdx.x >> tx_bits;
    const int c = 2 * tx;
    const bool has0 = c < nc, has1 = c + 1 < nc;
    const int64_t r_begin = (int64_t)blockIdx.x * rows_per_slab;
    const int64_t r_end = r_begin + rows_per_slab < m ? r_begin + rows_per_slab : m;
    double s0[4] = {0.0, 0.0, 0.0, 0.0}, s1[4] = {0.0, 0.0, 0.0, 0.0};
    if (has0) {
        const bool pair = has1 && vec_ok;
        auto load = [&](int64_t r, double &a, double &b) {
            const double *src = X + r * ldx + c;
            if (pair) {
                const v2f64 t = *reinterpret_cast<const v2f64 *>(src);
                a = t.x;
                b = t.y;
            } else {
                a = src[0];
                b = has1 ? src[1] : 0.0;
            }
        };
        int64_t r = r_begin + ty;
        for (; r + 3 * (int64_t)TY < r_end; r += 4 * (int64_t)TY) { // four rows in flight, one per strand
            double a[4], b[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) load(r + s * (int64_t)TY, a[s], b[s]);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                s0[s] += a[s] * a[s];
                s1[s] += b[s] * b[s];
            }
        }
#pragma unroll
        for (int s = 0; s < 3; ++s) // at most three rows are left: strands 0, 1, 2
            if (r + s * (int64_t)TY < r_end) {
                double a, b;
                load(r + s * (int64_t)TY, a, b);
                s0[s] += a * a;
                s1[s] += b * b;
            }
    }
    sh[threadIdx.x][0] = ((s0[0] + s0[1]) + s0[2]) + s0[3];
    sh[threadIdx.x][1] = ((s1[0] + s1[1]) + s1[2]) + s1[3];
    __syncthreads();
    for (int half = TY >> 1; half > 0; half >>= 1) { // row class ty += row class ty + half: a tree of fixed shape
        if (ty < half) {
            sh[threadIdx.x][0] += sh[threadIdx.x + (half << tx_bits)][0];
            sh[threadIdx.x][1] += sh[threadIdx.x + (half << tx_bits)][1];
        }
        __syncthreads();
    }
    if (ty == 0 && has0) {
        double *dst = partial + (int64_t)blockIdx.x * nc + c;
        dst[0] = sh[tx][0];
        if (has1) dst[1] = sh[tx][1];
    }
}

} // namespace

// out_dev[j] = sum over the local rows of X[:, j]^2, j < nc <= 512 (no all-reduce, no host copy)
int rails_colnorms2_dev(rails_ctx *c, const double *X, int ldx, int64_t m, int nc, double *out_dev)
{
    if (nc <= 0) return RAILS_OK;
    if (m <= 0) {
        RAILS_HIP_CHECK(hipMemsetAsync(out_dev, 0, (size_t)nc * sizeof(double), c->stream));
        return RAILS_OK;
    }
    const int pairs = (nc + 1) / 2;
    int tx_bits = 0;
    while ((1 << tx_bits) < pairs) ++tx_bits; // <= 8: nc <= 512
    const int TY = 256 >> tx_bits;
    // slabs of at least 8 rows per thread, at most 1024 of them
    int64_t nslab = std::max<int64_t>(1, std::min<int64_t>(1024, m / ((int64_t)TY * 8)));
    const int64_t rps = (m + nslab - 1) / nslab;
    nslab = (m + rps - 1) / rps;
    RAILS_TRY(rails_ws_reserve(c, (size_t)nslab * nc * sizeof(double)));
    const int vec_ok = ((((uintptr_t)X) & 15) == 0 && (ldx % 2) == 0) ? 1 : 0;
    RAILS_LAUNCH(k_colnorms2, dim3((unsigned)nslab), dim3(256), 0, c->stream, X, ldx, nc, m, rps, tx_bits, vec_ok, c->ws);
    RAILS_LAUNCH(k_reduce_partials, dim3((unsigned)((nc + 63) / 64)), dim3(1024), 0, c->stream, c->ws, nslab, (int64_t)nc, out_dev);
    RAILS_HIP_CHECK(hipGetLastError());
    return RAILS_OK;
}

extern "C" int rails_panel_colnorms2(rails_ctx *c, const rails_panel *X, int c0, int nc, double *out_host)
{
    if (c) hipSetDevice(c->device);
    RAILS_REQUIRE(c && X, "rails_panel_colnorms2: null argument");
    RAILS_REQUIRE(c0 >= 0 && nc >= 0 && c0 + nc <= X->cap, "rails_panel_colnorms2: window [%d,%d) outside capacity %d", c0, c0 + nc, X->cap);
    RAILS_REQUIRE(nc == 0 || out_host, "rails_panel_colnorms2: null output buffer");
    if (nc == 0) return RAILS_OK;
    RAILS_TRY(rails_small_reserve(c, (size_t)nc * sizeof(double)));
    RAILS_TRY(rails_pinned_reserve(c, (size_t)nc * sizeof(double)));
    for (int j0 = 0; j0 < nc; j0 += 512) // every column is read once whatever nc
        RAILS_TRY(rails_colnorms2_dev(c, X->d + c0 + j0, X->ld, X->m, std::min(512, nc - j0), c->small + j0));
    RAILS_TRY(rails_allreduce_dev(c, c->small, (size_t)nc));
    RAILS_HIP_CHECK(hipMemcpyAsync(c->pinned, c->small, (size_t)nc * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    RAILS_HIP_CHECK(rails_stream_sync(c));
    memcpy(out_host, c->pinned, (size_t)nc * sizeof(double));
    return RAILS_OK;
}

// ---- deferred small results --------------------------------------------------------------------------------------------------
// The block orthogonalisation of the coordinate-space back end is a chain Gram -> update -> Gram -> Cholesky -> update ... whose small
// matrices the host only needs for bookkeeping.  With these entry points the chain runs on the device without the host in between:
// a Gram result stays in a slot of a device arena (and is copied to its pinned mirror, to be read after a later synchronisation), the
// next update takes its coefficients from the slot, the Cholesky factor of a w x w slot is inverted into another slot by a small
// kernel.  Nothing here synchronises.

namespace {

// rows [0, k) of the r columns of a slot (leading dimension ld) packed into k x r
__global__ void k_compact_cols(const double *__restrict__ src, int ld, int k, int r, double *__restrict__ dst)
{
    const int64_t n = (int64_t)k * r;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) dst[q] = src[(q / k) * ld + (q % k)];
}

// G (w x w, symmetric positive definite, w <= 48) -> M = D^-1 R^-1 with D = sqrt(diag G), R'R = D^-1 G D^-1 (upper triangular):
// X M has orthonormal columns when X'X = G.  One wave, lane j = column j: a right-looking Cholesky (row i of R, then the rank-one update
// of the columns behind it: w steps of at most w dependent LDS round trips each) and one back substitution per lane for R^-1 -- about
// ten microseconds at w = 17, where one thread working through the ~w^3 / 2 dependent operations took 110 (two of these sit on the
// device's critical path of every trip).  A G that is not positive definite gives NaNs (the host repeats the factorisation on its copy
// of G and decides).
__global__ __launch_bounds__(64) void k_small_chol(const double *__restrict__ G, int w, double *__restrict__ M)
{
    constexpr int LD = 49; // up to 48 columns (Expand size 32 + the prefetched random vector: 33), rows of S a bank apart
    __shared__ double S[48 * LD], Ri[48 * LD], d[48];
    const int t = threadIdx.x;
    const bool mine = t < w;
    for (int q = t; q < w * w; q += 64) S[(q / w) * LD + (q % w)] = G[q]; // S[col][row]
    __syncthreads();
    if (mine) d[t] = sqrt(S[t * LD + t]);
    __syncthreads();
    for (int q = t; q < w * w; q += 64) S[(q / w) * LD + (q % w)] /= d[q % w] * d[q / w];
    __syncthreads();
    // R[i][j] (i <= j) ends up at S[j][i]
    for (int i = 0; i < w; ++i) {
        const double piv = sqrt(S[i * LD + i]);
        double rij = 0.0;
        if (mine && t >= i) rij = (t == i) ? piv : S[t * LD + i] / piv;
        __syncthreads();
        if (mine && t >= i) S[t * LD + i] = rij;
        __syncthreads();
        if (mine && t > i)
            for (int l = i + 1; l <= t; ++l) S[t * LD + l] -= S[l * LD + i] * rij;
        __syncthreads();
    }
    // column t of R^-1 by back substitution (every lane its own column: no exchange)
    if (mine) {
        for (int l = 0; l < w; ++l) Ri[t * LD + l] = 0.0;
        for (int i = t; i >= 0; --i) {
            double s = (i == t) ? 1.0 : 0.0;
            for (int l = i + 1; l <= t; ++l) s -= S[l * LD + i] * Ri[t * LD + l];
            Ri[t * LD + i] = s / S[i * LD + i];
        }
    }
    __syncthreads();
    for (int q = t; q < w * w; q += 64) {
        const int j = q / w, i = q % w;
        M[q] = i <= j ? Ri[j * LD + i] / d[i] : 0.0;
    }
}

} // namespace

extern "C" int rails_deferred_reserve(rails_ctx *c, int nslots, int64_t doubles_per_slot)
{
    RAILS_REQUIRE(c && nslots >= 1 && doubles_per_slot >= 1, "rails_deferred_reserve: bad argument");
    hipSetDevice(c->device);
    if (c->defer_dev && c->defer_nslots >= nslots && c->defer_slot >= (size_t)doubles_per_slot) return RAILS_OK;
    RAILS_HIP_CHECK(rails_stream_sync(c));
    if (c->defer_dev) hipFree(c->defer_dev);
    if (c->defer_pin) hipHostFree(c->defer_pin);
    c->defer_dev = c->defer_pin = nullptr;
    const size_t slot = ((size_t)doubles_per_slot * 3 / 2 + 63) / 64 * 64, bytes = slot * (size_t)nslots * sizeof(double);
    c->n_dev_alloc++;
    RAILS_HIP_CHECK(hipMalloc((void **)&c->defer_dev, bytes));
    RAILS_HIP_CHECK(hipHostMalloc((void **)&c->defer_pin, bytes, hipHostMallocDefault));
    c->defer_slot = slot;
    c->defer_nslots = nslots;
    return RAILS_OK;
}

#define RAILS_SLOT_CHECK(slot, n, what)                                                                                                    \
    RAILS_REQUIRE(c && c->defer_dev && (slot) >= 0 && (slot) < c->defer_nslots && (size_t)(n) <= c->defer_slot,                            \
                  what ": slot %d / %lld doubles outside the arena (rails_deferred_reserve)", (int)(slot), (long long)(n))

// slot <- X[:, xc0:xc0+a]' * Y[:, yc0:yc0+b] (a x b, column-major, leading dimension a), summed over the ranks; also on its way to the
// pinned mirror of the slot
extern "C" int rails_gram_deferred(rails_ctx *c, const rails_panel *X, int xc0, int a, const rails_panel *Y, int yc0, int b, int slot)
{
    if (c) hipSetDevice(c->device);
    RAILS_REQUIRE(c && X && Y, "rails_gram_deferred: null argument");
    RAILS_REQUIRE(a >= 1 && b >= 1 && xc0 >= 0 && yc0 >= 0 && xc0 + a <= X->cap && yc0 + b <= Y->cap && X->m == Y->m, "rails_gram_deferred: bad windows");
    const size_t n = (size_t)a * b;
    RAILS_SLOT_CHECK(slot, n, "rails_gram_deferred");
    double *out = c->defer_dev + (size_t)slot * c->defer_slot;
    if (X->m > 0)
        RAILS_TRY(rails_gram_dev(c, X->d + xc0, X->ld, Y->d + yc0, Y->ld, X->m, a, b, out));
    else
        RAILS_HIP_CHECK(hipMemsetAsync(out, 0, n * sizeof(double), c->stream));
    RAILS_TRY(rails_allreduce_dev(c, out, n));
    RAILS_HIP_CHECK(hipMemcpyAsync(c->defer_pin + (size_t)slot * c->defer_slot, out, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return RAILS_OK;
}

// Y[:, yc0:yc0+r] = beta Y + alpha X[:, xc0:xc0+k] * C, C = rows [0, k) of the r columns held in a slot with leading dimension ld
extern "C" int rails_panel_gemm_deferred(rails_ctx *c, double alpha, const rails_panel *X, int xc0, int k, int slot, int ld, int r, double beta,
                                         rails_panel *Y, int yc0)
{
    if (c) hipSetDevice(c->device);
    RAILS_REQUIRE(c && X && Y, "rails_panel_gemm_deferred: null argument");
    RAILS_REQUIRE(k >= 1 && r >= 1 && r <= 256 && ld >= k && xc0 >= 0 && yc0 >= 0 && xc0 + k <= X->cap && yc0 + r <= Y->cap && X->m == Y->m,
                  "rails_panel_gemm_deferred: bad shapes");
    RAILS_SLOT_CHECK(slot, (size_t)ld * r, "rails_panel_gemm_deferred");
    if (X->d == Y->d) RAILS_REQUIRE(xc0 == yc0 || xc0 + k <= yc0 || yc0 + r <= xc0, "rails_panel_gemm_deferred: partially overlapping windows of one panel");
    if (X->m == 0) return RAILS_OK;
    const double *C = c->defer_dev + (size_t)slot * c->defer_slot;
    if (ld != k) {
        RAILS_TRY(rails_small_reserve(c, (size_t)k * r * sizeof(double)));
        RAILS_LAUNCH(k_compact_cols, dim3((unsigned)std::min<int64_t>(256, ((int64_t)k * r + 255) / 256)), dim3(256), 0, c->stream, C, ld, k, r, c->small);
        C = c->small;
    }
    return rails_panel_gemm_dev(c, alpha, X->d + xc0, X->ld, k, C, r, beta, Y->d + yc0, Y->ld, X->m);
}

// ---- first update and second projection of a block in ONE pass over the basis ----------------------------------------------------
// Round 2 of the block orthogonalisation (Stl path: the second sweep of src/StlWrapper.cpp:314-344) needs Y' = Y - X C1 and then
// C2 = X' Y'.  As two kernels that is two passes over X (2.8 GB each at 350 basis columns x 1M rows: 0.6 + 0.42 ms); here a workgroup
// takes 16 rows at a time, its four waves split X's columns in interleaved blocks of 16 and keep their part of the tile in registers:
//   step 1  partial Y' tile = X_part C_part on the MFMA (layout A: lane (row, k mod 4) holds four consecutive columns of its row),
//           summed over the waves through LDS, Y' written back and kept in LDS;
//   step 2  C2_part += X_part' Y' : the same registers, turned around through 2 KiB of LDS per wave into the layout in which the
//           ROWS are the contraction index (lane (column, row mod 4)).
// Columns beyond 16 of the update (the prefetched random vector that rides at the end of an A*W block: r = 17) are done with plain
// multiply-adds on the values the lanes hold anyway -- a second MFMA column tile for one column doubles the matrix work and makes the
// pass MFMA-bound.  The next tile's rows are loaded while this one is worked on.  Per-workgroup partial C2 tiles go to the workspace
// and are summed in a fixed order by k_reduce_partials, like every Gram matrix here.
// Y is read from Yp (leading dimension ldy) and Y' is written to Yo (leading dimension ldo, no alignment assumed): the same place for the
// update in place, or another panel -- a block that is orthogonalised next is better off in a compact panel of its own than in the tail
// of the basis, where its 136 bytes per row are spread over two or three cache lines.  Only the two stores of Y' know Yo.
template <int NBW, int NE>
__global__ __launch_bounds__(256, (NBW <= 6 ? 2 : 1)) void k_update_gram(double alpha, const double *__restrict__ X, int ldx, int k, const double *__restrict__ C, int r,
                                                     const double *Yp, int ldy, double *Yo, int ldo, int r2, int64_t m, int64_t ntiles,
                                                     double *__restrict__ partial)
{
    constexpr int KMAX = 64 * NBW, RL = 20; // LDS row length of C (doubles): 16 + 4 keeps the four k-groups of a read on disjoint banks
    __shared__ double Cs[KMAX * RL];
    __shared__ double red[4][4][64]; // step-1 partial tiles: [wave][result register][lane]
    __shared__ double rede[4][1][16];
    __shared__ double awL[16 * 16];  // the updated tile, [row][column], zero beyond r2 columns / m rows
    __shared__ __attribute__((aligned(16))) double T[4][16 * 16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, kk = lane >> 4;
    for (int idx = threadIdx.x; idx < KMAX * RL; idx += 256) {
        const int kl = idx / RL, j = idx % RL;
        Cs[idx] = (kl < k && j < r) ? C[kl + (int64_t)j * k] : 0.0;
    }
    v4f64 acc2[NBW];
#pragma unroll
    for (int b = 0; b < NBW; ++b) acc2[b] = (v4f64){0.0, 0.0, 0.0, 0.0};

    // Loads without branches and without selects (either makes the compiler wait for a block's loads before it issues the next
    // block's: six memory latencies per tile): addresses are clamped into the panel and what comes back from outside the operands is
    // multiplied by zeros -- rows past m repeat row m - 1 and meet the zero rows of the Y' tile in step 2 (their step-1 results are
    // not stored); columns k .. k4 - 1 (k rounded up to 4) are the leading columns of Y itself (the host checks that Y sits right
    // behind X and is that wide), columns from k4 on repeat column 0, and both meet zero rows of C (rows of C2 that are not written).
    const int k4 = (k + 3) & ~3;
    auto fetch = [&](int64_t tile, double (*xs)[4]) {
        const int64_t myrow = (tile < ntiles ? tile : ntiles - 1) * 16 + li;
        const double *xrow = X + (myrow < m ? myrow : m - 1) * ldx;
#pragma unroll
        for (int b = 0; b < NBW; ++b) {
            const int kcol = (b * 4 + wave) * 16 + 4 * kk;
            const double *src = xrow + (kcol < k4 ? kcol : 0);
            const v2f64 t0 = *reinterpret_cast<const v2f64 *>(src);
            const v2f64 t1 = *reinterpret_cast<const v2f64 *>(src + 2);
            xs[b][0] = t0.x;
            xs[b][1] = t0.y;
            xs[b][2] = t1.x;
            xs[b][3] = t1.y;
        }
    };
    // this thread's entry of a tile of Y: result register `wave` of lane `lane` is row kk + 4 wave, column li; the threads that finish
    // the columns beyond 16: row erow, column 16 + ene
    const int erow = threadIdx.x & 15, ene = threadIdx.x >> 4;
    auto fetch_y = [&](int64_t tile, double &yv, double &ye) {
        const int64_t t16 = (tile < ntiles ? tile : ntiles - 1) * 16;
        const int64_t yrow = t16 + kk + 4 * wave, er = t16 + erow;
        yv = Yp[(yrow < m ? yrow : m - 1) * ldy + (li < r ? li : 0)]; // (used only where it is valid)
        ye = NE > 0 ? Yp[(er < m ? er : m - 1) * ldy + (16 + ene < r ? 16 + ene : 0)] : 0.0;
    };
    // one tile: `xs`, `yv`, `ye` were requested while the tile before was worked on; the next tile's go out first (two register sets
    // that swap roles: no copies, and a wait for this tile's values does not wait for the next one's)
    auto work = [&](int64_t tile, double (*xs)[4], double yv, double ye, double (*xn)[4], double &yvn, double &yen) {
        const int64_t row0 = tile * 16;
        fetch(tile + gridDim.x, xn); // (zeros past the last tile)
        fetch_y(tile + gridDim.x, yvn, yen);
        const int64_t yrow = row0 + kk + 4 * wave;
        const bool yok = yrow < m && li < r;
        const bool eok = ene < NE && 16 + ene < r && row0 + erow < m;
        // step 1
        v4f64 p = (v4f64){0.0, 0.0, 0.0, 0.0};
        double e[NE > 0 ? NE : 1];
#pragma unroll
        for (int q = 0; q < NE; ++q) e[q] = 0.0;
#pragma unroll
        for (int b = 0; b < NBW; ++b)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const double *crow = &Cs[((b * 4 + wave) * 16 + 4 * kk + s) * RL];
                p = mfma_f64(xs[b][s], crow[li], p);
#pragma unroll
                for (int q = 0; q < NE; ++q) e[q] += xs[b][s] * crow[16 + q];
            }
#pragma unroll
        for (int v = 0; v < 4; ++v) red[wave][v][lane] = p[v];
#pragma unroll
        for (int q = 0; q < NE; ++q) {
            double t = e[q];
            t += __shfl_xor(t, 16, 64);
            t += __shfl_xor(t, 32, 64);
            if (kk == 0) rede[wave][q][li] = t;
        }
        __syncthreads();
        {
            const double sum = ((red[0][wave][lane] + red[1][wave][lane]) + red[2][wave][lane]) + red[3][wave][lane];
            const double ynew = yv + alpha * sum;
            if (yok) Yo[yrow * ldo + li] = ynew;
            awL[(kk + 4 * wave) * 16 + li] = (yok && li < r2) ? ynew : 0.0;
            if (NE > 0 && eok) {
                const double se = ((rede[0][ene][erow] + rede[1][ene][erow]) + rede[2][ene][erow]) + rede[3][ene][erow];
                Yo[(row0 + erow) * ldo + 16 + ene] = ye + alpha * se;
            }
        }
        __syncthreads();
        // step 2
        double bq[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) bq[q] = awL[(4 * q + kk) * 16 + li];
        double *Tw = T[wave];
#pragma unroll
        for (int b = 0; b < NBW; ++b) {
            *reinterpret_cast<v2f64 *>(&Tw[li * 16 + 4 * kk]) = (v2f64){xs[b][0], xs[b][1]};
            *reinterpret_cast<v2f64 *>(&Tw[li * 16 + 4 * kk + 2]) = (v2f64){xs[b][2], xs[b][3]};
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            double a4[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) a4[q] = Tw[(4 * q + kk) * 16 + li];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int q = 0; q < 4; ++q) acc2[b] = mfma_f64(a4[q], bq[q], acc2[b]);
        }
    };
    double xa[NBW][4], xb[NBW][4], yva, yea, yvb, yeb;
    fetch(blockIdx.x, xa);
    fetch_y(blockIdx.x, yva, yea);
    __syncthreads();
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += 2 * (int64_t)gridDim.x) {
        work(tile, xa, yva, yea, xb, yvb, yeb);
        if (tile + gridDim.x < ntiles) work(tile + gridDim.x, xb, yvb, yeb, xa, yva, yea);
    }
    double *P = partial + (int64_t)blockIdx.x * k * r2;
#pragma unroll
    for (int b = 0; b < NBW; ++b)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int ci = (b * 4 + wave) * 16 + kk + 4 * v; // D row -> X column
            if (ci < k && li < r2) P[ci + (int64_t)li * k] = acc2[b][v];
        }
}

// The same pass on another schedule: the same partial sums, formed and added in the same order, so the same bits
// as k_update_gram; what differs is where the operands wait.
//   C in registers.  A lane multiplies every tile by the same 4 NBW entries of C (rows (4b + wave) 16 + 4 kk + s of column li), so it
//     loads them once: step 1 is 4 NBW MFMAs back to back with no LDS read and no wait between them, and the 40 to 80 KiB copy of C
//     leaves the LDS.  Column 16 (the 17th column's multiply-adds) stays in the LDS, 64 NBW doubles read 32 bytes at a time: its values
//     feed the vector unit, not the MFMA chain, and with them in registers <6, 1> does not fit 256 registers.
//   One set of X registers, refilled block by block.  As soon as step 1 has used a block of this tile, the same block of the next tile
//     is asked for into the same registers: every load has a whole tile's time to arrive, the loads are spread over the tile, and the
//     48 registers of the second set are free (two sets and C in registers spill from <5, 1> on, and a spill reload in the loop made
//     the compiler wait for every load in flight).
//   One turn-around per tile.  A block goes into the LDS for step 2 right before step 1 multiplies it (NBW slabs of 2 KiB per wave), so
//     the stores run under step 1's MFMAs and step 2 reads the slabs back without a store -> load round trip per block, a block's
//     four values asked for before the MFMAs of the block before.  Rows keep their stride of 128 bytes, and the 16-byte chunks of a
//     row are exchanged by (chunk ^ (row & 7)): the eight lanes of a 16-byte store's lane group hit eight different chunks (they all
//     hit the same one before: 8-way), and the 32 lanes of an 8-byte load's group still read two whole rows, one per half of the banks.
// The clamping of rows and columns, the cross-wave sums and the stores are those of k_update_gram, text for text.
template <int NBW, int NE>
__global__ __launch_bounds__(256, (NBW <= 6 ? 2 : 1)) void k_update_gram_p(double alpha, const double *__restrict__ X, int ldx, int k, const double *__restrict__ C, int r,
                                                       const double *Yp, int ldy, double *Yo, int ldo, int r2, int64_t m, int64_t ntiles,
                                                       double *__restrict__ partial)
{
    __shared__ double red[4][4][64]; // step-1 partial tiles: [wave][result register][lane]
    __shared__ double rede[4][1][16];
    __shared__ double awL[16 * 16];  // the updated tile, [row][column], zero beyond r2 columns / m rows
    __shared__ __attribute__((aligned(16))) double T[4][NBW][16 * 16];
    __shared__ __attribute__((aligned(16))) double c16[NE > 0 ? 64 * NBW : 2]; // column 16 of C, zero beyond k rows (the registers hold no more)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, kk = lane >> 4;
    // this lane's entries of C, zero beyond k rows / r columns
    double cr[NBW][4];
#pragma unroll
    for (int b = 0; b < NBW; ++b)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int kl = (b * 4 + wave) * 16 + 4 * kk + s;
            cr[b][s] = (kl < k && li < r) ? C[kl + (int64_t)li * k] : 0.0;
        }
    if (NE > 0) {
        for (int kl = threadIdx.x; kl < 64 * NBW; kl += 256) c16[kl] = (kl < k && 16 < r) ? C[kl + (int64_t)16 * k] : 0.0;
        __syncthreads();
    }
    v4f64 acc2[NBW];
#pragma unroll
    for (int b = 0; b < NBW; ++b) acc2[b] = (v4f64){0.0, 0.0, 0.0, 0.0};

    // One set of X registers: a block's part of the NEXT tile is asked for as soon as step 1 has used that block of this tile (its copy
    // for step 2 is in the LDS by then), so every load has a whole tile's time to arrive, the loads of a tile are spread over step 1
    // and not sent in one burst, and a wait for block b waits for nothing behind it.  Addresses are clamped as in k_update_gram: no
    // branches and no selects on what comes back, zeros of C and of the Y' tile meet whatever lies outside the operands.
    const int k4 = (k + 3) & ~3;
    auto xrow_of = [&](int64_t tile) {
        const int64_t myrow = (tile < ntiles ? tile : ntiles - 1) * 16 + li;
        return X + (myrow < m ? myrow : m - 1) * ldx;
    };
    auto fetch_block = [&](const double *xrow, int b, double *xs) {
        const int kcol = (b * 4 + wave) * 16 + 4 * kk;
        const double *src = xrow + (kcol < k4 ? kcol : 0);
        const v2f64 t0 = *reinterpret_cast<const v2f64 *>(src);
        const v2f64 t1 = *reinterpret_cast<const v2f64 *>(src + 2);
        xs[0] = t0.x;
        xs[1] = t0.y;
        xs[2] = t1.x;
        xs[3] = t1.y;
    };
    const int erow = threadIdx.x & 15, ene = threadIdx.x >> 4;
    auto fetch_y = [&](int64_t tile, double &yv, double &ye) {
        const int64_t t16 = (tile < ntiles ? tile : ntiles - 1) * 16;
        const int64_t yrow = t16 + kk + 4 * wave, er = t16 + erow;
        yv = Yp[(yrow < m ? yrow : m - 1) * ldy + (li < r ? li : 0)]; // (used only where it is valid)
        ye = NE > 0 ? Yp[(er < m ? er : m - 1) * ldy + (16 + ene < r ? 16 + ene : 0)] : 0.0;
    };
    // the turn-around's places (doubles within a slab of 16 x 16): this lane's two 16-byte chunks of row li on the way in, its entry
    // (row 4 q + kk, column li) on the way out (rows 4 q + kk and 4 (q + 2) + kk have the same three low bits: two places and a constant)
    const int tw0 = li * 16 + 2 * ((2 * kk) ^ (li & 7)), tw1 = li * 16 + 2 * ((2 * kk + 1) ^ (li & 7));
    const int tr0 = kk * 16 + 2 * ((li >> 1) ^ kk) + (li & 1), tr1 = (4 + kk) * 16 + 2 * ((li >> 1) ^ (4 + kk)) + (li & 1);
    double xs[NBW][4], yv, ye;
    {
        const double *xrow = xrow_of(blockIdx.x);
#pragma unroll
        for (int b = 0; b < NBW; ++b) fetch_block(xrow, b, xs[b]);
        fetch_y(blockIdx.x, yv, ye);
    }
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row0 = tile * 16;
        const double *xnext = xrow_of(tile + gridDim.x); // (past the last tile: the last tile again, and nobody uses it)
        const int64_t yrow = row0 + kk + 4 * wave;
        const bool yok = yrow < m && li < r;
        const bool eok = ene < NE && 16 + ene < r && row0 + erow < m;
        // step 1
        v4f64 p = (v4f64){0.0, 0.0, 0.0, 0.0};
        double e[NE > 0 ? NE : 1];
#pragma unroll
        for (int q = 0; q < NE; ++q) e[q] = 0.0;
#pragma unroll
        for (int b = 0; b < NBW; ++b) {
            *reinterpret_cast<v2f64 *>(&T[wave][b][tw0]) = (v2f64){xs[b][0], xs[b][1]};
            *reinterpret_cast<v2f64 *>(&T[wave][b][tw1]) = (v2f64){xs[b][2], xs[b][3]};
            double ce[4] = {0.0, 0.0, 0.0, 0.0};
            if (NE > 0) {
                const v2f64 c0 = *reinterpret_cast<const v2f64 *>(&c16[(b * 4 + wave) * 16 + 4 * kk]);
                const v2f64 c1 = *reinterpret_cast<const v2f64 *>(&c16[(b * 4 + wave) * 16 + 4 * kk + 2]);
                ce[0] = c0.x, ce[1] = c0.y, ce[2] = c1.x, ce[3] = c1.y;
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                p = mfma_f64(xs[b][s], cr[b][s], p);
#pragma unroll
                for (int q = 0; q < NE; ++q) e[q] += xs[b][s] * ce[s];
            }
            __builtin_amdgcn_sched_barrier(0); // (the load below stays below: above, it needs a second set of registers)
            fetch_block(xnext, b, xs[b]);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) red[wave][v][lane] = p[v];
#pragma unroll
        for (int q = 0; q < NE; ++q) {
            double t = e[q];
            t += __shfl_xor(t, 16, 64);
            t += __shfl_xor(t, 32, 64);
            if (kk == 0) rede[wave][q][li] = t;
        }
        __syncthreads();
        {
            const double sum = ((red[0][wave][lane] + red[1][wave][lane]) + red[2][wave][lane]) + red[3][wave][lane];
            const double ynew = yv + alpha * sum;
            if (yok) Yo[yrow * ldo + li] = ynew;
            awL[(kk + 4 * wave) * 16 + li] = (yok && li < r2) ? ynew : 0.0;
            if (NE > 0 && eok) {
                const double se = ((rede[0][ene][erow] + rede[1][ene][erow]) + rede[2][ene][erow]) + rede[3][ene][erow];
                Yo[(row0 + erow) * ldo + 16 + ene] = ye + alpha * se;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        fetch_y(tile + gridDim.x, yv, ye);
        __syncthreads();
        // step 2 (a block's four values are asked for before the MFMAs of the block before, and no earlier)
        double bq[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) bq[q] = awL[(4 * q + kk) * 16 + li];
        double a4[2][4];
#pragma unroll
        for (int q = 0; q < 4; ++q) a4[0][q] = T[wave][0][((q & 1) ? tr1 : tr0) + 128 * (q >> 1)];
#pragma unroll
        for (int b = 0; b < NBW; ++b) {
            if (b + 1 < NBW) {
#pragma unroll
                for (int q = 0; q < 4; ++q) a4[(b + 1) & 1][q] = T[wave][b + 1][((q & 1) ? tr1 : tr0) + 128 * (q >> 1)];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < 4; ++q) acc2[b] = mfma_f64(a4[b & 1][q], bq[q], acc2[b]);
            __builtin_amdgcn_sched_barrier(0);
        }
        // (the next tile's stores into T stay behind these loads)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    double *P = partial + (int64_t)blockIdx.x * k * r2;
#pragma unroll
    for (int b = 0; b < NBW; ++b)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int ci = (b * 4 + wave) * 16 + kk + 4 * v; // D row -> X column
            if (ci < k && li < r2) P[ci + (int64_t)li * k] = acc2[b][v];
        }
}

template <int NBW>
static void launch_update_gram(rails_ctx *c, int ne, unsigned grid, double alpha, const double *X, int ldx, int k, const double *C, int r, const double *Y, int ldy,
                               double *Yo, int ldo, int r2, int64_t m, int64_t ntiles)
{
    const bool pipeline = dense_update_gram_pipeline();
    if (pipeline && ne == 0)
        RAILS_LAUNCH((k_update_gram_p<NBW, 0>), dim3(grid), dim3(256), 0, c->stream, alpha, X, ldx, k, C, r, Y, ldy, Yo, ldo, r2, m, ntiles, c->ws);
    else if (pipeline)
        RAILS_LAUNCH((k_update_gram_p<NBW, 1>), dim3(grid), dim3(256), 0, c->stream, alpha, X, ldx, k, C, r, Y, ldy, Yo, ldo, r2, m, ntiles, c->ws);
    else if (ne == 0)
        RAILS_LAUNCH((k_update_gram<NBW, 0>), dim3(grid), dim3(256), 0, c->stream, alpha, X, ldx, k, C, r, Y, ldy, Yo, ldo, r2, m, ntiles, c->ws);
    else
        RAILS_LAUNCH((k_update_gram<NBW, 1>), dim3(grid), dim3(256), 0, c->stream, alpha, X, ldx, k, C, r, Y, ldy, Yo, ldo, r2, m, ntiles, c->ws);
    c->last_update_gram_form = pipeline ? 2 : 1;
    c->last_update_gram_nbw = NBW;
}

// Y[:, yc0:yc0+r] += alpha X[:, xc0:xc0+k] C (C on the host, k x r, leading dimension ldc), then slot <- X[:, xc0:xc0+k]' Y[:, yc0:yc0+r2]
// (k x r2, leading dimension k, summed over the ranks, on its way to the slot's pinned mirror).  One pass over X where the shapes
// allow (r <= 17, r2 <= 16, 32 <= k <= 512), the two separate kernels otherwise.
// The updated columns go to Yout[:, oc0:oc0+r] and the input Y stays as it was; Yout = Y with oc0 = yc0 is the update in place
// (rails_update_gram_deferred).  The arithmetic does not know where the result goes: both forms give the same bits.  Where the two
// separate kernels run, Y is copied to Yout first (rails_panel_copy's kernel) and they work on Yout.
extern "C" int rails_update_gram_deferred_out(rails_ctx *c, double alpha, const rails_panel *X, int xc0, int k, const double *C_host, int ldc, int r,
                                              const rails_panel *Y, int yc0, rails_panel *Yout, int oc0, int r2, int slot)
{
    if (c) hipSetDevice(c->device);
    rails_slow_guard slow__(c, "rails_update_gram_deferred", k, r);
    RAILS_REQUIRE(c && X && Y && Yout && C_host, "rails_update_gram_deferred: null argument");
    RAILS_REQUIRE(k >= 1 && r >= 1 && r <= 256 && r2 >= 1 && r2 <= r && ldc >= k && xc0 >= 0 && yc0 >= 0 && xc0 + k <= X->cap && yc0 + r <= Y->cap && X->m == Y->m,
                  "rails_update_gram_deferred: bad shapes");
    RAILS_REQUIRE(oc0 >= 0 && oc0 + r <= Yout->cap && Yout->m == X->m, "rails_update_gram_deferred: output window [%d,%d) outside capacity %d, or row mismatch", oc0,
                  oc0 + r, Yout->cap);
    if (X->d == Y->d) RAILS_REQUIRE(xc0 + k <= yc0 || yc0 + r <= xc0, "rails_update_gram_deferred: overlapping windows of one panel");
    if (X->d == Yout->d) RAILS_REQUIRE(xc0 + k <= oc0 || oc0 + r <= xc0, "rails_update_gram_deferred: overlapping windows of one panel");
    if (Y->d == Yout->d) RAILS_REQUIRE(yc0 == oc0 || yc0 + r <= oc0 || oc0 + r <= yc0, "rails_update_gram_deferred: partially overlapping windows of one panel");
    const size_t n = (size_t)k * r2;
    RAILS_SLOT_CHECK(slot, n, "rails_update_gram_deferred");
    double *out = c->defer_dev + (size_t)slot * c->defer_slot;
    if (X->m == 0) {
        RAILS_HIP_CHECK(hipMemsetAsync(out, 0, n * sizeof(double), c->stream));
    } else {
        const size_t nc = (size_t)k * r;
        RAILS_TRY(rails_small_reserve(c, nc * sizeof(double)));
        RAILS_TRY(rails_pinned_begin_write(c, nc * sizeof(double)));
        for (int j = 0; j < r; ++j) memcpy(c->pinned + (size_t)j * k, C_host + (size_t)j * ldc, sizeof(double) * k);
        RAILS_HIP_CHECK(hipMemcpyAsync(c->small, c->pinned, nc * sizeof(double), hipMemcpyHostToDevice, c->stream));
        RAILS_TRY(rails_pinned_end_write(c));
        static const int fused_env = getenv("RAILS_FUSED_UPDATE_GRAM") ? atoi(getenv("RAILS_FUSED_UPDATE_GRAM")) : 1;
        const double *Xp = X->d + xc0;
        const double *Ypp = Y->d + yc0;
        double *Yop = Yout->d + oc0;
        // (16-byte loads of four columns at a time: aligned rows, and the columns between k and k rounded up to 4 are Y's own)
        const int k4 = (k + 3) & ~3;
        const bool rows_ok = ((((uintptr_t)Xp) & 15) == 0 && (X->ld % 2) == 0) && (k4 == k || (X->d == Y->d && yc0 == xc0 + k && r >= k4 - k));
        if (fused_env && rows_ok && r <= 17 && r2 <= 16 && k >= 32 && k <= 512 && X->m >= 4096) {
            const int64_t ntiles = (X->m + 15) / 16;
            const unsigned grid = (unsigned)std::min<int64_t>(ntiles, 2 * (int64_t)std::max(c->num_cu, 1));
            const int ne = r > 16 ? r - 16 : 0;
            RAILS_TRY(rails_ws_reserve(c, (size_t)grid * n * sizeof(double)));
            if (k <= 256)
                launch_update_gram<4>(c, ne, grid, alpha, Xp, X->ld, k, c->small, r, Ypp, Y->ld, Yop, Yout->ld, r2, X->m, ntiles);
            else if (k <= 320 && dense_tile_fit()) // (the waves' interleaved blocks of 16 columns: 20 of them instead of 24)
                launch_update_gram<5>(c, ne, grid, alpha, Xp, X->ld, k, c->small, r, Ypp, Y->ld, Yop, Yout->ld, r2, X->m, ntiles);
            else if (k <= 384)
                launch_update_gram<6>(c, ne, grid, alpha, Xp, X->ld, k, c->small, r, Ypp, Y->ld, Yop, Yout->ld, r2, X->m, ntiles);
            else
                launch_update_gram<8>(c, ne, grid, alpha, Xp, X->ld, k, c->small, r, Ypp, Y->ld, Yop, Yout->ld, r2, X->m, ntiles);
            RAILS_LAUNCH(k_reduce_partials, dim3((unsigned)((n + 63) / 64)), dim3(1024), 0, c->stream, c->ws, (int64_t)grid, (int64_t)n, out);
            RAILS_HIP_CHECK(hipGetLastError());
            c->n_update_gram_fused++;
        } else {
            if (Yop != Ypp) RAILS_TRY(rails_panel_copy(c, Y, yc0, r, Yout, oc0));
            RAILS_TRY(rails_panel_gemm_dev(c, alpha, Xp, X->ld, k, c->small, r, 1.0, Yop, Yout->ld, X->m));
            RAILS_TRY(rails_gram_dev(c, Xp, X->ld, Yop, Yout->ld, X->m, k, r2, out));
        }
    }
    RAILS_TRY(rails_allreduce_dev(c, out, n));
    RAILS_HIP_CHECK(hipMemcpyAsync(c->defer_pin + (size_t)slot * c->defer_slot, out, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return RAILS_OK;
}

extern "C" int rails_update_gram_deferred(rails_ctx *c, double alpha, const rails_panel *X, int xc0, int k, const double *C_host, int ldc, int r,
                                          rails_panel *Y, int yc0, int r2, int slot)
{
    return rails_update_gram_deferred_out(c, alpha, X, xc0, k, C_host, ldc, r, Y, yc0, Y, yc0, r2, slot);
}

// slot_out <- D^-1 R^-1 for the w x w Gram matrix in slot_in (see k_small_chol)
extern "C" int rails_chol_inverse_deferred(rails_ctx *c, int slot_in, int w, int slot_out)
{
    if (c) hipSetDevice(c->device);
    RAILS_REQUIRE(c && w >= 1 && w <= 48 && slot_in != slot_out, "rails_chol_inverse_deferred: bad argument (w = %d)", w);
    RAILS_SLOT_CHECK(slot_in, (size_t)w * w, "rails_chol_inverse_deferred");
    RAILS_SLOT_CHECK(slot_out, (size_t)w * w, "rails_chol_inverse_deferred");
    RAILS_LAUNCH(k_small_chol, dim3(1), dim3(64), 0, c->stream, c->defer_dev + (size_t)slot_in * c->defer_slot, w, c->defer_dev + (size_t)slot_out * c->defer_slot);
    RAILS_HIP_CHECK(hipGetLastError());
    RAILS_HIP_CHECK(hipMemcpyAsync(c->defer_pin + (size_t)slot_out * c->defer_slot, c->defer_dev + (size_t)slot_out * c->defer_slot, (size_t)w * w * sizeof(double),
                                   hipMemcpyDeviceToHost, c->stream)); // (the mirror: diagnostics and tests)
    return RAILS_OK;
}

// the first n doubles of a slot's pinned mirror (valid once the stream has been synchronised after the call that filled the slot)
extern "C" int rails_deferred_fetch(rails_ctx *c, int slot, int64_t n, double *host_out)
{
    RAILS_REQUIRE(host_out && n >= 0, "rails_deferred_fetch: bad argument");
    RAILS_SLOT_CHECK(slot, n, "rails_deferred_fetch");
    memcpy(host_out, c->defer_pin + (size_t)slot * c->defer_slot, (size_t)n * sizeof(double));
    return RAILS_OK;
}

int rails_panel_gemm_dev(rails_ctx *c, double alpha, const double *X, int ldx, int k, const double *C_dev, int r, double beta,
                         double *Y, int ldy, int64_t m)
{
    if (r <= 0 || m <= 0) return RAILS_OK;
    int vec_ok = ((((uintptr_t)X) & 15) == 0 && (ldx % 2) == 0) ? 1 : 0;
    int tr = (r + 15) / 16;
    if (tr <= 1)
        launch_pg<1, 32>(c, alpha, X, ldx, k, C_dev, r, beta, Y, ldy, m, vec_ok);
    else if (tr <= 2)
        launch_pg<2, 32>(c, alpha, X, ldx, k, C_dev, r, beta, Y, ldy, m, vec_ok);
    else if (tr <= 4)
        launch_pg<4, 32>(c, alpha, X, ldx, k, C_dev, r, beta, Y, ldy, m, vec_ok);
    else if (tr <= 8)
        launch_pg<8, 32>(c, alpha, X, ldx, k, C_dev, r, beta, Y, ldy, m, vec_ok);
    else
        launch_pg<16, 16>(c, alpha, X, ldx, k, C_dev, r, beta, Y, ldy, m, vec_ok);
    RAILS_HIP_CHECK(hipGetLastError());
    return RAILS_OK;
}

// Y += alpha [X1 X2] C, C (a x r, ld a, a = a1 + a2) on the device; r <= 32
int rails_panel_gemm2_dev(rails_ctx *c, double alpha, const double *X1, int ldx1, int a1, const double *X2, int ldx2, int a2, const double *C_dev,
                          int r, double *Y, int ldy, int64_t m)
{
    if (r <= 0 || m <= 0) return RAILS_OK;
    const int a = a1 + a2;
    const int vec1 = ((((uintptr_t)X1) & 15) == 0 && (ldx1 % 2) == 0) ? 1 : 0;
    const int vec2 = ((((uintptr_t)X2) & 15) == 0 && (ldx2 % 2) == 0 && (a1 % 2) == 0) ? 1 : 0;
    const unsigned grid = (unsigned)((m + 63) / 64);
    if (r <= 16)
        RAILS_LAUNCH((k_panel_gemm2<1, 32>), dim3(grid), dim3(256), 0, c->stream, alpha, X1, ldx1, a1, X2, ldx2, a, C_dev, r, 1.0, Y, ldy, m, vec1, vec2);
    else
        RAILS_LAUNCH((k_panel_gemm2<2, 32>), dim3(grid), dim3(256), 0, c->stream, alpha, X1, ldx1, a1, X2, ldx2, a, C_dev, r, 1.0, Y, ldy, m, vec1, vec2);
    RAILS_HIP_CHECK(hipGetLastError());
    return RAILS_OK;
}

// ---- the plain wide GEMM of a basis rotation through rocBLAS -----------------------------------------------------------------------
// P2 = P Q with m = 1M rows, k and r in the hundreds, is a plain DGEMM, compute-bound: rocBLAS runs it at 44 TFLOP/s where
// k_panel_gemm<8, 32> (built around the bandwidth-bound narrow shapes) reaches 30 -- 3.9 instead of 5.8 ms per restart at k = 324,
// r = 268.  librocblas is resolved with dlopen (a library GEMM is what the platform's BLAS is for; everything else in this file is
// hand-written); creating the handle takes 0.3 s, so a solver that is going to rotate asks for it up front
// (rails_ctx_enable_library_gemm), not in the middle of a solve.  RAILS_WIDE_GEMM=own keeps the hand-written kernel.
namespace {
struct RocblasApi {
    void *handle = nullptr;
    int (*create)(void **) = nullptr;
    int (*destroy)(void *) = nullptr;
    int (*set_stream)(void *, hipStream_t) = nullptr;
    int (*dgemm)(void *, int, int, int, int, int, const double *, const double *, int, const double *, int, const double *, double *, int) = nullptr;
    bool tried = false, ok = false;
};
RocblasApi g_rocblas;
std::mutex g_rocblas_mutex;

bool load_rocblas()
{
    std::lock_guard<std::mutex> lock(g_rocblas_mutex);
    if (g_rocblas.tried) return g_rocblas.ok;
    g_rocblas.tried = true;
    // opt-in since round 3: the hand-written one-pass kernel (k_panel_gemm_wide) is the default
    const char *e = getenv("RAILS_WIDE_GEMM");
    if (!e || strcmp(e, "rocblas")) return false;
    const char *names[] = {getenv("RAILS_ROCBLAS_LIB"), "librocblas.so", "/opt/rocm/lib/librocblas.so", "librocblas.so.5", "librocblas.so.4"};
    for (const char *n : names) {
        if (!n || !*n) continue;
        if ((g_rocblas.handle = dlopen(n, RTLD_NOW | RTLD_LOCAL))) break;
    }
    if (!g_rocblas.handle) return false;
    g_rocblas.create = (int (*)(void **))dlsym(g_rocblas.handle, "rocblas_create_handle");
    g_rocblas.destroy = (int (*)(void *))dlsym(g_rocblas.handle, "rocblas_destroy_handle");
    g_rocblas.set_stream = (int (*)(void *, hipStream_t))dlsym(g_rocblas.handle, "rocblas_set_stream");
    g_rocblas.dgemm = (decltype(g_rocblas.dgemm))dlsym(g_rocblas.handle, "rocblas_dgemm");
    g_rocblas.ok = g_rocblas.create && g_rocblas.destroy && g_rocblas.set_stream && g_rocblas.dgemm;
    return g_rocblas.ok;
}
constexpr int ROCBLAS_OP_N = 111, ROCBLAS_OP_T = 112;
} // namespace

// One handle per process (for the device of the first context that asks).  rocblas_create_handle takes 0.3 s and is NOT done behind the
// caller's back on another thread (tried: a native program that starts using the GPU at once crashed now and then while rocBLAS was
// loading its code objects): whoever wants the library path asks for it at a convenient moment -- bench.py when it sets up.  The
// coordinate-space back end used to ask at the second restart a process saw; in a cold process that was a stall of seconds (the
// library and its kernels come from disk) for 2 ms saved per restart, so it no longer does.
namespace {
struct LibraryGemm {
    std::atomic<int> state{0}; // 0 not asked for, 2 ready, 3 not available
    int device = -1;
    void *handle = nullptr;
    std::mutex use; // creation; set_stream + dgemm of one caller at a time
};
LibraryGemm g_libgemm;
} // namespace

extern "C" int rails_ctx_enable_library_gemm(rails_ctx *c)
{
    RAILS_REQUIRE(c, "rails_ctx_enable_library_gemm: null context");
    std::lock_guard<std::mutex> lock(g_libgemm.use);
    if (g_libgemm.state.load() != 0) return RAILS_OK;
    g_libgemm.device = c->device;
    void *h = nullptr;
    if (!load_rocblas() || hipSetDevice(c->device) != hipSuccess || g_rocblas.create(&h) != 0 || !h) {
        g_libgemm.state = 3;
        return RAILS_OK; // without the library the hand-written kernel does the work
    }
    g_libgemm.handle = h;
    g_libgemm.state = 2;
    return RAILS_OK;
}

// 1 when rails_panel_gemm_wide on this context goes through the library from now on
extern "C" int rails_ctx_library_gemm_ready(const rails_ctx *c) { return c && g_libgemm.state.load() == 2 && g_libgemm.device == c->device ? 1 : 0; }

void rails_library_gemm_release(rails_ctx *) {}

// Y[:, yc0:yc0+r] = beta * Y + alpha * X[:, xc0:xc0+k] * C for any r: C goes to the device in ONE upload and the product is launched in
// slices of 128 output columns (the faster tile shape) without the host waiting in between -- rails_panel_gemm re-uses one staging
// buffer per call, so a loop over it makes the host wait for every slice's kernel but the last (the basis rotation P <- P Q of the
// coordinate-space back end: 2.6 ms of host time per restart).  X and Y must be different panels or disjoint windows.
extern "C" int rails_panel_gemm_wide(rails_ctx *c, double alpha, const rails_panel *X, int xc0, int k, const double *C_host, int ldc, int r,
                                     double beta, rails_panel *Y, int yc0)
{
    if (c) hipSetDevice(c->device); // allocations and launches go to the context's device whatever the caller's current device is
    rails_slow_guard slow__(c, "rails_panel_gemm_wide", k, r);
    RAILS_REQUIRE(c && X && Y, "rails_panel_gemm_wide: null argument");
    RAILS_REQUIRE(k >= 0 && r >= 0 && xc0 >= 0 && yc0 >= 0 && xc0 + k <= X->cap && yc0 + r <= Y->cap,
                  "rails_panel_gemm_wide: windows [%d,%d) / [%d,%d) outside capacities %d / %d", xc0, xc0 + k, yc0, yc0 + r, X->cap, Y->cap);
    RAILS_REQUIRE(X->m == Y->m, "rails_panel_gemm_wide: row mismatch %lld vs %lld", (long long)X->m, (long long)Y->m);
    RAILS_REQUIRE(k == 0 || r == 0 || (C_host && ldc >= k), "rails_panel_gemm_wide: bad coefficient matrix (ldc %d < %d)", ldc, k);
    if (X->d == Y->d) RAILS_REQUIRE((xc0 + k <= yc0) || (yc0 + r <= xc0), "rails_panel_gemm_wide: overlapping windows of one panel");
    if (r == 0 || X->m == 0) return RAILS_OK;
    if (k == 0) {
        if (beta == 0.0) return rails_panel_fill(c, Y, yc0, r, 0.0);
        if (beta == 1.0) return RAILS_OK;
        return rails_panel_scale(c, Y, yc0, r, beta);
    }
    size_t n = (size_t)k * r;
    RAILS_TRY(rails_small_reserve(c, n * sizeof(double)));
    RAILS_TRY(rails_pinned_begin_write(c, n * sizeof(double)));
    for (int j = 0; j < r; ++j) memcpy(c->pinned + (size_t)j * k, C_host + (size_t)j * ldc, sizeof(double) * k);
    RAILS_HIP_CHECK(hipMemcpyAsync(c->small, c->pinned, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    RAILS_TRY(rails_pinned_end_write(c));
    if (k >= 64 && r >= 64 && X->m < 0x7fffffffLL && rails_ctx_library_gemm_ready(c)) {
        // (opt-in, RAILS_WIDE_GEMM=rocblas + rails_ctx_enable_library_gemm) row-major panels are column-major matrices transposed:
        // Y' (r x m, ld) = alpha C' (r x k) X' (k x m, ld) + beta Y'
        const int m32 = (int)X->m;
        std::lock_guard<std::mutex> lock(g_libgemm.use);
        int rc = g_rocblas.set_stream(g_libgemm.handle, c->stream);
        if (rc == 0) rc = g_rocblas.dgemm(g_libgemm.handle, ROCBLAS_OP_T, ROCBLAS_OP_N, r, m32, k, &alpha, c->small, k, X->d + xc0, X->ld, &beta, Y->d + yc0, Y->ld);
        if (rc == 0) return RAILS_OK;
        rails_set_error("rails_panel_gemm_wide: rocblas_dgemm failed with status %d", rc);
        return RAILS_EHIP;
    }
    // slices of equal width, at most 288 columns (18 tiles of 16: what a wave's registers hold), X read once per slice
    static const int wide_env = getenv("RAILS_PANEL_GEMM_WIDE") ? atoi(getenv("RAILS_PANEL_GEMM_WIDE")) : 1;
    const int vec_ok = ((((uintptr_t)(X->d + xc0)) & 15) == 0 && (X->ld % 2) == 0) ? 1 : 0;
    if (wide_env && r > 64 && k >= 32) {
        const int nslices = (r + 287) / 288, width = ((r + nslices - 1) / nslices + 15) / 16 * 16;
        const size_t ct_doubles = (size_t)((k + 31) / 32 * 32) * (16 * 18 + 4);
        RAILS_TRY(rails_ws_reserve(c, (size_t)nslices * ct_doubles * sizeof(double)));
        int slice = 0;
        for (int j0 = 0; j0 < r; j0 += width, ++slice) {
            // tiles of 16 output columns per wave: an even count, or with the tile fit the exact count where that is 13, 15 or 17
            // (a rank of 257 to 272 after compress() is 17 tiles: as 18, one tile in eighteen of every k-step multiplied zeros)
            const int nc = std::min(width, r - j0), exact = (nc + 15) / 16;
            const int tr = (dense_tile_fit() && (exact == 13 || exact == 15 || exact == 17)) ? exact : (nc + 31) / 32 * 2;
            const double *Cj = c->small + (size_t)j0 * k;
            double *Yj = Y->d + yc0 + j0, *ct = c->ws + (size_t)slice * ct_doubles;
            switch (tr) {
            case 13: RAILS_TRY((launch_pg_wide<13>(c, alpha, X->d + xc0, X->ld, k, Cj, nc, beta, Yj, Y->ld, X->m, vec_ok, ct))); break;
            case 15: RAILS_TRY((launch_pg_wide<15>(c, alpha, X->d + xc0, X->ld, k, Cj, nc, beta, Yj, Y->ld, X->m, vec_ok, ct))); break;
            case 17: RAILS_TRY((launch_pg_wide<17>(c, alpha, X->d + xc0, X->ld, k, Cj, nc, beta, Yj, Y->ld, X->m, vec_ok, ct))); break;
            case 2: case 4: case 6: RAILS_TRY((launch_pg_wide<6>(c, alpha, X->d + xc0, X->ld, k, Cj, nc, beta, Yj, Y->ld, X->m, vec_ok, ct))); break;
            case 8: RAILS_TRY((launch_pg_wide<8>(c, alpha, X->d + xc0, X->ld, k, Cj, nc, beta, Yj, Y->ld, X->m, vec_ok, ct))); break;
            case 10: RAILS_TRY((launch_pg_wide<10>(c, alpha, X->d + xc0, X->ld, k, Cj, nc, beta, Yj, Y->ld, X->m, vec_ok, ct))); break;
            case 12: RAILS_TRY((launch_pg_wide<12>(c, alpha, X->d + xc0, X->ld, k, Cj, nc, beta, Yj, Y->ld, X->m, vec_ok, ct))); break;
            case 14: RAILS_TRY((launch_pg_wide<14>(c, alpha, X->d + xc0, X->ld, k, Cj, nc, beta, Yj, Y->ld, X->m, vec_ok, ct))); break;
            case 16: RAILS_TRY((launch_pg_wide<16>(c, alpha, X->d + xc0, X->ld, k, Cj, nc, beta, Yj, Y->ld, X->m, vec_ok, ct))); break;
            default: RAILS_TRY((launch_pg_wide<18>(c, alpha, X->d + xc0, X->ld, k, Cj, nc, beta, Yj, Y->ld, X->m, vec_ok, ct))); break;
            }
        }
        RAILS_HIP_CHECK(hipGetLastError());
        return RAILS_OK;
    }
    for (int j0 = 0; j0 < r; j0 += 128) {
        const int nc = std::min(128, r - j0);
        RAILS_TRY(rails_panel_gemm_dev(c, alpha, X->d + xc0, X->ld, k, c->small + (size_t)j0 * k, nc, beta, Y->d + yc0 + j0, Y->ld, X->m));
    }
    return RAILS_OK;
}

extern "C" int rails_panel_gemm(rails_ctx *c, double alpha, const rails_panel *X, int xc0, int k, const double *C_host, int ldc,
                                int r, double beta, rails_panel *Y, int yc0)
{
    if (c) hipSetDevice(c->device); // allocations and launches go to the context's device whatever the caller's current device is
    rails_slow_guard slow__(c, "rails_panel_gemm", k, r);
    RAILS_REQUIRE(c && X && Y, "rails_panel_gemm: null argument");
    RAILS_REQUIRE(k >= 0 && r >= 0 && xc0 >= 0 && yc0 >= 0 && xc0 + k <= X->cap && yc0 + r <= Y->cap,
                  "rails_panel_gemm: windows [%d,%d) / [%d,%d) outside capacities %d / %d", xc0, xc0 + k, yc0, yc0 + r, X->cap, Y->cap);
    RAILS_REQUIRE(X->m == Y->m, "rails_panel_gemm: row mismatch %lld vs %lld", (long long)X->m, (long long)Y->m);
    RAILS_REQUIRE(r <= 256, "rails_panel_gemm: r = %d > 256 output columns per call", r);
    RAILS_REQUIRE(k == 0 || r == 0 || (C_host && ldc >= k), "rails_panel_gemm: bad coefficient matrix (ldc %d < %d)", ldc, k);
    if (X->d == Y->d) {
        bool same = (xc0 == yc0);
        bool disjoint = (xc0 + k <= yc0) || (yc0 + r <= xc0);
        RAILS_REQUIRE(same || disjoint, "rails_panel_gemm: partially overlapping windows of one panel");
    }
    if (r == 0 || X->m == 0) return RAILS_OK;
    if (k == 0) {
        if (beta == 0.0) return rails_panel_fill(c, Y, yc0, r, 0.0);
        if (beta == 1.0) return RAILS_OK;
        return rails_panel_scale(c, Y, yc0, r, beta);
    }
    size_t n = (size_t)k * r;
    // asynchronous: the coefficient block goes through the pinned staging buffer (the next host write into it waits for this
    // upload, rails_pinned_begin_write) into the context's small device buffer (re-used in stream order)
    RAILS_TRY(rails_small_reserve(c, n * sizeof(double)));
    RAILS_TRY(rails_pinned_begin_write(c, n * sizeof(double)));
    for (int j = 0; j < r; ++j) memcpy(c->pinned + (size_t)j * k, C_host + (size_t)j * ldc, sizeof(double) * k);
    RAILS_HIP_CHECK(hipMemcpyAsync(c->small, c->pinned, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    RAILS_TRY(rails_pinned_end_write(c));
    return rails_panel_gemm_dev(c, alpha, X->d + xc0, X->ld, k, c->small, r, beta, Y->d + yc0, Y->ld, X->m);
}
