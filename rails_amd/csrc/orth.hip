// orth.hip -- orthonormalisation of newly appended panel columns.
//
// Reference: StlWrapper::orthogonalize (src/StlWrapper.cpp:305-321): for every column past the
// watermark, normalise, twice subtract the projection on ALL previous columns, normalise -- four
// passes over the m x k panel per new column.
//
// Here (auto / block method): the w new columns W are treated as a block,
//     twice:  C = V_old^T W  (MFMA Gram, one all-reduce);  W -= V_old C  (MFMA panel GEMM)
//     twice:  G = W^T W;  G = R^T R (host Cholesky, w x w);  W <- W R^-1          (CholQR2)
// which is two Gram and two update passes for all w columns together.  Gram-Schmidt on the columns
// of W in order and the Cholesky factor of W^T W produce the same Q (QR with positive diagonal is
// unique), so the result equals the reference's up to rounding.  When the block Gram matrix is
// numerically rank deficient (Cholesky fails or its diagonal collapses) the routine falls back to
// the reference's column-wise recurrence, evaluated with the same device kernels.
//
// rails_orthogonalize_deflated does the same with a nullspace N (q orthonormal columns of another panel) projected out in every
// projection round: [N | V_old] is one left operand, so a round is one Gram pass over W, one all-reduce and one update pass
// (k_gram_cols_seg2 or k_gram_seg2, k_panel_gemm_seg2 below).  With q = 0 it is rails_orthogonalize.
#include "rails_internal.h"

#include <cmath>
#include <cstdlib>
#include <vector>

namespace {

typedef double v4f64 __attribute__((ext_vector_type(4)));
typedef double v2f64 __attribute__((ext_vector_type(2)));

// ---- two-segment kernels of the deflated projection -------------------------------------------------------------------------------
// The left operand X has a columns: [0, a1) are columns of X1 (the nullspace panel, leading dimension ldx1), [a1, a) columns of X2 (the old
// basis columns, ldx2).  Otherwise these are dense.hip's row-split Gram (k_gram) and panel GEMM (k_panel_gemm) with the same lane maps; they
// live here, in a translation unit of their own, so that the benchmarked kernels of dense.hip compile exactly as before.

// partial[slab] (a x b, col-major) = X[slab rows]' Y[slab rows]; grid.x = row slabs, grid.y = tile groups, 4 waves split the slab's rows
template <int TI, int TJ>
__global__ __launch_bounds__(256) void k_gram_seg2(const double *__restrict__ X1, int ldx1, int a1, const double *__restrict__ X2, int ldx2, int a,
                                                   const double *__restrict__ Y, int ldy, int b, int64_t m, int64_t rows_per_slab, int ngj,
                                                   double *__restrict__ partial)
{
    __shared__ double red[TI * TJ * 256];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int li = lane & 15, kk = lane >> 4;
    const int gi = blockIdx.y / ngj, gj = blockIdx.y % ngj;
    const int xcol0 = gi * TI * 16, ycol0 = gj * TJ * 16;
    const int64_t r_begin = (int64_t)blockIdx.x * rows_per_slab;
    int64_t r_end = r_begin + rows_per_slab;
    if (r_end > m) r_end = m;

    v4f64 acc[TI][TJ];
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j) acc[i][j] = (v4f64){0.0, 0.0, 0.0, 0.0};
    // columns outside the operand are clamped to column 0 (results never written); the segment is chosen per lane by address
    int xoff[TI], yoff[TJ];
    bool x2[TI];
#pragma unroll
    for (int i = 0; i < TI; ++i) {
        const int c = (xcol0 + 16 * i + li) < a ? xcol0 + 16 * i + li : 0;
        x2[i] = c >= a1;
        xoff[i] = x2[i] ? c - a1 : c;
    }
#pragma unroll
    for (int j = 0; j < TJ; ++j) yoff[j] = (ycol0 + 16 * j + li) < b ? ycol0 + 16 * j + li : 0;

    auto fetch = [&](int64_t r, double *xa, double *yb) {
        const int64_t row = r + kk;
        const bool rok = row < r_end;
        const int64_t rc = rok ? row : (r_end > 0 ? r_end - 1 : 0);
        const double *x1r = X1 + rc * ldx1, *x2r = X2 + rc * ldx2;
        const double *yr = Y + rc * ldy;
#pragma unroll
        for (int i = 0; i < TI; ++i) xa[i] = (x2[i] ? x2r : x1r)[xoff[i]];
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
            const double t = yr[yoff[j]];
            yb[j] = rok ? t : 0.0;
        }
    };
    double xa[TI], yb[TJ], xn[TI], yn[TJ];
    int64_t r = r_begin + 4 * wave;
    if (r < r_end) fetch(r, xa, yb);
    for (; r < r_end; r += 16) {
        const bool more = r + 16 < r_end;
        if (more) fetch(r + 16, xn, yn);
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int j = 0; j < TJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[i], yb[j], acc[i][j], 0, 0, 0);
        if (more) {
#pragma unroll
            for (int i = 0; i < TI; ++i) xa[i] = xn[i];
#pragma unroll
            for (int j = 0; j < TJ; ++j) yb[j] = yn[j];
        }
    }
    for (int w = 1; w < 4; ++w) { // cross-wave reduction in a fixed order
        if (wave == w) {
#pragma unroll
            for (int i = 0; i < TI; ++i)
#pragma unroll
                for (int j = 0; j < TJ; ++j)
#pragma unroll
                    for (int v = 0; v < 4; ++v) red[((i * TJ + j) * 4 + v) * 64 + lane] = acc[i][j][v];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int i = 0; i < TI; ++i)
#pragma unroll
                for (int j = 0; j < TJ; ++j)
#pragma unroll
                    for (int v = 0; v < 4; ++v) acc[i][j][v] += red[((i * TJ + j) * 4 + v) * 64 + lane];
        }
        __syncthreads();
    }
    if (wave == 0) {
        double *P = partial + (int64_t)blockIdx.x * a * b;
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int j = 0; j < TJ; ++j)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int ci = xcol0 + 16 * i + kk + 4 * v, cj = ycol0 + 16 * j + li;
                    if (ci < a && cj < b) P[ci + (int64_t)cj * a] = acc[i][j][v];
                }
    }
}

// Wide-X / narrow-Y form (a >= 128, b <= 32: the solver's [N V_old]'W), dense.hip's k_gram_cols with the two-segment X: the four waves of a
// block take four adjacent 16 TI-column strips of X for the same rows, so a block reads whole row segments; NE columns of Y past 16 TJ (b = 17)
// are done with plain multiply-adds.  Rows past the slab are clamped with the Y operand zeroed; columns past a are clamped to column 0.
template <int TI, int TJ, int NE>
__global__ __launch_bounds__(256) void k_gram_cols_seg2(const double *__restrict__ X1, int ldx1, int a1, const double *__restrict__ X2, int ldx2, int a,
                                                        const double *__restrict__ Y, int ldy, int b, int64_t m, int64_t rows_per_slab,
                                                        double *__restrict__ partial)
{
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int li = lane & 15, kk = lane >> 4;
    const int xcol0 = ((int)blockIdx.y * 4 + wave) * TI * 16;
    if (xcol0 >= a) return; // wave-uniform; no barrier below
    const int64_t r_begin = (int64_t)blockIdx.x * rows_per_slab;
    int64_t r_end = r_begin + rows_per_slab;
    if (r_end > m) r_end = m;
    constexpr int NEX = NE > 0 ? NE : 1;
    v4f64 acc[TI][TJ];
    double acce[TI][NEX];
#pragma unroll
    for (int i = 0; i < TI; ++i) {
#pragma unroll
        for (int j = 0; j < TJ; ++j) acc[i][j] = (v4f64){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int e = 0; e < NEX; ++e) acce[i][e] = 0.0;
    }
    int xoff[TI], yoff[TJ], eoff[NEX];
    bool x2[TI];
#pragma unroll
    for (int i = 0; i < TI; ++i) {
        const int c = (xcol0 + 16 * i + li) < a ? xcol0 + 16 * i + li : 0;
        x2[i] = c >= a1;
        xoff[i] = x2[i] ? c - a1 : c;
    }
#pragma unroll
    for (int j = 0; j < TJ; ++j) yoff[j] = (16 * j + li) < b ? 16 * j + li : 0;
#pragma unroll
    for (int e = 0; e < NEX; ++e) eoff[e] = 16 * TJ + e < b ? 16 * TJ + e : 0;

    auto fetch = [&](int64_t r, double *xa, double *yb, double *ye) {
        const int64_t row = r + kk;
        const bool rok = row < r_end;
        const int64_t rc = rok ? row : (r_end > 0 ? r_end - 1 : 0);
        const double *x1r = X1 + rc * ldx1, *x2r = X2 + rc * ldx2;
        const double *yr = Y + rc * ldy;
#pragma unroll
        for (int i = 0; i < TI; ++i) xa[i] = (x2[i] ? x2r : x1r)[xoff[i]];
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
            const double t = yr[yoff[j]];
            yb[j] = rok ? t : 0.0;
        }
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const double t = yr[eoff[e]];
            ye[e] = rok ? t : 0.0;
        }
    };
    auto work = [&](const double *xa, const double *yb, const double *ye) {
#pragma unroll
        for (int i = 0; i < TI; ++i) {
#pragma unroll
            for (int j = 0; j < TJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[i], yb[j], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int e = 0; e < NE; ++e) acce[i][e] += xa[i] * ye[e];
        }
    };
    double xa[TI], ya[TJ], xb[TI], yb[TJ], ea[NEX], eb[NEX];
    fetch(r_begin, xa, ya, ea);
    fetch(r_begin + 4, xb, yb, eb);
    for (int64_t r = r_begin; r < r_end; r += 8) {
        work(xa, ya, ea);
        fetch(r + 8, xa, ya, ea);
        work(xb, yb, eb);
        fetch(r + 12, xb, yb, eb);
    }
    double *P = partial + (int64_t)blockIdx.x * a * b;
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int ci = xcol0 + 16 * i + kk + 4 * v, cj = 16 * j + li;
                if (ci < a && cj < b) P[ci + (int64_t)cj * a] = acc[i][j][v];
            }
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const double t0 = acce[i][e];
            const double t1 = __shfl(t0, li + 16, 64), t2 = __shfl(t0, li + 32, 64), t3 = __shfl(t0, li + 48, 64);
            const int ci = xcol0 + 16 * i + li;
            if (kk == 0 && ci < a && 16 * TJ + e < b) P[ci + (int64_t)(16 * TJ + e) * a] = ((t0 + t1) + t2) + t3;
        }
}

// out[e] = sum_t partial[t][e] in a fixed order (dense.hip's k_reduce_partials)
__global__ __launch_bounds__(1024) void k_reduce_partials_seg2(const double *__restrict__ partial, int64_t nslab, int64_t n, double *__restrict__ out)
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

// Y (m x r) = beta Y + alpha X C, C (a x r, col-major, ld a) on the device; each wave owns 16 rows and all r <= 16 TR columns, C streams
// through LDS in chunks of KC rows.  X is read 4 consecutive columns per lane (vector loads where the 4 lie in one segment that allows them).
template <int TR, int KC>
__global__ __launch_bounds__(256) void k_panel_gemm_seg2(double alpha, const double *X1, int ldx1, int a1, const double *X2, int ldx2, int a,
                                                         const double *__restrict__ C, int r, double beta, double *Yp, int ldy, int64_t m, int vec1,
                                                         int vec2)
{
    constexpr int RL = 16 * TR + 4;
    __shared__ double Cs[KC * RL];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int li = lane & 15, kk = lane >> 4;
    const int64_t r0 = ((int64_t)blockIdx.x * 4 + wave) * 16;
    const int64_t myrow = r0 + li;
    const bool rowok = myrow < m;
    const int64_t srow = rowok ? myrow : 0; // (rows past m read row 0 and are never written)

    v4f64 acc[TR];
#pragma unroll
    for (int t = 0; t < TR; ++t) acc[t] = (v4f64){0.0, 0.0, 0.0, 0.0};

    const double *x1row = X1 + srow * ldx1, *x2row = X2 + srow * ldx2;
    for (int kc = 0; kc < a; kc += KC) {
        __syncthreads();
        for (int idx = threadIdx.x; idx < KC * 16 * TR; idx += 256) {
            const int kl = idx % KC, j = idx / KC;
            double v = 0.0;
            if (kc + kl < a && j < r) v = C[(kc + kl) + (int64_t)j * a];
            Cs[kl * RL + j] = v;
        }
        __syncthreads();
#pragma unroll
        for (int kb = 0; kb < KC; kb += 16) {
            const int kcol = kc + kb + 4 * kk;
            double xs[4];
            const bool in1 = kcol + 4 <= a1, in2 = kcol >= a1 && kcol + 4 <= a;
            if ((in1 && vec1) || (in2 && vec2)) {
                const double *src = in1 ? x1row + kcol : x2row + (kcol - a1);
                const v2f64 t0 = *reinterpret_cast<const v2f64 *>(src);
                const v2f64 t1 = *reinterpret_cast<const v2f64 *>(src + 2);
                xs[0] = t0.x;
                xs[1] = t0.y;
                xs[2] = t1.x;
                xs[3] = t1.y;
            } else {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int col = kcol + s;
                    xs[s] = col < a ? (col < a1 ? x1row[col] : x2row[col - a1]) : 0.0;
                }
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const double *crow = &Cs[(kb + 4 * kk + s) * RL + li];
#pragma unroll
                for (int t = 0; t < TR; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(xs[s], crow[16 * t], acc[t], 0, 0, 0);
            }
        }
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

// C_dev (a x b, ld a, a = a1 + a2) = [X1 X2]' Y, before the all-reduce; b <= 32
int gram_seg2_dev(rails_ctx *c, const double *X1, int ldx1, int a1, const double *X2, int ldx2, int a2, const double *Y, int ldy, int64_t m, int b,
                  double *C_dev)
{
    const int a = a1 + a2;
    if (a <= 0 || b <= 0) return RAILS_OK;
    // slab count as in rails_gram_dev: enough blocks to fill the chip, partial-tile traffic bounded to ~4% of the input
    double bound = 0.02 * (double)m * (double)(a + b) / ((double)a * (double)b);
    int64_t nslab = (int64_t)std::min<double>(1024.0, std::max<double>(1.0, bound));
    int64_t maxslab = (m + 15) / 16;
    if (nslab > maxslab) nslab = std::max<int64_t>(1, maxslab);
    int64_t rps = (m + nslab - 1) / nslab;
    rps = (rps + 15) / 16 * 16;
    if (rps < 16) rps = 16;
    nslab = std::max<int64_t>(1, (m + rps - 1) / rps);
    const size_t n = (size_t)a * b;
    RAILS_TRY(rails_ws_reserve(c, (size_t)nslab * n * sizeof(double)));
#define RAILS_GRAM_SEG2(TI, TJ)                                                                                                              \
    do {                                                                                                                                     \
        const int ngi = (a + 16 * TI - 1) / (16 * TI), ngj = (b + 16 * TJ - 1) / (16 * TJ);                                                 \
        RAILS_LAUNCH((k_gram_seg2<TI, TJ>), dim3((unsigned)nslab, (unsigned)(ngi * ngj)), dim3(256), 0, c->stream, X1, ldx1, a1, X2, ldx2, a, Y, \
                     ldy, b, m, rps, ngj, c->ws);                                                                                            \
    } while (0)
    if (a >= 128 && b <= 32) { // the wide-X form, with the tile choice of rails_gram_dev
        const int ntiles = (a + 15) / 16;
        const bool extra = b == 17;
        const int cand2[3] = {3, 4, 5}, cand1[3] = {4, 6, 8};
        const int *cand = (b <= 16 || extra) ? cand1 : cand2;
        int best = cand[1], best_cost = 1 << 30;
        for (int t = 0; t < 3; ++t) {
            const int ti = cand[t], strips = (ntiles + ti - 1) / ti, cost = (strips + 3) / 4 * 4 * ti;
            if (cost < best_cost) best = ti, best_cost = cost;
        }
        const dim3 grid((unsigned)nslab, (unsigned)(((ntiles + best - 1) / best + 3) / 4));
#define RAILS_GRAM_COLS_SEG2(TI, TJ, NE)                                                                                                     \
    RAILS_LAUNCH((k_gram_cols_seg2<TI, TJ, NE>), grid, dim3(256), 0, c->stream, X1, ldx1, a1, X2, ldx2, a, Y, ldy, b, m, rps, c->ws)
        if (extra) {
            if (best == 4)
                RAILS_GRAM_COLS_SEG2(4, 1, 1);
            else if (best == 6)
                RAILS_GRAM_COLS_SEG2(6, 1, 1);
            else
                RAILS_GRAM_COLS_SEG2(8, 1, 1);
        } else if (b <= 16) {
            if (best == 4)
                RAILS_GRAM_COLS_SEG2(4, 1, 0);
            else if (best == 6)
                RAILS_GRAM_COLS_SEG2(6, 1, 0);
            else
                RAILS_GRAM_COLS_SEG2(8, 1, 0);
        } else if (best == 3)
            RAILS_GRAM_COLS_SEG2(3, 2, 0);
        else if (best == 4)
            RAILS_GRAM_COLS_SEG2(4, 2, 0);
        else
            RAILS_GRAM_COLS_SEG2(5, 2, 0);
#undef RAILS_GRAM_COLS_SEG2
    } else if (a <= 16 && b <= 16)
        RAILS_GRAM_SEG2(1, 1);
    else if (b <= 16)
        RAILS_GRAM_SEG2(8, 1);
    else
        RAILS_GRAM_SEG2(4, 2);
#undef RAILS_GRAM_SEG2
    RAILS_LAUNCH(k_reduce_partials_seg2, dim3((unsigned)((n + 63) / 64)), dim3(1024), 0, c->stream, c->ws, nslab, (int64_t)n, C_dev);
    RAILS_HIP_CHECK(hipGetLastError());
    return RAILS_OK;
}

// Y += alpha [X1 X2] C, C (a x r, ld a) on the device; r <= 32
int panel_gemm_seg2_dev(rails_ctx *c, double alpha, const double *X1, int ldx1, int a1, const double *X2, int ldx2, int a2, const double *C_dev, int r,
                        double *Y, int ldy, int64_t m)
{
    if (r <= 0 || m <= 0) return RAILS_OK;
    const int a = a1 + a2;
    const int vec1 = ((((uintptr_t)X1) & 15) == 0 && (ldx1 % 2) == 0) ? 1 : 0;
    const int vec2 = ((((uintptr_t)X2) & 15) == 0 && (ldx2 % 2) == 0 && (a1 % 2) == 0) ? 1 : 0;
    const unsigned grid = (unsigned)((m + 63) / 64);
    if (r <= 16)
        RAILS_LAUNCH((k_panel_gemm_seg2<1, 32>), dim3(grid), dim3(256), 0, c->stream, alpha, X1, ldx1, a1, X2, ldx2, a, C_dev, r, 1.0, Y, ldy, m, vec1, vec2);
    else
        RAILS_LAUNCH((k_panel_gemm_seg2<2, 32>), dim3(grid), dim3(256), 0, c->stream, alpha, X1, ldx1, a1, X2, ldx2, a, C_dev, r, 1.0, Y, ldy, m, vec1, vec2);
    RAILS_HIP_CHECK(hipGetLastError());
    return RAILS_OK;
}

int sync_small_to_host(rails_ctx *c, size_t n, std::vector<double> &out)
{
    RAILS_TRY(rails_pinned_reserve(c, n * sizeof(double)));
    RAILS_HIP_CHECK(hipMemcpyAsync(c->pinned, c->small, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    RAILS_HIP_CHECK(rails_stream_sync(c));
    out.assign(c->pinned, c->pinned + n);
    return RAILS_OK;
}

int upload_small(rails_ctx *c, const std::vector<double> &in, double *dst)
{
    RAILS_TRY(rails_pinned_begin_write(c, in.size() * sizeof(double)));
    memcpy(c->pinned, in.data(), in.size() * sizeof(double));
    RAILS_HIP_CHECK(hipMemcpyAsync(dst, c->pinned, in.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    RAILS_HIP_CHECK(rails_stream_sync(c));
    return RAILS_OK;
}

// 2-norm of one column = sqrt(|v^T v|) (StlWrapper::norm on a single column, src/StlWrapper.cpp:280-288)
int column_norm(rails_ctx *c, const rails_panel *V, int col, double *nrm)
{
    RAILS_TRY(rails_small_reserve(c, sizeof(double)));
    RAILS_TRY(rails_gram_dev(c, V->d + col, V->ld, V->d + col, V->ld, V->m, 1, 1, c->small));
    RAILS_TRY(rails_allreduce_dev(c, c->small, 1));
    std::vector<double> h;
    RAILS_TRY(sync_small_to_host(c, 1, h));
    *nrm = std::sqrt(std::fabs(h[0]));
    return RAILS_OK;
}

// one pass "v -= P (P^T v)" of column i against the columns [c0, c1) of V
int project_column(rails_ctx *c, rails_panel *V, int i, int c0, int c1)
{
    const int n = c1 - c0;
    if (n <= 0) return RAILS_OK;
    RAILS_TRY(rails_small_reserve(c, (size_t)n * sizeof(double)));
    RAILS_TRY(rails_gram_dev(c, V->d + c0, V->ld, V->d + i, V->ld, V->m, n, 1, c->small));
    RAILS_TRY(rails_allreduce_dev(c, c->small, (size_t)n));
    return rails_panel_gemm_dev(c, -1.0, V->d + c0, V->ld, n, c->small, 1, 1.0, V->d + i, V->ld, V->m);
}

// The nullspace of rails_orthogonalize_deflated: columns [c0, c0 + q) of panel N (q = 0: none)
struct Nullspace {
    const rails_panel *N = nullptr;
    int c0 = 0, q = 0;
};

// W (w columns from column k_old of V) -= [N V_old] ([N V_old]' W): one Gram pass over W, one all-reduce, one update pass.  Above 32 columns
// of N or of W the two-segment kernels are not instantiated: two Gram and two update calls, still one all-reduce.
int project_block(rails_ctx *c, rails_panel *V, int k_old, int w, Nullspace const &ns)
{
    const int q = ns.q, a = q + k_old;
    const double *Nd = ns.N->d + ns.c0;
    double *W = V->d + k_old;
    RAILS_TRY(rails_small_reserve(c, (size_t)a * w * sizeof(double)));
    if (q <= 32 && w <= 32) {
        RAILS_TRY(gram_seg2_dev(c, Nd, ns.N->ld, q, V->d, V->ld, k_old, W, V->ld, V->m, w, c->small));
        RAILS_TRY(rails_allreduce_dev(c, c->small, (size_t)a * w));
        return panel_gemm_seg2_dev(c, -1.0, Nd, ns.N->ld, q, V->d, V->ld, k_old, c->small, w, W, V->ld, V->m);
    }
    double *D = c->small, *Cv = c->small + (size_t)q * w; // N'W (q x w), V_old'W (k_old x w)
    RAILS_TRY(rails_gram_dev(c, Nd, ns.N->ld, W, V->ld, V->m, q, w, D));
    if (k_old > 0) RAILS_TRY(rails_gram_dev(c, V->d, V->ld, W, V->ld, V->m, k_old, w, Cv));
    RAILS_TRY(rails_allreduce_dev(c, c->small, (size_t)a * w));
    for (int j0 = 0; j0 < w; j0 += 256) { // panel GEMM handles <= 256 output columns per launch
        const int wc = w - j0 < 256 ? w - j0 : 256;
        RAILS_TRY(rails_panel_gemm_dev(c, -1.0, Nd, ns.N->ld, q, D + (size_t)j0 * q, wc, 1.0, W + j0, V->ld, V->m));
        if (k_old > 0) RAILS_TRY(rails_panel_gemm_dev(c, -1.0, V->d, V->ld, k_old, Cv + (size_t)j0 * k_old, wc, 1.0, W + j0, V->ld, V->m));
    }
    return RAILS_OK;
}

// one pass of column i against N and the columns [0, i) of V, in the same way
int project_column(rails_ctx *c, rails_panel *V, int i, Nullspace const &ns)
{
    if (ns.q == 0) return project_column(c, V, i, 0, i);
    const int q = ns.q, a = q + i;
    const double *Nd = ns.N->d + ns.c0;
    RAILS_TRY(rails_small_reserve(c, (size_t)a * sizeof(double)));
    RAILS_TRY(gram_seg2_dev(c, Nd, ns.N->ld, q, V->d, V->ld, i, V->d + i, V->ld, V->m, 1, c->small));
    RAILS_TRY(rails_allreduce_dev(c, c->small, (size_t)a));
    return panel_gemm_seg2_dev(c, -1.0, Nd, ns.N->ld, q, V->d, V->ld, i, c->small, 1, V->d + i, V->ld, V->m);
}

// The reference's recurrence (src/StlWrapper.cpp:308-319) for columns [from, to): normalise, twice subtract the
// projection on ALL previous columns (and on the nullspace), normalise.
int columnwise(rails_ctx *c, rails_panel *V, int from, int to, Nullspace const &ns = Nullspace())
{
    for (int i = from; i < to; ++i) {
        double nrm = 0.0;
        RAILS_TRY(column_norm(c, V, i, &nrm));
        RAILS_TRY(rails_panel_scale(c, V, i, 1, 1.0 / nrm));
        for (int pass = 0; pass < 2; ++pass) RAILS_TRY(project_column(c, V, i, ns));
        RAILS_TRY(column_norm(c, V, i, &nrm));
        RAILS_TRY(rails_panel_scale(c, V, i, 1, 1.0 / nrm));
    }
    return RAILS_OK;
}

// Fallback after the block projection against the old columns has already been applied to all new columns: Gram-Schmidt column by
// column, each column twice against ALL columns before it -- the old ones included.  (Until round 3 the two passes ran inside the
// block only, m x w traffic, and a column got the full treatment only when it lost more than five digits there.  A column that keeps a
// fraction f of its length inherits the defects of the block's earlier columns against the old ones magnified by 1 / f, and a chain of
// nearly dependent columns compounds that: the coordinate-space back end's copy of this shortcut cost it eight digits of V'AV on
// BASELINE configs[1], DESIGN.md section 5 (vi).  This path is rare -- the repair round takes the rank-deficient blocks -- so it pays the
// reference's price: src/StlWrapper.cpp:308-319.)
int columnwise_in_block(rails_ctx *c, rails_panel *V, int k_old, int w, Nullspace const &ns = Nullspace())
{
    for (int i = k_old; i < k_old + w; ++i) {
        double n0 = 0.0, n1 = 0.0;
        RAILS_TRY(column_norm(c, V, i, &n0));
        if (n0 > 0.0) RAILS_TRY(rails_panel_scale(c, V, i, 1, 1.0 / n0));
        for (int pass = 0; pass < 2; ++pass) RAILS_TRY(project_column(c, V, i, ns));
        RAILS_TRY(column_norm(c, V, i, &n1));
        if (!(n1 > 0.0) || !std::isfinite(n1)) {
            // nothing at all survived: the column was a bitwise copy of the one before it once that one had been orthogonalised (two
            // dependent columns that the repair round left identical).  The reference would divide by zero here; like the coordinate-space
            // back end's orthogonalize(), take a random direction instead and orthogonalise that.
            RAILS_TRY(rails_panel_random(c, V, i, 1));
            RAILS_TRY(column_norm(c, V, i, &n1));
            RAILS_TRY(rails_panel_scale(c, V, i, 1, 1.0 / n1));
            for (int pass = 0; pass < 2; ++pass) RAILS_TRY(project_column(c, V, i, ns));
            RAILS_TRY(column_norm(c, V, i, &n1));
        }
        if (!(n1 > 1e-5)) { // the column was normalised before the projection: n1 is the fraction that survived -- once more, from unit length
            RAILS_TRY(rails_panel_scale(c, V, i, 1, 1.0 / n1));
            for (int pass = 0; pass < 2; ++pass) RAILS_TRY(project_column(c, V, i, ns));
            RAILS_TRY(column_norm(c, V, i, &n1));
        }
        RAILS_TRY(rails_panel_scale(c, V, i, 1, 1.0 / n1));
    }
    return RAILS_OK;
}

// Repair step of the block method for a numerically rank-deficient block (typical in RAILS: the Ritz values of the
// residual operator come in +/- pairs whose vectors coincide once span(V) is projected out, so about every second
// expansion vector is dependent on its predecessors).  The reference's recurrence turns such a column into the
// normalised rounding noise of its projection and carries on.  Here: Cholesky of the block Gram matrix G with the
// dependent pivots skipped (r_ii = 1, row i of R zero): W <- W R^-1 orthonormalises the independent columns among
// themselves and leaves every dependent column as its (tiny) residual against the independent columns before it; those
// residuals are scaled to unit norm and the block procedure is run once more on the repaired block, which is then
// generically of full rank.  All block operations: no per-column passes over the m x k panel.
int repair_block(rails_ctx *c, rails_panel *V, int k_old, int w, const std::vector<double> &G, int *n_bad)
{
    std::vector<double> R((size_t)w * w, 0.0);
    std::vector<char> bad(w, 0);
    *n_bad = 0;
    for (int i = 0; i < w; ++i) {
        double piv = G[i + (size_t)i * w];
        for (int j = 0; j < i; ++j) {
            if (bad[j]) continue; // row j of R is zero beyond its diagonal
            double s = G[j + (size_t)i * w];
            for (int l = 0; l < j; ++l)
                if (!bad[l]) s -= R[l + (size_t)j * w] * R[l + (size_t)i * w];
            s /= R[j + (size_t)j * w];
            R[j + (size_t)i * w] = s;
            piv -= s * s;
        }
        if (piv > 1e-10 * G[i + (size_t)i * w] && G[i + (size_t)i * w] > 0.0)
            R[i + (size_t)i * w] = std::sqrt(piv);
        else {
            bad[i] = 1;
            R[i + (size_t)i * w] = 1.0;
            (*n_bad)++;
        }
    }
    std::vector<double> Rinv((size_t)w * w, 0.0);
    for (int j = 0; j < w; ++j) {
        Rinv[j + (size_t)j * w] = 1.0 / R[j + (size_t)j * w];
        for (int i = j - 1; i >= 0; --i) {
            double s = 0.0;
            for (int l = i + 1; l <= j; ++l) s += R[i + (size_t)l * w] * Rinv[l + (size_t)j * w];
            Rinv[i + (size_t)j * w] = -s / R[i + (size_t)i * w];
        }
    }
    double *W = V->d + k_old;
    RAILS_TRY(rails_small_reserve(c, (size_t)w * w * sizeof(double)));
    RAILS_TRY(upload_small(c, Rinv, c->small));
    RAILS_TRY(rails_panel_gemm_dev(c, 1.0, W, V->ld, w, c->small, w, 0.0, W, V->ld, V->m));
    // norms of the residual columns (one block Gram), then scale them to unit length
    RAILS_TRY(rails_gram_dev(c, W, V->ld, W, V->ld, V->m, w, w, c->small));
    RAILS_TRY(rails_allreduce_dev(c, c->small, (size_t)w * w));
    std::vector<double> G2;
    RAILS_TRY(sync_small_to_host(c, (size_t)w * w, G2));
    for (int i = 0; i < w; ++i) {
        if (!bad[i]) continue;
        double n2 = G2[i + (size_t)i * w];
        if (n2 > 0.0 && std::isfinite(n2)) RAILS_TRY(rails_panel_scale(c, V, k_old + i, 1, 1.0 / std::sqrt(n2)));
    }
    return RAILS_OK;
}

// rails_orthogonalize (ns.q = 0) and rails_orthogonalize_deflated
int orthogonalize(rails_ctx *c, rails_panel *V, int k_old, int w, Nullspace const &ns, int method, int *used)
{
    if (used) *used = 0;
    if (w == 0) return RAILS_OK;
    if (method == 1 || w > 256) {
        if (used) *used = 1;
        c->n_orth_columnwise++;
        return columnwise(c, V, k_old, k_old + w, ns);
    }
    double *W = V->d + k_old;
    for (int round = 0; round < 2; ++round) {
    bool repaired = false;
    // block CGS2 against the nullspace and the old columns
    if (ns.q > 0) {
        for (int pass = 0; pass < 2; ++pass) RAILS_TRY(project_block(c, V, k_old, w, ns));
    } else if (k_old > 0) {
        RAILS_TRY(rails_small_reserve(c, (size_t)k_old * w * sizeof(double)));
        for (int pass = 0; pass < 2; ++pass) {
            RAILS_TRY(rails_gram_dev(c, V->d, V->ld, W, V->ld, V->m, k_old, w, c->small));
            RAILS_TRY(rails_allreduce_dev(c, c->small, (size_t)k_old * w));
            for (int j0 = 0; j0 < w; j0 += 256) { // panel GEMM handles <= 256 output columns per launch
                int wc = w - j0 < 256 ? w - j0 : 256;
                RAILS_TRY(rails_panel_gemm_dev(c, -1.0, V->d, V->ld, k_old, c->small + (size_t)j0 * k_old, wc, 1.0, W + j0, V->ld, V->m));
            }
        }
    }
    // CholQR2 inside the block
    RAILS_TRY(rails_small_reserve(c, (size_t)w * w * sizeof(double)));
    for (int pass = 0; pass < 2; ++pass) {
        RAILS_TRY(rails_gram_dev(c, W, V->ld, W, V->ld, V->m, w, w, c->small));
        RAILS_TRY(rails_allreduce_dev(c, c->small, (size_t)w * w));
        std::vector<double> G;
        RAILS_TRY(sync_small_to_host(c, (size_t)w * w, G));
        double dmax = 0.0;
        for (int i = 0; i < w; ++i) dmax = std::max(dmax, G[i + (size_t)i * w]);
        std::vector<double> R = G;
        int info = 0;
        rails_dpotrf('U', w, R.data(), w, &info);
        bool bad = (info != 0) || !(dmax > 0.0);
        if (!bad) {
            // a diagonal of R much smaller than the column norm means the column lies (numerically)
            // in the span of the others: CholQR would amplify rounding by (norm/r_ii)^2
            for (int i = 0; i < w; ++i) {
                double rii = R[i + (size_t)i * w];
                double nrm = std::sqrt(G[i + (size_t)i * w]);
                if (!(rii > 1e-5 * nrm)) bad = true;
            }
        }
        if (bad) {
            static const int repair_env = [] {
                const char *e = getenv("RAILS_ORTH_REPAIR");
                return e ? atoi(e) : 1;
            }();
            if (round == 0 && repair_env && dmax > 0.0) {
                int n_bad = 0;
                RAILS_TRY(repair_block(c, V, k_old, w, G, &n_bad));
                if (n_bad > 0) {
                    c->n_orth_repair++;
                    repaired = true;
                    break; // run the block procedure once more on the repaired block
                }
            }
            if (method == 2) {
                rails_set_error("rails_orthogonalize: block Gram matrix is rank deficient (dpotrf info %d)", info);
                return RAILS_ELAPACK;
            }
            if (used) *used = 1;
            c->n_orth_columnwise++;
            return columnwise_in_block(c, V, k_old, w, ns);
        }
        // Rinv (upper triangular): solve R * Rinv = I column by column
        std::vector<double> Rinv((size_t)w * w, 0.0);
        for (int j = 0; j < w; ++j) {
            Rinv[j + (size_t)j * w] = 1.0 / R[j + (size_t)j * w];
            for (int i = j - 1; i >= 0; --i) {
                double s = 0.0;
                for (int l = i + 1; l <= j; ++l) s += R[i + (size_t)l * w] * Rinv[l + (size_t)j * w];
                Rinv[i + (size_t)j * w] = -s / R[i + (size_t)i * w];
            }
        }
        RAILS_TRY(upload_small(c, Rinv, c->small));
        RAILS_TRY(rails_panel_gemm_dev(c, 1.0, W, V->ld, w, c->small, w, 0.0, W, V->ld, V->m)); // in place, row-local
    }
    if (!repaired) {
        if (used) *used = round == 0 ? 2 : 3;
        c->n_orth_block++;
        return RAILS_OK;
    }
    }
    if (used) *used = 1; // not reached: the second round either succeeds or takes the column-wise path
    return columnwise_in_block(c, V, k_old, w, ns);
}

} // namespace

extern "C" int rails_orthogonalize(rails_ctx *c, rails_panel *V, int k_old, int w, int method, int *used)
{
    if (c) hipSetDevice(c->device); // allocations and launches go to the context's device whatever the caller's current device is
    RAILS_REQUIRE(c && V, "rails_orthogonalize: null argument");
    RAILS_REQUIRE(k_old >= 0 && w >= 0 && k_old + w <= V->cap, "rails_orthogonalize: columns [%d,%d) outside capacity %d", k_old,
                  k_old + w, V->cap);
    RAILS_REQUIRE(method >= 0 && method <= 2, "rails_orthogonalize: bad method %d", method);
    return orthogonalize(c, V, k_old, w, Nullspace(), method, used);
}

extern "C" int rails_orthogonalize_deflated(rails_ctx *c, rails_panel *V, int k_old, int w, const rails_panel *N, int nc0, int q, int method,
                                            int *used)
{
    if (c) hipSetDevice(c->device);
    RAILS_REQUIRE(c && V && (q == 0 || N), "rails_orthogonalize_deflated: null argument");
    RAILS_REQUIRE(k_old >= 0 && w >= 0 && k_old + w <= V->cap, "rails_orthogonalize_deflated: columns [%d,%d) outside capacity %d", k_old,
                  k_old + w, V->cap);
    RAILS_REQUIRE(q >= 0 && (q == 0 || (nc0 >= 0 && nc0 + q <= N->cap)), "rails_orthogonalize_deflated: nullspace columns [%d,%d) outside capacity %d",
                  nc0, nc0 + q, q ? N->cap : 0);
    RAILS_REQUIRE(q == 0 || N->m == V->m, "rails_orthogonalize_deflated: the nullspace has %lld rows, V %lld", q ? (long long)N->m : 0LL,
                  (long long)V->m);
    RAILS_REQUIRE(q == 0 || N != V, "rails_orthogonalize_deflated: the nullspace must be a panel of its own");
    RAILS_REQUIRE(method >= 0 && method <= 2, "rails_orthogonalize_deflated: bad method %d", method);
    Nullspace ns;
    ns.N = N;
    ns.c0 = nc0;
    ns.q = q;
    return orthogonalize(c, V, k_old, w, ns, method, used);
}
