// dense_gram.hip -- Gram products of tall-skinny panels and column sums of squares (dense_common.h has what the dense files share):
//   rails_gram             C = X^T Y          (MultiVector::dot,  src/StlWrapper.cpp:394-412)
//   rails_panel_colnorms2  column sums of squares of a wide window
#include "dense_common.h"

namespace {

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

} // namespace

DenseSwitch g_dense_tile_fit{"RAILS_DENSE_TILE_FIT", 1};

extern "C" void rails_dense_set_tile_fit(int on) { g_dense_tile_fit.set(on); }

extern "C" int rails_dense_tile_fit(void) { return g_dense_tile_fit.get() ? 1 : 0; }

extern "C" int rails_dense_last_tiles(const rails_ctx *c, int *update_gram_nbw, int *gram_cols_ti, int *gemm_wide_tr)
{
    RAILS_REQUIRE(c, "rails_dense_last_tiles: null context");
    if (update_gram_nbw) *update_gram_nbw = c->last_update_gram_nbw;
    if (gram_cols_ti) *gram_cols_ti = c->last_gram_cols_ti;
    if (gemm_wide_tr) *gemm_wide_tr = c->last_gemm_wide_tr;
    return RAILS_OK;
}

int rails_reduce_partials(rails_ctx *c, const double *partial, int64_t nslab, int64_t n, double *out)
{
    RAILS_LAUNCH(k_reduce_partials, dim3((unsigned)((n + 63) / 64)), dim3(1024), 0, c->stream, partial, nslab, n, out);
    RAILS_HIP_CHECK(hipGetLastError());
    return RAILS_OK;
}

namespace {

// What the Gram rule reads beside the shape.  Only a wide-X shape reads anything, so each variable is read once per process at the
// first such call (RAILS_GRAM_EXTRA_COLUMN: the first with the wide-X form on); the two-segment operand reads neither.
dense::DenseSwitches gram_switches(int a, int b, bool two_segment)
{
    dense::DenseSwitches sw;
    if (!dense::gram_wide_shape(a, b)) return sw;
    if (!two_segment) {
        static const int cols_form = spmm_env("RAILS_GRAM_COLS", 1);
        sw.gram_cols = cols_form;
        if (cols_form) {
            static const int extra_env = spmm_env("RAILS_GRAM_EXTRA_COLUMN", 1);
            sw.gram_extra_column = extra_env;
        }
    }
    if (two_segment || sw.gram_cols) sw.tile_fit = g_dense_tile_fit.get();
    return sw;
}

} // namespace

int rails_gram_dev(rails_ctx *c, const double *X, int ldx, const double *Y, int ldy, int64_t m, int a, int b, double *C_dev)
{
    if (a <= 0 || b <= 0) return RAILS_OK;
    const dense::GramChoice g = dense::gram_choice(m, a, b, false, gram_switches(a, b, false));
    const size_t n = (size_t)a * b;
    RAILS_TRY(rails_ws_reserve(c, (size_t)g.nslab * n * sizeof(double)));
    const dim3 grid((unsigned)g.nslab, g.grid_y);
    if (g.form == dense::GramForm::WideX) {
        c->last_gram_cols_ti = g.ti;
        switch (g.key()) {
#define RAILS_CASE(TI, TJ, NE)                                                                                                             \
    case dense::inst(TI, TJ, NE):                                                                                                          \
        RAILS_LAUNCH((k_gram_cols<TI, TJ, NE>), grid, dim3(256), 0, c->stream, X, ldx, a, Y, ldy, b, m, g.rps, c->ws);                     \
        break;
            RAILS_DENSE_GRAM_COLS_TABLE(RAILS_CASE)
#undef RAILS_CASE
        default: RAILS_REQUIRE(false, "rails_gram: no k_gram_cols<%d, %d, %d>", g.ti, g.tj, g.ne);
        }
    } else {
        switch (g.key()) {
#define RAILS_CASE(TI, TJ)                                                                                                                 \
    case dense::inst(TI, TJ):                                                                                                              \
        RAILS_LAUNCH((k_gram<TI, TJ>), grid, dim3(256), 0, c->stream, X, ldx, a, Y, ldy, b, m, g.rps, g.ngj, c->ws);                       \
        break;
            RAILS_DENSE_GRAM_TABLE(RAILS_CASE)
#undef RAILS_CASE
        default: RAILS_REQUIRE(false, "rails_gram: no k_gram<%d, %d>", g.ti, g.tj);
        }
    }
    return rails_reduce_partials(c, c->ws, g.nslab, (int64_t)n, C_dev);
}

// the same for a left operand in two panels, [X1 X2]' Y with a = a1 + a2 columns (the deflated projection of orth.hip); b <= 32
int rails_gram2_dev(rails_ctx *c, const double *X1, int ldx1, int a1, const double *X2, int ldx2, int a2, const double *Y, int ldy, int64_t m, int b,
                    double *C_dev)
{
    const int a = a1 + a2;
    if (a <= 0 || b <= 0) return RAILS_OK;
    const dense::GramChoice g = dense::gram_choice(m, a, b, true, gram_switches(a, b, true));
    const size_t n = (size_t)a * b;
    RAILS_TRY(rails_ws_reserve(c, (size_t)g.nslab * n * sizeof(double)));
    const dim3 grid((unsigned)g.nslab, g.grid_y);
    if (g.form == dense::GramForm::WideX) {
        c->last_gram_cols_ti = g.ti;
        switch (g.key()) {
#define RAILS_CASE(TI, TJ, NE)                                                                                                             \
    case dense::inst(TI, TJ, NE):                                                                                                          \
        RAILS_LAUNCH((k_gram_cols2<TI, TJ, NE>), grid, dim3(256), 0, c->stream, X1, ldx1, a1, X2, ldx2, a, Y, ldy, b, m, g.rps, c->ws);    \
        break;
            RAILS_DENSE_GRAM_COLS_TABLE(RAILS_CASE)
#undef RAILS_CASE
        default: RAILS_REQUIRE(false, "rails_gram2: no k_gram_cols2<%d, %d, %d>", g.ti, g.tj, g.ne);
        }
    } else {
        switch (g.key()) {
#define RAILS_CASE(TI, TJ)                                                                                                                 \
    case dense::inst(TI, TJ):                                                                                                              \
        RAILS_LAUNCH((k_gram2<TI, TJ>), grid, dim3(256), 0, c->stream, X1, ldx1, a1, X2, ldx2, a, Y, ldy, b, m, g.rps, g.ngj, c->ws);      \
        break;
            RAILS_DENSE_GRAM2_TABLE(RAILS_CASE)
#undef RAILS_CASE
        default: RAILS_REQUIRE(false, "rails_gram2: no k_gram2<%d, %d>", g.ti, g.tj);
        }
    }
    return rails_reduce_partials(c, c->ws, g.nslab, (int64_t)n, C_dev);
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
    const int vec_ok = dense::rows_vec_ok(X, ldx) ? 1 : 0;
    RAILS_LAUNCH(k_colnorms2, dim3((unsigned)nslab), dim3(256), 0, c->stream, X, ldx, nc, m, rps, tx_bits, vec_ok, c->ws);
    return rails_reduce_partials(c, c->ws, nslab, (int64_t)nc, out_dev);
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
