// dense_gemm.hip -- products of a tall-skinny panel with a small matrix (dense_common.h has what the dense files share):
//   rails_panel_gemm       Y = beta Y + alpha X C   (MultiVector * DenseMatrix, src/StlWrapper.cpp:168-187)
//   rails_panel_gemm_wide  the same for any number of output columns: the restart rotation, in one pass or through rocBLAS
#include "dense_common.h"

#include <dlfcn.h>
#include <mutex>

namespace {

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
int launch_pg_wide(rails_ctx *c, double alpha, const double *X, int ldx, int k, const double *C, int r, double beta, double *Y, int ldy, int64_t m, int vec_ok, int skip_tail,
                   double *ct)
{
    constexpr int RL = 16 * TR + 4;
    const int kpad = (k + 31) / 32 * 32;
    RAILS_LAUNCH(k_pack_ct, dim3((unsigned)std::min<int64_t>(512, ((int64_t)kpad * RL + 255) / 256)), dim3(256), 0, c->stream, C, k, r, kpad, RL, ct);
    const size_t lds = (size_t)2 * 32 * RL * sizeof(double);
    RAILS_HIP_CHECK(hipFuncSetAttribute((const void *)k_panel_gemm_wide<TR>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    RAILS_LAUNCH((k_panel_gemm_wide<TR>), dim3((unsigned)((m + 127) / 128)), dim3(512), lds, c->stream, alpha, X, ldx, k, ct, r, beta, Y, ldy, m, vec_ok,
                 skip_tail);
    c->last_gemm_wide_tr = TR;
    return RAILS_OK;
}

// the product without X (k = 0): Y = beta Y
int scale_only(rails_ctx *c, rails_panel *Y, int yc0, int r, double beta)
{
    if (beta == 0.0) return rails_panel_fill(c, Y, yc0, r, 0.0);
    if (beta == 1.0) return RAILS_OK;
    return rails_panel_scale(c, Y, yc0, r, beta);
}

} // namespace

int rails_panel_gemm_dev(rails_ctx *c, double alpha, const double *X, int ldx, int k, const double *C_dev, int r, double beta,
                         double *Y, int ldy, int64_t m)
{
    if (r <= 0 || m <= 0) return RAILS_OK;
    const int vec_ok = dense::rows_vec_ok(X, ldx) ? 1 : 0;
    const dense::PanelGemmChoice p = dense::panel_gemm_choice(r);
    const unsigned grid = (unsigned)((m + 63) / 64);
    switch (p.key()) {
#define RAILS_CASE(TR, KC)                                                                                                                 \
    case dense::inst(TR, KC):                                                                                                              \
        RAILS_LAUNCH((k_panel_gemm<TR, KC>), dim3(grid), dim3(256), 0, c->stream, alpha, X, ldx, k, C_dev, r, beta, Y, ldy, m, vec_ok);    \
        break;
        RAILS_DENSE_PANEL_GEMM_TABLE(RAILS_CASE)
#undef RAILS_CASE
    default: RAILS_REQUIRE(false, "rails_panel_gemm: no k_panel_gemm<%d, %d>", p.tr, p.kc);
    }
    RAILS_HIP_CHECK(hipGetLastError());
    return RAILS_OK;
}

// Y += alpha [X1 X2] C, C (a x r, ld a, a = a1 + a2) on the device; r <= 32
int rails_panel_gemm2_dev(rails_ctx *c, double alpha, const double *X1, int ldx1, int a1, const double *X2, int ldx2, int a2, const double *C_dev,
                          int r, double *Y, int ldy, int64_t m)
{
    if (r <= 0 || m <= 0) return RAILS_OK;
    const int a = a1 + a2;
    const int vec1 = dense::rows_vec_ok(X1, ldx1) ? 1 : 0;
    const int vec2 = (dense::rows_vec_ok(X2, ldx2) && (a1 % 2) == 0) ? 1 : 0; // (its first column is column a1 of the whole)
    const dense::PanelGemmChoice p = dense::panel_gemm2_choice(r);
    const unsigned grid = (unsigned)((m + 63) / 64);
    switch (p.key()) {
#define RAILS_CASE(TR, KC)                                                                                                                 \
    case dense::inst(TR, KC):                                                                                                              \
        RAILS_LAUNCH((k_panel_gemm2<TR, KC>), dim3(grid), dim3(256), 0, c->stream, alpha, X1, ldx1, a1, X2, ldx2, a, C_dev, r, 1.0, Y, ldy, m, vec1, vec2); \
        break;
        RAILS_DENSE_PANEL_GEMM2_TABLE(RAILS_CASE)
#undef RAILS_CASE
    default: RAILS_REQUIRE(false, "rails_panel_gemm2: no k_panel_gemm2<%d, %d>", p.tr, p.kc);
    }
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
    if (k == 0) return scale_only(c, Y, yc0, r, beta);
    RAILS_TRY(upload_coefficients(c, C_host, ldc, k, r));
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
    dense::DenseSwitches sw;
    static const int wide_env = spmm_env("RAILS_PANEL_GEMM_WIDE", 1);
    sw.panel_gemm_wide = wide_env;
    sw.tile_fit = g_dense_tile_fit.get();
    const dense::GemmWidePlan plan = dense::gemm_wide_plan(k, r, sw);
    if (!plan.own_kernel) {
        for (int j0 = 0; j0 < r; j0 += 128) {
            const int nc = std::min(128, r - j0);
            RAILS_TRY(rails_panel_gemm_dev(c, alpha, X->d + xc0, X->ld, k, c->small + (size_t)j0 * k, nc, beta, Y->d + yc0 + j0, Y->ld, X->m));
        }
        return RAILS_OK;
    }
    const int vec_ok = dense::rows_vec_ok(X->d + xc0, X->ld) ? 1 : 0;
    RAILS_TRY(rails_ws_reserve(c, (size_t)plan.nslices * plan.ct_doubles * sizeof(double)));
    for (int j = 0; j < plan.count(); ++j) {
        const dense::GemmWideSlice s = plan.slice(j);
        const double *Cj = c->small + (size_t)s.j0 * k;
        double *Yj = Y->d + yc0 + s.j0, *ct = c->ws + (size_t)j * plan.ct_doubles;
        switch (s.tr) {
#define RAILS_CASE(TR)                                                                                                                     \
    case TR:                                                                                                                               \
        RAILS_TRY((launch_pg_wide<TR>(c, alpha, X->d + xc0, X->ld, k, Cj, s.nc, beta, Yj, Y->ld, X->m, vec_ok, plan.tile_fit ? 1 : 0, ct))); \
        break;
            RAILS_DENSE_GEMM_WIDE_TABLE(RAILS_CASE)
#undef RAILS_CASE
        default: RAILS_REQUIRE(false, "rails_panel_gemm_wide: no k_panel_gemm_wide<%d>", s.tr);
        }
    }
    RAILS_HIP_CHECK(hipGetLastError());
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
    if (k == 0) return scale_only(c, Y, yc0, r, beta);
    RAILS_TRY(upload_coefficients(c, C_host, ldc, k, r));
    return rails_panel_gemm_dev(c, alpha, X->d + xc0, X->ld, k, c->small, r, beta, Y->d + yc0, Y->ld, X->m);
}
