// solution.hip -- the device kernel of the solution object (include/rails_solution.h):
//   rails_panel_rowquad   out[i] = sum_{j,l} U[i,j] S[j,l] U[i,l] = diag(U S U')_i
// the pointwise variance of a low-rank solution X = U S U' (the field the reference's application is solved for; its driver gets at the
// full covariance only through products, src/SchurOperator.cpp:191-342).
//
// One pass over U and no m x k temporary: a wave owns 16 rows.  Its 16 x k row tile is the A operand of v_mfma_f64_16x16x4 (lane l supplies
// U[row l&15][column 4s + (l>>4)]), S streams through LDS in chunks of 32 of its rows as the B operand -- the double buffer fed by LDS-DMA
// that k_panel_gemm_wide (dense_gemm.hip) uses, in the same packed layout, row length 16 TR + 4 doubles so that the four row groups of a wave
// read different banks -- and the product tile P = U_tile S stays in the accumulators (TR <= 16 column tiles, 64 doubles per lane).  The
// epilogue multiplies it with U_tile again where it sits: lane l holds P[row (l>>4) + 4v][column 16t + (l&15)], reads the matching entries of U
// (the lines the wave has just read: L2 / L0 hits), sums its own columns and the 16 lanes of a row group are added by four xor-shuffles, a
// fixed order: the result does not depend on the launch.  k > 256 is done in slices of at most 256 columns of S, one launch each, the later
// ones adding to `out` (stream order).  Extra device memory: the packed S (k x (k + 4) doubles at most per slice) and the m results.
//
// 8 waves x 16 rows per workgroup; LDS is 2 x 32 x (16 TR + 4) doubles: 66 KiB at k = 128 (two workgroups per CU), 130 KiB at 256.
#include "rails_internal.h"

#include <algorithm>

namespace {

typedef double v4f64 __attribute__((ext_vector_type(4)));
typedef double v2f64 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ v4f64 mfma_f64(double a, double b, v4f64 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// S slice (k x r, column-major, leading dimension lds) -> packed kpad x RL, zero padded: row kl of the slice's columns, contiguous
__global__ void k_pack_s(const double *__restrict__ S, int lds, int k, int r, int kpad, int RL, double *__restrict__ out)
{
    const int64_t n = (int64_t)kpad * RL;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
        const int kl = (int)(q / RL), j = (int)(q % RL);
        out[q] = (kl < k && j < r) ? S[kl + (int64_t)j * lds] : 0.0;
    }
}

// out[row] (+)= sum_{j < r} (sum_{l < k} U[row, l] St[l, j]) U[row, j0 + j]; U points at the first column of the window, St is the packed slice
template <int TR>
__global__ __launch_bounds__(512) void k_panel_rowquad(const double *__restrict__ U, int ldu, int k, const double *__restrict__ St /* packed, kpad x RL */, int j0, int r,
                                                       double *__restrict__ out, int ldo, int64_t m, int vec_ok, int accumulate)
{
    constexpr int KC = 32, RL = 16 * TR + 4, CHUNK_B = KC * RL * 8, PIECES = CHUNK_B / 1024;
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
        const char *src = reinterpret_cast<const char *>(St) + (size_t)chunk * CHUNK_B;
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
    const double *xrow = U + (rowok ? myrow : m - 1) * ldu; // rows past the end read the last row; their results are never written
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
        fetch((ci + 1) * KC + 4 * kk, xc); // past k: zeros, no load
        fetch((ci + 1) * KC + 16 + 4 * kk, xd);
        const double *cb = Cs + (size_t)(ci & 1) * (KC * RL);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const double *crow = &cb[(4 * kk + s) * RL + li];
#pragma unroll
            for (int t = 0; t < TR; ++t) acc[t] = mfma_f64(xa[s], crow[16 * t], acc[t]);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const double *crow = &cb[(16 + 4 * kk + s) * RL + li];
#pragma unroll
            for (int t = 0; t < TR; ++t) acc[t] = mfma_f64(xb[s], crow[16 * t], acc[t]);
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
    // P[row kk + 4v][column 16t + li] is in acc[t][v]: times U at the same place, summed over the columns
    double q[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const int64_t row = r0 + kk + 4 * v;
        const double *urow = U + (row < m ? row : m - 1) * ldu + j0;
#pragma unroll
        for (int t = 0; t < TR; ++t) {
            const int j = 16 * t + li;
            const double u = urow[j < r ? j : 0]; // columns past the slice: acc is zero there (zero padding of the packed S)
            q[v] += acc[t][v] * (j < r ? u : 0.0);
        }
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) q[v] += __shfl_xor(q[v], off, 64);
    }
    if (li == 0) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int64_t row = r0 + kk + 4 * v;
            if (row >= m) continue;
            double *dst = out + row * ldo;
            *dst = accumulate ? *dst + q[v] : q[v];
        }
    }
}

template <int TR>
int launch_rowquad(rails_ctx *c, const double *U, int ldu, int k, const double *S_dev, int j0, int r, double *out, int ldo, int64_t m, int vec_ok, int accumulate, double *st)
{
    constexpr int RL = 16 * TR + 4;
    const int kpad = (k + 31) / 32 * 32;
    RAILS_LAUNCH(k_pack_s, dim3((unsigned)std::min<int64_t>(512, ((int64_t)kpad * RL + 255) / 256)), dim3(256), 0, c->stream, S_dev + (size_t)j0 * k, k, k, r, kpad, RL, st);
    const size_t lds = (size_t)2 * 32 * RL * sizeof(double);
    RAILS_HIP_CHECK(hipFuncSetAttribute((const void *)k_panel_rowquad<TR>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    RAILS_LAUNCH((k_panel_rowquad<TR>), dim3((unsigned)((m + 127) / 128)), dim3(512), lds, c->stream, U, ldu, k, st, j0, r, out, ldo, m, vec_ok, accumulate);
    c->last_rowquad_tr[c->last_rowquad_nslices++] = TR; // k <= 512: two slices at most
    return RAILS_OK;
}

} // namespace

extern "C" int rails_panel_rowquad(rails_ctx *c, const rails_panel *U, int c0, int k, const double *S_host, int lds, rails_panel *Out, int oc0)
{
    if (c) hipSetDevice(c->device);
    rails_slow_guard slow__(c, "rails_panel_rowquad", k, U ? (long long)U->m : 0);
    RAILS_REQUIRE(c && U && Out, "rails_panel_rowquad: null argument");
    RAILS_REQUIRE(k >= 0 && k <= 512, "rails_panel_rowquad: k = %d outside [0, 512]", k);
    RAILS_REQUIRE(c0 >= 0 && c0 + k <= U->cap && oc0 >= 0 && oc0 < Out->cap, "rails_panel_rowquad: window [%d,%d) / column %d outside capacities %d / %d", c0, c0 + k, oc0,
                  U->cap, Out->cap);
    RAILS_REQUIRE(U->m == Out->m, "rails_panel_rowquad: row mismatch %lld vs %lld", (long long)U->m, (long long)Out->m);
    RAILS_REQUIRE(k == 0 || (S_host && lds >= k), "rails_panel_rowquad: bad small matrix (leading dimension %d < %d)", lds, k);
    if (U->d == Out->d) RAILS_REQUIRE(oc0 < c0 || oc0 >= c0 + k, "rails_panel_rowquad: the output column lies inside the input window");
    c->last_rowquad_nslices = 0;
    if (U->m == 0) return RAILS_OK;
    if (k == 0) return rails_panel_fill(c, Out, oc0, 1, 0.0);
    // S goes to the device once, through the pinned staging buffer into the context's small buffer (re-used in stream order)
    const size_t n = (size_t)k * k;
    RAILS_TRY(rails_small_reserve(c, n * sizeof(double)));
    RAILS_TRY(rails_pinned_begin_write(c, n * sizeof(double)));
    for (int j = 0; j < k; ++j) memcpy(c->pinned + (size_t)j * k, S_host + (size_t)j * lds, sizeof(double) * k);
    RAILS_HIP_CHECK(hipMemcpyAsync(c->small, c->pinned, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    RAILS_TRY(rails_pinned_end_write(c));
    // slices of equal width, at most 256 columns of S (16 tiles of 16: the accumulators of a wave)
    const int nslices = (k + 255) / 256, width = ((k + nslices - 1) / nslices + 15) / 16 * 16;
    const size_t st_doubles = (size_t)((k + 31) / 32 * 32) * (16 * 16 + 4);
    RAILS_TRY(rails_ws_reserve(c, (size_t)nslices * st_doubles * sizeof(double)));
    const double *Ud = U->d + c0;
    const int vec_ok = ((((uintptr_t)Ud) & 15) == 0 && (U->ld % 2) == 0) ? 1 : 0;
    double *od = Out->d + oc0;
    int slice = 0;
    for (int j0 = 0; j0 < k; j0 += width, ++slice) {
        const int nc = std::min(width, k - j0), tiles = (nc + 15) / 16, acc = slice > 0 ? 1 : 0;
        double *st = c->ws + (size_t)slice * st_doubles;
        if (tiles <= 2)
            RAILS_TRY((launch_rowquad<2>(c, Ud, U->ld, k, c->small, j0, nc, od, Out->ld, U->m, vec_ok, acc, st)));
        else if (tiles <= 4)
            RAILS_TRY((launch_rowquad<4>(c, Ud, U->ld, k, c->small, j0, nc, od, Out->ld, U->m, vec_ok, acc, st)));
        else if (tiles <= 8)
            RAILS_TRY((launch_rowquad<8>(c, Ud, U->ld, k, c->small, j0, nc, od, Out->ld, U->m, vec_ok, acc, st)));
        else if (tiles <= 12)
            RAILS_TRY((launch_rowquad<12>(c, Ud, U->ld, k, c->small, j0, nc, od, Out->ld, U->m, vec_ok, acc, st)));
        else
            RAILS_TRY((launch_rowquad<16>(c, Ud, U->ld, k, c->small, j0, nc, od, Out->ld, U->m, vec_ok, acc, st)));
    }
    RAILS_HIP_CHECK(hipGetLastError());
    c->n_rowquad++;
    return RAILS_OK;
}

// what the context's last rails_panel_rowquad launched: the number of slices and the TR of k_panel_rowquad<TR> for the first `cap` of them
extern "C" int rails_panel_rowquad_last_plan(const rails_ctx *c, int *nslices, int *tr, int cap)
{
    RAILS_REQUIRE(c && nslices && (tr || cap <= 0), "rails_panel_rowquad_last_plan: null argument");
    *nslices = c->last_rowquad_nslices;
    for (int q = 0; q < cap && q < c->last_rowquad_nslices; ++q) tr[q] = c->last_rowquad_tr[q];
    return RAILS_OK;
}

namespace {

// scatter == 0: Y row i <- X row idx[i]; scatter != 0: Y row idx[i] <- X row i; i < n
__global__ void k_move_rows(const double *__restrict__ X, int ldx, const int32_t *__restrict__ idx, int scatter, double *__restrict__ Y, int ldy, int64_t n, int nc)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n * nc) return;
    const int64_t i = q / nc;
    const int j = (int)(q % nc);
    const int64_t src = scatter ? i : idx[i], dst = scatter ? idx[i] : i;
    Y[dst * ldy + j] = X[src * ldx + j];
}

} // namespace

// Rows moved between panels of DIFFERENT row counts (rails_panel_permute_rows wants equal ones): the row gather of rails_solution_block and
// the row scatter that puts the two parts of a lifted Schur solution into the original row order.  The indices come from the host and are
// checked here, so that no index leaves the panels.
extern "C" int rails_panel_move_rows(rails_ctx *c, const rails_panel *X, int xc0, int nc, const int32_t *idx_host, int64_t n, int scatter, rails_panel *Y, int yc0)
{
    if (c) hipSetDevice(c->device);
    RAILS_REQUIRE(c && X && Y && (n == 0 || idx_host), "rails_panel_move_rows: null argument");
    RAILS_REQUIRE(n >= 0 && nc >= 0 && xc0 >= 0 && yc0 >= 0 && xc0 + nc <= X->cap && yc0 + nc <= Y->cap, "rails_panel_move_rows: bad windows");
    RAILS_REQUIRE(X->d != Y->d, "rails_panel_move_rows: in place is not supported");
    const int64_t lim = scatter ? Y->m : X->m;
    RAILS_REQUIRE(n <= (scatter ? X->m : Y->m), "rails_panel_move_rows: %lld indices for a panel of %lld rows", (long long)n, (long long)(scatter ? X->m : Y->m));
    for (int64_t i = 0; i < n; ++i) RAILS_REQUIRE(idx_host[i] >= 0 && idx_host[i] < lim, "rails_panel_move_rows: index %d at %lld outside [0, %lld)", idx_host[i], (long long)i, (long long)lim);
    if (n == 0 || nc == 0) return RAILS_OK;
    const size_t bytes = ((size_t)n * sizeof(int32_t) + 7) / 8 * 8;
    RAILS_TRY(rails_small_reserve(c, bytes));
    RAILS_TRY(rails_pinned_begin_write(c, bytes));
    memcpy(c->pinned, idx_host, (size_t)n * sizeof(int32_t));
    RAILS_HIP_CHECK(hipMemcpyAsync(c->small, c->pinned, bytes, hipMemcpyHostToDevice, c->stream));
    RAILS_TRY(rails_pinned_end_write(c));
    const int64_t work = n * nc;
    RAILS_LAUNCH(k_move_rows, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, c->stream, X->d + xc0, X->ld, (const int32_t *)c->small, scatter ? 1 : 0, Y->d + yc0, Y->ld, n, nc);
    RAILS_HIP_CHECK(hipGetLastError());
    return RAILS_OK;
}
