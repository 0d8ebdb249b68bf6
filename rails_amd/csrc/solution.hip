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
//
//   rails_panel_rowpair   out[i] = sum_{j,l} U[ia_i,j] S[j,l] U[ib_i,l] = X[ia_i, ib_i]
// is the same body (solution_rowform.inc, included once in each kernel) on gathered rows: the wave's A-operand rows are rows ia[.], the
// epilogue multiplies the accumulator tile with rows ib[.].  Same slices, instantiations, packed S, double buffer and summation order; the
// row form is the case ia = ib = identity of it and keeps its code.  The indices are checked on the host and ride behind S in the call's one
// staged upload.
#include "rails_internal.h"

#include <algorithm>
#include <initializer_list>
#include <type_traits>

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

// Which rows of U result i of the shared body (solution_rowform.inc) reads: its own (the row form, n = rows of U) ...
struct SameRows {
    int64_t n;
    __device__ __forceinline__ int64_t a(int64_t i) const { return i; }
    __device__ __forceinline__ int64_t b(int64_t i) const { return i; }
};
// ... or rows ia[i] and ib[i] (the pair form).  The indices were checked on the host.  An identity side (a null array in the call) has its
// flag clear and its pointer at any readable int32: the load is unconditional and its value unused, so that the body stays free of branches
// (with one, the compiler issues the epilogue's loads of U a result group at a time around it and runs out of registers at TR = 16).
struct PairRows {
    const int32_t *ia, *ib;
    int64_t n;
    int use_a, use_b;
    __device__ __forceinline__ int64_t a(int64_t i) const
    {
        const int32_t t = ia[use_a ? i : 0];
        return use_a ? (int64_t)t : i;
    }
    __device__ __forceinline__ int64_t b(int64_t i) const
    {
        const int32_t t = ib[use_b ? i : 0];
        return use_b ? (int64_t)t : i;
    }
};

// out[row] (+)= sum_{j < r} (sum_{l < k} U[row, l] St[l, j]) U[row, j0 + j]; U points at the first column of the window, St is the packed slice
template <int TR>
__global__ __launch_bounds__(512) void k_panel_rowquad(const double *__restrict__ U, int ldu, int k, const double *__restrict__ St /* packed, kpad x RL */, int j0, int r,
                                                       double *__restrict__ out, int ldo, int64_t m, int vec_ok, int accumulate)
{
    const SameRows Rw{m};
#include "solution_rowform.inc"
}

// out[i] (+)= sum_{j < r} (sum_{l < k} U[ia[i], l] St[l, j]) U[ib[i], j0 + j], i < n: the same body on gathered rows.  The four row pointers of
// the epilogue cost a few registers more than the row form's one; up to TR = 8 the kernel is told to stay at the row form's four waves per
// SIMD (two workgroups per CU, which is what the LDS of TR = 8 allows)
template <int TR>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(TR <= 8 ? 4 : 2))) void k_panel_rowpair(const double *__restrict__ U, int ldu, int k, const double *__restrict__ St /* packed, kpad x RL */, int j0, int r,
                                                       double *__restrict__ out, int ldo, const int32_t *__restrict__ ia, const int32_t *__restrict__ ib, int64_t n, int use_a,
                                                       int use_b, int vec_ok, int accumulate)
{
    const PairRows Rw{ia, ib, n, use_a, use_b};
#include "solution_rowform.inc"
}

__global__ void k_zero_rows(double *__restrict__ out, int ldo, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i * ldo] = 0.0;
}

// Out[i, j] <- Out[i, j] / (sqrt(var[i]) sqrt(rv[j])), 0 where either variance is not > 0, and exactly 1 where row i IS reference unknown j
// (rows[j] == i) and its variance is > 0: the covariance map becomes the correlation map
__global__ void k_corr_scale(double *__restrict__ out, int ldo, int64_t m, int q, const double *__restrict__ var, int ldv, const double *__restrict__ rv,
                             const int32_t *__restrict__ rows)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= m * q) return;
    const int64_t i = e / q;
    const int j = (int)(e % q);
    const double vi = var[i * ldv], vj = rv[j];
    double *dst = out + i * ldo + j;
    if (!(vi > 0.0) || !(vj > 0.0))
        *dst = 0.0;
    else
        *dst = ((int64_t)rows[j] == i) ? 1.0 : *dst / (sqrt(vi) * sqrt(vj));
}

// one slice of either form: pack the slice of S, launch the instantiation, note it for rails_panel_rowquad_last_plan
template <int TR, class Rows>
int launch_rowquad(rails_ctx *c, const double *U, int ldu, int k, const double *S_dev, int j0, int r, double *out, int ldo, Rows rw, int vec_ok, int accumulate, double *st)
{
    constexpr int RL = 16 * TR + 4;
    const int kpad = (k + 31) / 32 * 32;
    RAILS_LAUNCH(k_pack_s, dim3((unsigned)std::min<int64_t>(512, ((int64_t)kpad * RL + 255) / 256)), dim3(256), 0, c->stream, S_dev + (size_t)j0 * k, k, k, r, kpad, RL, st);
    const size_t lds = (size_t)2 * 32 * RL * sizeof(double);
    const dim3 grid((unsigned)((rw.n + 127) / 128));
    if constexpr (std::is_same<Rows, SameRows>::value) {
        RAILS_HIP_CHECK(hipFuncSetAttribute((const void *)k_panel_rowquad<TR>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        RAILS_LAUNCH((k_panel_rowquad<TR>), grid, dim3(512), lds, c->stream, U, ldu, k, st, j0, r, out, ldo, rw.n, vec_ok, accumulate);
    } else {
        RAILS_HIP_CHECK(hipFuncSetAttribute((const void *)k_panel_rowpair<TR>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        RAILS_LAUNCH((k_panel_rowpair<TR>), grid, dim3(512), lds, c->stream, U, ldu, k, st, j0, r, out, ldo, rw.ia, rw.ib, rw.n, rw.use_a, rw.use_b, vec_ok, accumulate);
    }
    c->last_rowquad_tr[c->last_rowquad_nslices++] = TR; // k <= 512: two slices at most
    return RAILS_OK;
}

// S (k x k, leading dimension lds) and the pair form's index arrays (n entries each; null: none) go to the device once, through the pinned
// staging buffer into the context's small buffer (re-used in stream order): S first, then each array on an 8-byte boundary.  *ia_dev and
// *ib_dev (may be null pointers-to) receive where the arrays will be.
int stage_small(rails_ctx *c, int k, const double *S_host, int lds, const int32_t *ia, const int32_t *ib, int64_t n, const int32_t **ia_dev, const int32_t **ib_dev)
{
    const size_t ns = (size_t)k * k, each = ((size_t)n * sizeof(int32_t) + 7) / 8, na = ia ? each : 0, nb = ib ? each : 0; // in doubles
    const size_t bytes = (ns + na + nb) * sizeof(double);
    RAILS_TRY(rails_small_reserve(c, bytes));
    RAILS_TRY(rails_pinned_begin_write(c, bytes));
    for (int j = 0; j < k; ++j) memcpy(c->pinned + (size_t)j * k, S_host + (size_t)j * lds, sizeof(double) * k);
    if (ia) memcpy(c->pinned + ns, ia, (size_t)n * sizeof(int32_t));
    if (ib) memcpy(c->pinned + ns + na, ib, (size_t)n * sizeof(int32_t));
    RAILS_HIP_CHECK(hipMemcpyAsync(c->small, c->pinned, bytes, hipMemcpyHostToDevice, c->stream));
    if (ia_dev) *ia_dev = ia ? reinterpret_cast<const int32_t *>(c->small + ns) : nullptr;
    if (ib_dev) *ib_dev = ib ? reinterpret_cast<const int32_t *>(c->small + ns + na) : nullptr;
    return rails_pinned_end_write(c);
}

// the slices of either form, S already in c->small: equal widths, at most 256 columns of S (16 tiles of 16: the accumulators of a wave), one
// launch each, the later ones adding to the output column (stream order)
template <class Rows>
int rowform_slices(rails_ctx *c, const rails_panel *U, int c0, int k, Rows rw, double *od, int ldo)
{
    const int nslices = (k + 255) / 256, width = ((k + nslices - 1) / nslices + 15) / 16 * 16;
    const size_t st_doubles = (size_t)((k + 31) / 32 * 32) * (16 * 16 + 4);
    RAILS_TRY(rails_ws_reserve(c, (size_t)nslices * st_doubles * sizeof(double)));
    const double *Ud = U->d + c0;
    const int vec_ok = ((((uintptr_t)Ud) & 15) == 0 && (U->ld % 2) == 0) ? 1 : 0;
    int slice = 0;
    for (int j0 = 0; j0 < k; j0 += width, ++slice) {
        const int nc = std::min(width, k - j0), tiles = (nc + 15) / 16, acc = slice > 0 ? 1 : 0;
        double *st = c->ws + (size_t)slice * st_doubles;
        if (tiles <= 2)
            RAILS_TRY((launch_rowquad<2>(c, Ud, U->ld, k, c->small, j0, nc, od, ldo, rw, vec_ok, acc, st)));
        else if (tiles <= 4)
            RAILS_TRY((launch_rowquad<4>(c, Ud, U->ld, k, c->small, j0, nc, od, ldo, rw, vec_ok, acc, st)));
        else if (tiles <= 8)
            RAILS_TRY((launch_rowquad<8>(c, Ud, U->ld, k, c->small, j0, nc, od, ldo, rw, vec_ok, acc, st)));
        else if (tiles <= 12)
            RAILS_TRY((launch_rowquad<12>(c, Ud, U->ld, k, c->small, j0, nc, od, ldo, rw, vec_ok, acc, st)));
        else
            RAILS_TRY((launch_rowquad<16>(c, Ud, U->ld, k, c->small, j0, nc, od, ldo, rw, vec_ok, acc, st)));
    }
    RAILS_HIP_CHECK(hipGetLastError());
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
    RAILS_TRY(stage_small(c, k, S_host, lds, nullptr, nullptr, 0, nullptr, nullptr));
    RAILS_TRY(rowform_slices(c, U, c0, k, SameRows{U->m}, Out->d + oc0, Out->ld));
    c->n_rowquad++;
    return RAILS_OK;
}

// The pair form, out[i] = X[ia[i], ib[i]]: the row form's kernel body, slices, packed S and summation order on rows gathered through two
// index arrays.  The indices travel behind S in the one staged upload of the call.
extern "C" int rails_panel_rowpair(rails_ctx *c, const rails_panel *U, int c0, int k, const double *S_host, int lds, const int32_t *ia, const int32_t *ib, int64_t n,
                                   rails_panel *Out, int oc0)
{
    if (c) hipSetDevice(c->device);
    rails_slow_guard slow__(c, "rails_panel_rowpair", k, (long long)n);
    RAILS_REQUIRE(c && U && Out, "rails_panel_rowpair: null argument");
    RAILS_REQUIRE(k >= 0 && k <= 512, "rails_panel_rowpair: k = %d outside [0, 512]", k);
    RAILS_REQUIRE(c0 >= 0 && c0 + k <= U->cap && oc0 >= 0 && oc0 < Out->cap, "rails_panel_rowpair: window [%d,%d) / column %d outside capacities %d / %d", c0, c0 + k, oc0,
                  U->cap, Out->cap);
    RAILS_REQUIRE(n >= 0 && n <= Out->m, "rails_panel_rowpair: %lld pairs for an output panel of %lld rows", (long long)n, (long long)Out->m);
    RAILS_REQUIRE((ia && ib) || n <= U->m, "rails_panel_rowpair: a null index array is the identity, and %lld pairs exceed the %lld rows of U", (long long)n, (long long)U->m);
    RAILS_REQUIRE(k == 0 || (S_host && lds >= k), "rails_panel_rowpair: bad small matrix (leading dimension %d < %d)", lds, k);
    if (U->d == Out->d) RAILS_REQUIRE(oc0 < c0 || oc0 >= c0 + k, "rails_panel_rowpair: the output column lies inside the input window");
    c->last_rowquad_nslices = 0;
    if (n == 0 || U->m == 0) return RAILS_OK;
    for (const int32_t *idx : {ia, ib})
        for (int64_t i = 0; idx && i < n; ++i)
            RAILS_REQUIRE(idx[i] >= 0 && idx[i] < U->m, "rails_panel_rowpair: index %d at %lld outside [0, %lld)", idx[i], (long long)i, (long long)U->m);
    if (k == 0) {
        RAILS_LAUNCH(k_zero_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, Out->d + oc0, Out->ld, n);
        RAILS_HIP_CHECK(hipGetLastError());
        return RAILS_OK;
    }
    PairRows rw{nullptr, nullptr, n, ia ? 1 : 0, ib ? 1 : 0};
    RAILS_TRY(stage_small(c, k, S_host, lds, ia, ib, n, &rw.ia, &rw.ib)); // [S | ia | ib] in one upload
    const int32_t *readable = reinterpret_cast<const int32_t *>(c->small);  // an identity side reads (and ignores) S's first word
    if (!ia) rw.ia = readable;
    if (!ib) rw.ib = readable;
    RAILS_TRY(rowform_slices(c, U, c0, k, rw, Out->d + oc0, Out->ld));
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

// host[0..n) summed over the ranks of the partition, with the context's all-reduce (the one rails_gram uses); one rank without a hook or a
// communicator: nothing happens, nothing is queued.  Synchronises otherwise.
extern "C" int rails_allreduce_host(rails_ctx *c, double *host, int64_t n)
{
    if (c) hipSetDevice(c->device);
    RAILS_REQUIRE(c && n >= 0 && (n == 0 || host), "rails_allreduce_host: null argument");
    if (n == 0 || (c->nranks <= 1 && !c->allreduce && !c->rccl)) return RAILS_OK;
    const size_t bytes = (size_t)n * sizeof(double);
    RAILS_TRY(rails_small_reserve(c, bytes));
    RAILS_TRY(rails_pinned_begin_write(c, bytes));
    memcpy(c->pinned, host, bytes);
    RAILS_HIP_CHECK(hipMemcpyAsync(c->small, c->pinned, bytes, hipMemcpyHostToDevice, c->stream));
    RAILS_TRY(rails_pinned_end_write(c));
    RAILS_TRY(rails_allreduce_dev(c, c->small, (size_t)n));
    RAILS_HIP_CHECK(hipMemcpyAsync(c->pinned, c->small, bytes, hipMemcpyDeviceToHost, c->stream));
    RAILS_HIP_CHECK(rails_stream_sync(c));
    memcpy(host, c->pinned, bytes);
    return RAILS_OK;
}

// Covariances to correlations: Out[i, oc0 + j] /= sqrt(Var[i, vc]) sqrt(rv[j]) for j < q, 0 where either variance is not > 0, exactly 1 where
// i == rows[j] (the unknown with itself) and its variance is > 0.  rv and rows on the host (q <= 64 entries each).  Asynchronous.
extern "C" int rails_panel_corr_scale(rails_ctx *c, rails_panel *Out, int oc0, int q, const rails_panel *Var, int vc, const double *rv_host, const int32_t *rows_host)
{
    if (c) hipSetDevice(c->device);
    RAILS_REQUIRE(c && Out && Var && (q == 0 || (rv_host && rows_host)), "rails_panel_corr_scale: null argument");
    RAILS_REQUIRE(q >= 0 && q <= 64 && oc0 >= 0 && oc0 + q <= Out->cap && vc >= 0 && vc < Var->cap, "rails_panel_corr_scale: bad windows");
    RAILS_REQUIRE(Out->m == Var->m, "rails_panel_corr_scale: row mismatch %lld vs %lld", (long long)Out->m, (long long)Var->m);
    if (Out->d == Var->d) RAILS_REQUIRE(vc < oc0 || vc >= oc0 + q, "rails_panel_corr_scale: the variance column lies inside the scaled window");
    if (q == 0 || Out->m == 0) return RAILS_OK;
    const size_t nd = (size_t)q + ((size_t)q * sizeof(int32_t) + 7) / 8; // doubles: rv, then rows
    RAILS_TRY(rails_small_reserve(c, nd * sizeof(double)));
    RAILS_TRY(rails_pinned_begin_write(c, nd * sizeof(double)));
    memcpy(c->pinned, rv_host, (size_t)q * sizeof(double));
    memcpy(c->pinned + q, rows_host, (size_t)q * sizeof(int32_t));
    RAILS_HIP_CHECK(hipMemcpyAsync(c->small, c->pinned, nd * sizeof(double), hipMemcpyHostToDevice, c->stream));
    RAILS_TRY(rails_pinned_end_write(c));
    const int64_t work = Out->m * q;
    RAILS_LAUNCH(k_corr_scale, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, c->stream, Out->d + oc0, Out->ld, Out->m, q, Var->d + vc, Var->ld, c->small,
                 reinterpret_cast<const int32_t *>(c->small + q));
    RAILS_HIP_CHECK(hipGetLastError());
    return RAILS_OK;
}
