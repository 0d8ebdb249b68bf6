// dense_common.h -- what the tall-skinny dense kernels on v_mfma_f64_16x16x4_f64 (gfx950) share: dense_gram.hip (C = X^T Y, column
// norms), dense_gemm.hip (Y = beta Y + alpha X C) and dense_deferred.hip (the chain of a block orthogonalisation without the host in
// between).  Which kernel takes a call is decided in dense_choice.h.
//
// fp64 MFMA on gfx950 runs at the fp64 vector rate; it is used here because it needs ONE operand
// register per lane per 2048 flop (no LDS broadcast of the small operand, no register tiling),
// which leaves the load path free: the kernels are HBM-bound whenever one small dimension is
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
// a function is optimised once on its own and again after inlining, which alone reordered operands in k_gram.)  The same discipline
// holds between the files: a kernel stands whole in one of them, and nothing is factored out of the two schedules of the fused update.
#pragma once
#include "rails_internal.h"

#include <algorithm>
#include <atomic>

#include "dense_choice.h"

// A process-wide on/off switch of the dense kernels: its setter, or its environment variable, read at the first get() unless the setter
// came first.  The same bits come out either way.
struct DenseSwitch {
    const char *variable;
    int on_by_default;
    std::atomic<int> v{-1}; // -1: not decided yet
    bool get()
    {
        if (v.load(std::memory_order_relaxed) < 0) {
            const char *e = getenv(variable);
            int undecided = -1;
            v.compare_exchange_strong(undecided, (e ? atoi(e) : on_by_default) ? 1 : 0); // (a setter that got in between wins)
        }
        return v.load(std::memory_order_relaxed) != 0;
    }
    void set(int on) { v.store(on ? 1 : 0); }
};
// Tile counts fitted to the widths a solve runs at: k_update_gram<5, .>, k_gram_cols<5, 1, .>, the odd TR of k_panel_gemm_wide and its
// skipped half chunk.  Off: the choices before the fit; the fitted forms leave out work on zero padding and nothing else.
extern DenseSwitch g_dense_tile_fit; // dense_gram.hip: rails_dense_set_tile_fit, RAILS_DENSE_TILE_FIT
// The schedule of the fused update + second projection: k_update_gram_p, or k_update_gram as it was.
extern DenseSwitch g_dense_update_gram_pipeline; // dense_deferred.hip: rails_dense_set_update_gram_pipeline, RAILS_UPDATE_GRAM_PIPELINE

// dense_gram.hip: out[e] = sum over the nslab partial tiles of n doubles at `partial`, in a fixed order (k_reduce_partials)
int rails_reduce_partials(rails_ctx *c, const double *partial, int64_t nslab, int64_t n, double *out);

// A coefficient block on the host (k x r, leading dimension ldc) -> c->small, packed k x r.  Asynchronous: through the pinned staging
// buffer (the next host write into it waits for this upload, rails_pinned_begin_write) into the context's small device buffer (re-used
// in stream order).
inline int upload_coefficients(rails_ctx *c, const double *C_host, int ldc, int k, int r)
{
    const size_t n = (size_t)k * r;
    RAILS_TRY(rails_small_reserve(c, n * sizeof(double)));
    RAILS_TRY(rails_pinned_begin_write(c, n * sizeof(double)));
    for (int j = 0; j < r; ++j) memcpy(c->pinned + (size_t)j * k, C_host + (size_t)j * ldc, sizeof(double) * k);
    RAILS_HIP_CHECK(hipMemcpyAsync(c->small, c->pinned, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    return rails_pinned_end_write(c);
}

namespace {

typedef double v4f64 __attribute__((ext_vector_type(4)));
typedef double v2f64 __attribute__((ext_vector_type(2)));

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

} // namespace
