// Internal declarations shared by the HIP translation units of librails_hip.so.
#ifndef RAILS_INTERNAL_H
#define RAILS_INTERNAL_H

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <ctime>
#include <string>
#include <vector>

#include "rails_hip.h"

void rails_set_error(const char *fmt, ...);

#define RAILS_HIP_CHECK(expr)                                                                      \
    do {                                                                                           \
        hipError_t e__ = (expr);                                                                   \
        if (e__ != hipSuccess) {                                                                   \
            rails_set_error("%s:%d: %s failed: %s", __FILE__, __LINE__, #expr, hipGetErrorString(e__)); \
            return RAILS_EHIP;                                                                     \
        }                                                                                          \
    } while (0)

#define RAILS_REQUIRE(cond, ...)                                                                   \
    do {                                                                                           \
        if (!(cond)) {                                                                             \
            rails_set_error(__VA_ARGS__);                                                          \
            return RAILS_EINVAL;                                                                   \
        }                                                                                          \
    } while (0)

#define RAILS_TRY(expr)                                                                            \
    do {                                                                                           \
        int rc__ = (expr);                                                                         \
        if (rc__ != RAILS_OK) return rc__;                                                         \
    } while (0)

// pad the leading dimension to a multiple of 16 doubles (128 B): every row starts on a cache line
static inline int rails_pad_ld(int capacity) { return ((capacity < 1 ? 1 : capacity) + 15) / 16 * 16; }

struct rails_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // second stream + fork / join events: work that may run beside the first stream's (the interior rows of a row-partitioned product
    // while the ghost rows travel); made on first use (rails_ctx_second_stream)
    hipStream_t stream2 = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    int num_cu = 256;
    // RNG
    uint64_t seed = 1;
    uint64_t next_stream = 0;
    // partition
    int rank = 0, nranks = 1;
    int64_t row0 = 0, m_global = -1;
    rails_allreduce_fn allreduce = nullptr;
    void *allreduce_user = nullptr;
    // RCCL communicator over the ranks of the partition (rccl_comm.hip); used when no hook is installed
    void *rccl = nullptr;
    bool own_rccl = false;
    int rccl_nranks = 0, rccl_rank = 0;
    // device workspace for reduction partials / small matrices
    double *ws = nullptr;
    size_t ws_bytes = 0;
    // device buffers of destroyed panels, kept for the next panel of the same size (stream-ordered re-use: no synchronisation,
    // no allocator call inside a solve that creates and drops temporaries of a few recurring sizes)
    std::vector<std::pair<size_t, double *>> free_panels;
    size_t free_panel_bytes = 0;
    // second device scratch (small matrices uploaded per call)
    double *small = nullptr;
    size_t small_bytes = 0;
    // pinned host staging
    double *pinned = nullptr;
    size_t pinned_bytes = 0;
    // timing
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev_h2d = nullptr; // recorded after an asynchronous upload out of `pinned`; waited for before the host writes there again
    bool h2d_pending = false;
    // deferred small results (dense_deferred.hip: rails_gram_deferred ...): slots of `defer_slot` doubles on the device with a pinned mirror
    double *defer_dev = nullptr, *defer_pin = nullptr;
    size_t defer_slot = 0;
    int defer_nslots = 0;
    // busy meter (rails_ctx_set_meter): a pair of events around every launch; the pairs are read at the next synchronisation of the stream
    bool meter = false;
    std::vector<hipEvent_t> meter_events; // 2 x RAILS_METER_PAIRS
    int meter_open = 0;                   // pairs recorded since the last synchronisation
    long meter_missed = 0;                // launches that found no free pair
    double gpu_busy_ms = 0.0;
    // counters (rails_ctx_stats)
    void *lz = nullptr; // rails_lanczos_state (lanczos.hip), released by rails_lanczos_release
    long n_orth_block = 0, n_orth_columnwise = 0, n_spmm_tiled = 0, n_spmm_planes = 0, n_spmm_overlapped = 0, n_spmm_sweep = 0, n_spmm_rowgather = 0, n_spmm_callback = 0, n_dev_alloc = 0, n_allreduce = 0, n_lanczos = 0, n_lanczos_start = 0, n_orth_repair = 0, n_update_gram_fused = 0, n_rowquad = 0;
    long n_orth_range = 0, n_orth_range_passes = 0, n_orth_range_syncs = 0; // rails_orthogonalize_range: calls, passes over a block of columns, host synchronisations
    // template parameter of the last launch of k_update_gram<NBW, .>, k_gram_cols[2]<TI, ., .> and k_panel_gemm_wide<TR> (rails_dense_last_tiles); 0: none yet
    int last_update_gram_nbw = 0, last_gram_cols_ti = 0, last_gemm_wide_tr = 0;
    int last_update_gram_form = 0; // the fused update + second projection's last launch: 1 k_update_gram, 2 k_update_gram_p (rails_dense_last_update_gram_form); 0: none yet
    // slices of the last rails_panel_rowquad and the template parameter of k_panel_rowquad<TR> each one launched (rails_panel_rowquad_last_plan); 0 slices: none yet, or k = 0
    int last_rowquad_nslices = 0, last_rowquad_tr[2] = {0, 0};
};

// the busy meter (see rails_ctx): RAILS_LAUNCH brackets a launch, rails_stream_sync reads what has been bracketed since the last one
constexpr int RAILS_METER_PAIRS = 512;
inline bool rails_meter_before(rails_ctx *c)
{
    if (!c->meter) return false;
    if (c->meter_open >= RAILS_METER_PAIRS) {
        c->meter_missed++;
        return false;
    }
    hipEventRecord(c->meter_events[2 * c->meter_open], c->stream);
    return true;
}
inline void rails_meter_after(rails_ctx *c) { hipEventRecord(c->meter_events[2 * c->meter_open++ + 1], c->stream); }
inline hipError_t rails_stream_sync(rails_ctx *c)
{
    const hipError_t e = hipStreamSynchronize(c->stream);
    for (int i = 0; i < c->meter_open; ++i) {
        float ms = 0.0f;
        if (e == hipSuccess && hipEventElapsedTime(&ms, c->meter_events[2 * i], c->meter_events[2 * i + 1]) == hipSuccess) c->gpu_busy_ms += ms;
    }
    c->meter_open = 0;
    return e;
}
#define RAILS_LAUNCH(...)                                                                                                                  \
    do {                                                                                                                                   \
        const bool rails_metered = rails_meter_before(c);                                                                                  \
        hipLaunchKernelGGL(__VA_ARGS__);                                                                                                   \
        if (rails_metered) rails_meter_after(c);                                                                                           \
    } while (0)

struct rails_panel {
    rails_ctx *ctx = nullptr;
    double *d = nullptr;
    int64_t m = 0; // local rows (+ ghost rows for operator inputs are held separately)
    int cap = 0;
    int ld = 0;
};

struct rails_planes_plan; // spmm_planes.hip: coefficient records of a structured-grid stencil
struct rails_sweep_cache; // spmm_sweep.hip: device copies of the sweep kernel's schedules, one per column-chunk count
struct rails_tile_cache;  // spmm_tiled.hip: device copy of the LDS-staged kernels' tile plan (tile_plan.h) and what they last launched
struct rails_bsr;         // spmm_bsr.hip: a block-CSR matrix on the device, with its host copy and its lazily built transposed copy

struct rails_csr {
    rails_ctx *ctx = nullptr;
    rails_sweep_cache *sweep = nullptr;
    rails_planes_plan *planes = nullptr;
    rails_tile_cache *tiled = nullptr;
    int64_t m = 0, ncols_ext = 0, nnz = 0;
    bool rect = false; // rails_csr_create_rect: n_rows x n_cols with n_cols != n_rows, all columns local (X has ncols_ext rows, Y has m)
    int64_t *rowptr = nullptr;
    int32_t *col = nullptr;
    double *val = nullptr;
    int max_row_nnz = 0;
    int64_t window_rows = 0; // mean (max col - min col + 1) over a sample of rows: the sliding window of X rows a row block gathers from
    // transposed copy, built lazily
    rails_csr *AT = nullptr;
    // host copy kept for building the transpose / tiling analysis
    std::vector<int64_t> h_rowptr;
    std::vector<int32_t> h_col;
    std::vector<double> h_val;
    // halo
    int64_t n_send = 0, n_ghost = 0;
    int64_t int_lo = 0, int_hi = 0; // interior rows [int_lo, int_hi): no ghost columns (rails_csr_set_halo)
    int64_t window_rows_int = 0;    // window_rows of the interior rows alone
    int64_t *send_rows = nullptr;
    double *send_buf = nullptr;
    double *ext = nullptr; // [m + n_ghost] x ld_ext staging of X with ghosts appended
    size_t send_cap = 0, ext_cap = 0;
    rails_halo_fn halo = nullptr;
    void *halo_user = nullptr;
    std::vector<int64_t> send_counts, recv_counts; // rows per neighbour rank (rails_csr_set_halo_counts): the RCCL form of the exchange
    int variant = 0;  // rails_csr_set_variant: the kernel rails_spmm is to take (0: its own choice)
    int is_grid = -1; // structured-grid stencil? (-1: not looked at yet; rails_csr_is_grid, spmm.hip)
    const char *last_kernel = "";
    // What rails_spmm does with the operator: multiplies by the stored matrix, or hands the panels to a delegate -- the action given to
    // rails_csr_create_callback (apply_fn with `delegate` as its user pointer), a sparse LU (rails_csr_create_lu, splu.hip: rails_lu_solve),
    // a sparse right-hand side (rails_csr_create_sprhs, sprhs.hip: rails_sprhs_apply) or an iterative solve (rails_csr_create_iter,
    // itsolve.hip: rails_iter_solve).  The caller owns the delegate object -- except a block-CSR matrix (rails_csr_create_bsr, spmm_bsr.hip:
    // rails_bsr_apply), which the handle owns and which keeps rowptr / col / val and their host copies empty.
    enum Kind { STORED, CALLBACK, LU, SPRHS, ITER, BSR } kind = STORED;
    void *delegate = nullptr;
    rails_apply_fn apply_fn = nullptr;
    rails_lu *lu() const { return kind == LU ? static_cast<rails_lu *>(delegate) : nullptr; }
    rails_sprhs *sprhs() const { return kind == SPRHS ? static_cast<rails_sprhs *>(delegate) : nullptr; }
    rails_iter *iter() const { return kind == ITER ? static_cast<rails_iter *>(delegate) : nullptr; }
    rails_bsr *bsr() const { return kind == BSR ? static_cast<rails_bsr *>(delegate) : nullptr; }
};

// Sparse right-hand side B (m x p) and its transpose, both as rectangular CSR operators on the device (sprhs.hip), and the host-made plan
// of the transposed product c = B'r of the fused Lanczos (lanczos.hip): transposed rows of at most RAILS_SPRHS_SHORT entries are summed by
// one thread each, longer ones are cut into items of RAILS_SPRHS_CHUNK entries, one wave per item, and their partial sums added per row
// in item order.
constexpr int RAILS_SPRHS_SHORT = 32;
constexpr int RAILS_SPRHS_CHUNK = 512;
struct rails_sprhs {
    rails_ctx *ctx = nullptr;
    int64_t m = 0, nnz = 0;
    int p = 0;
    rails_csr *B = nullptr;  // m x max(p, 1)
    rails_csr *Bt = nullptr; // max(p, 1) x m, from rails_csr_transpose_host
    double gram_norm2 = 0.0; // ||B'B||_F^2 (rails_csr_gram_norm2_host)
    // items of the long transposed rows: entries [item_beg[i], item_beg[i] + item_len[i]) of Bt; long row l is long_row[l], its items
    // [long_item0[l], long_item0[l + 1])
    int64_t n_items = 0, n_long = 0;
    int64_t *item_beg = nullptr;
    int32_t *item_len = nullptr;
    int32_t *long_row = nullptr;
    int64_t *long_item0 = nullptr;
    double *item_partial = nullptr; // n_items doubles
};

// Diagnostics: with RAILS_TRACE_SLOW_MS=x every guarded entry point synchronises before and after its work and reports on stderr
// when it took longer than x ms (finds the one call behind a slow trip; off by default: no synchronisation, no cost).
struct rails_slow_guard {
    rails_ctx *c;
    const char *what;
    long long a, b;
    double t0 = 0.0;
    static double limit_ms()
    {
        static const double v = getenv("RAILS_TRACE_SLOW_MS") ? atof(getenv("RAILS_TRACE_SLOW_MS")) : 0.0;
        return v;
    }
    static double now()
    {
        timespec ts;
        clock_gettime(CLOCK_MONOTONIC, &ts);
        return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
    }
    rails_slow_guard(rails_ctx *ctx, const char *w, long long a_ = 0, long long b_ = 0) : c(ctx), what(w), a(a_), b(b_)
    {
        if (limit_ms() > 0.0 && c) {
            hipStreamSynchronize(c->stream);
            t0 = now();
        }
    }
    ~rails_slow_guard()
    {
        if (limit_ms() > 0.0 && c) {
            hipStreamSynchronize(c->stream);
            const double dt = now() - t0;
            if (dt > limit_ms()) fprintf(stderr, "[rails slow] %s(%lld, %lld): %.2f ms\n", what, a, b, dt);
        }
    }
};

// integer environment switch (the RAILS_SPMM_* of the SpMM sources)
inline int spmm_env(const char *name, int def)
{
    const char *e = getenv(name);
    return e ? atoi(e) : def;
}

// ---- helpers implemented in ctx.hip ----
int rails_ws_reserve(rails_ctx *ctx, size_t bytes);
int rails_small_reserve(rails_ctx *ctx, size_t bytes);
int rails_pinned_reserve(rails_ctx *ctx, size_t bytes);
// host -> pinned -> device staging without a stream synchronisation: begin_write waits until the previous upload out of the
// pinned buffer has been consumed (and reserves), end_write marks the upload just enqueued
int rails_pinned_begin_write(rails_ctx *ctx, size_t bytes);
int rails_pinned_end_write(rails_ctx *ctx);
int rails_allreduce_dev(rails_ctx *ctx, double *dev, size_t n);
int rails_ctx_second_stream(rails_ctx *ctx); // makes stream2 / ev_fork / ev_join when missing

// rccl_comm.hip
int rails_rccl_allreduce(rails_ctx *c, double *dev, size_t n);
int rails_rccl_halo(rails_ctx *c, const rails_csr *A, const double *send_buf, double *recv_buf, int ncols);
void rails_rccl_release(rails_ctx *c);

// ---- kernels / launchers across translation units ----
// spmm.hip: the facts op_choice.h decides on, for a product of nc columns between windows of that alignment
struct OpFacts;
OpFacts rails_op_facts(const rails_ctx *c, const rails_csr *A, int nc, bool x_vec2, bool y_vec2);
// spmm.hip: rails_spmm's ghost-row exchange on its own -- pack nc columns of the rows the neighbours need from Xp (row stride ldx), exchange;
// afterwards, in stream order, A->ext holds the ghost rows with row stride nc.  Grows the operator's two buffers as rails_spmm does.
int rails_halo_exchange(rails_ctx *c, rails_csr *A, const double *Xp, int ldx, int nc);
// spmm_sweep.hip: the sweep kernel for banded patterns; *done tells whether it computed the product
int rails_spmm_sweep(rails_ctx *c, rails_csr *A, const double *X, int ldx, const double *Xg, int ldg, double *Y, int ldy, int nc, bool aligned,
                     bool force, bool *done);
int rails_sweep_prepare(rails_ctx *c, rails_csr *A, int nc, bool *fits); // the schedule for nc columns, now
void rails_sweep_release(rails_csr *A);
// the interior rows of a row-partitioned operator as a sweep of their own (on stream st, beside the halo exchange); aligned: X and Y rows
// 16-byte aligned
int rails_spmm_sweep_interior(rails_ctx *c, rails_csr *A, const double *X, int ldx, double *Y, int ldy, int nc, bool aligned, hipStream_t st, bool *done);
int rails_sweep_prepare_interior(rails_ctx *c, rails_csr *A, int nc, bool *fits);
// spmm_planes.hip: the plane-sweep kernel for structured-grid stencils; *done tells whether it computed the product
int rails_spmm_planes(rails_ctx *c, rails_csr *A, const double *X, int ldx, double *Y, int ldy, int nc, bool aligned, bool build, bool *done);
void rails_planes_release(rails_csr *A);
// the interior planes of a z-slab of a grid stencil (rows without ghost columns) on stream st; *done = false: not that kind of operator
int rails_spmm_planes_interior(rails_ctx *c, rails_csr *A, const double *X, int ldx, double *Y, int ldy, int nc, bool aligned, hipStream_t st, bool *done);
bool planes_last_interior(const rails_csr *A);
// spmm_tiled.hip: the LDS-staged footprint kernels over the tile plan of tile_plan.h (which also has the grid detection); *done
// tells whether they computed the product.  x_room: columns of the padded X row from the window's first one on
int rails_spmm_tiled(rails_ctx *c, rails_csr *A, const double *X, int ldx, const double *Xg, int ldg, double *Y, int ldy, int nc, bool vec2,
                     int x_room, bool *done);
void rails_tiled_release(rails_csr *A);
// spmm_bsr.hip: the product of a block-CSR handle (windows checked, nc >= 1), and the release of its matrix with the handle
int rails_bsr_apply(rails_ctx *c, rails_csr *A, int trans, const rails_panel *X, int xc0, int nc, rails_panel *Y, int yc0);
void rails_bsr_release(rails_csr *A);
// ... and the host copy the handle keeps: block size, block rows, the three arrays (false: not a block-CSR handle)
bool rails_bsr_host_arrays(const rails_csr *A, int *b, int64_t *mb, const int64_t **browptr, const int32_t **bcol, const double **bval);
// ... and its device arrays with the block rows and the longest block row (false: not a block-CSR handle)
bool rails_bsr_device_arrays(const rails_csr *A, int64_t *mb, int64_t *max_brow, const int64_t **browptr, const int32_t **bcol, const double **bval);
// dense_gram.hip: partial Gram into device memory (no host copy / all-reduce): C_dev (a x b col-major, ldc = a)
int rails_gram_dev(rails_ctx *ctx, const double *X, int ldx, const double *Y, int ldy, int64_t m, int a, int b,
                   double *C_dev);
// dense_gemm.hip: Y = beta Y + alpha X C with C on the device (k x r, packed)
int rails_panel_gemm_dev(rails_ctx *ctx, double alpha, const double *X, int ldx, int k, const double *C_dev,
                         int r, double beta, double *Y, int ldy, int64_t m);
// dense_gram.hip: local column sums of squares of nc <= 512 columns into device memory (no all-reduce, no host copy)
int rails_colnorms2_dev(rails_ctx *ctx, const double *X, int ldx, int64_t m, int nc, double *out_dev);
// the same with the left operand in two panels, [X1 X2] with a1 + a2 columns (b, r <= 32; Y += alpha [X1 X2] C)
int rails_gram2_dev(rails_ctx *ctx, const double *X1, int ldx1, int a1, const double *X2, int ldx2, int a2, const double *Y, int ldy, int64_t m,
                    int b, double *C_dev);
int rails_panel_gemm2_dev(rails_ctx *ctx, double alpha, const double *X1, int ldx1, int a1, const double *X2, int ldx2, int a2,
                          const double *C_dev, int r, double *Y, int ldy, int64_t m);

#endif
