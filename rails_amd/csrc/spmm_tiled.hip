// spmm_tiled.hip -- the LDS-staged footprint kernels of Y = A X (k_spmm_tiled, k_spmm_tiled_pipe, k_spmm_tiled_reg) for gfx950.
//
// Kernel 2 of the product `A_ * W` (src/LyapunovSolver.hpp:146; the row kernels and the dispatcher are in spmm.hip).  Rows are grouped
// into tiles on the host (tile_plan.h / tile_plan.cpp: runs of consecutive rows, or boxes of a structured grid).  A workgroup owns one
// tile: it copies the tile's CSR block into LDS once, then per chunk of KC columns stages footprint x KC doubles of X in LDS (coalesced
// 64/128-B row segments) and every row of the tile accumulates from LDS.  Each X row segment crosses the L2->CU fabric once per tile
// instead of once per nonzero, and the inner loop has no global loads.
#include "rails_internal.h"
#include "tile_plan.h"

#include <algorithm>

// the plan's arrays on the device (tile_plan.h says what they hold): passed to the kernels by value.  Nine separate allocations that
// the kernels only read: they never alias each other, X or Y (inside a struct the pointers cannot carry __restrict__ to say so)
struct TileView {
    const int32_t *t_rowptr, *t_rows, *t_rp, *fp_ptr, *fp;
    const int64_t *t_nzptr;
    const double *t_val;
    const uint16_t *t_lcol, *fpos;
    int64_t m, ntiles;
};

// device side of an operator's tile plan, made by the first product that asks for it (rails_csr::tiled)
struct rails_tile_cache {
    bool ok = false; // the plan was worthwhile and fits: v holds it
    TileView v = {};
    int max_fp = 0, max_nz = 0, max_pos = 0, tile_rows = 0;
    double reuse = 0.0;
    bool grid = false;
    // the most recent launch (rails_csr_tile_stats): kernel 1 = k_spmm_tiled, 2 = k_spmm_tiled_pipe, 3 = k_spmm_tiled_reg
    struct {
        int kernel, kc, nnz, nl, v2, ns;
    } last = {};
};

void rails_tiled_release(rails_csr *A)
{
    if (!A->tiled) return;
    const TileView &v = A->tiled->v;
    for (const void *p : std::initializer_list<const void *>{v.t_rowptr, v.t_rows, v.t_rp, v.fp_ptr, v.fp, v.t_nzptr, v.t_val, v.t_lcol, v.fpos})
        if (p) (void)hipFree(const_cast<void *>(p));
    delete A->tiled;
    A->tiled = nullptr;
}

namespace {

typedef double double2_t __attribute__((ext_vector_type(2)));

// this workgroup's tile: its rows [tr0, tr0 + nrows) of t_rows, nonzeros [z0, z0 + nz), footprint entries [f0, f0 + nf).
// XCD-aware block -> tile map as in the row kernels (spmm.hip); false: a block past the last tile.
struct Tile {
    int64_t t, z0;
    int tr0, nrows, nz, f0, nf;
};
__device__ __forceinline__ bool tile_of_block(const TileView &tv, int64_t tiles_per_xcd, Tile &h)
{
    h.t = blockIdx.x;
    if (tiles_per_xcd > 0) h.t = (int64_t)(blockIdx.x & 7) * tiles_per_xcd + (blockIdx.x >> 3);
    if (h.t >= tv.ntiles) return false;
    // (all six loads in front of the first difference: issued together, one wait -- a round trip per array otherwise)
    const int tr0 = tv.t_rowptr[h.t], tr1 = tv.t_rowptr[h.t + 1], f0 = tv.fp_ptr[h.t], f1 = tv.fp_ptr[h.t + 1];
    const int64_t z0 = tv.t_nzptr[h.t], z1 = tv.t_nzptr[h.t + 1];
    h.tr0 = tr0, h.nrows = tr1 - tr0, h.z0 = z0, h.nz = (int)(z1 - z0), h.f0 = f0, h.nf = f1 - f0;
    return true;
}

// the tile's CSR block into LDS: values, LDS rows of their X rows, nrows + 1 row offsets
__device__ __forceinline__ void tile_csr_to_lds(const TileView &tv, const Tile &h, double *vals, uint16_t *lcols, int32_t *rp)
{
    for (int i = threadIdx.x; i < h.nz; i += 256) {
        vals[i] = tv.t_val[h.z0 + i];
        lcols[i] = tv.t_lcol[h.z0 + i];
    }
    for (int i = threadIdx.x; i <= h.nrows; i += 256) rp[i] = tv.t_rp[h.tr0 + h.t + i];
}

// columns [cidx, cidx + 2) of every row of the tile from the chunk staged in Xs: KC/2 lanes per row
template <int KC>
__device__ __forceinline__ void tile_rows_from_lds(const TileView &tv, const Tile &h, const double *vals, const uint16_t *lcols, const int32_t *rp,
                                                   const double *Xs, double *Y, int ldy, int cidx, int nc)
{
    constexpr int LPR = KC / 2;    // lanes per row, 2 doubles (16 B) each
    constexpr int RPP = 256 / LPR; // rows per pass of the workgroup
    const int part = threadIdx.x % LPR;
    for (int i = threadIdx.x / LPR; i < h.nrows; i += RPP) {
        const int p0 = rp[i], p1 = rp[i + 1];
        double2_t acc = (double2_t){0.0, 0.0};
        int p = p0;
        for (; p + 4 <= p1; p += 4) {
            double a[4];
            int lc[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                a[u] = vals[p + u];
                lc[u] = lcols[p + u];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const double2_t x = *reinterpret_cast<const double2_t *>(&Xs[lc[u] * KC + 2 * part]);
                acc.x = __builtin_fma(a[u], x.x, acc.x);
                acc.y = __builtin_fma(a[u], x.y, acc.y);
            }
        }
        for (; p < p1; ++p) {
            const double a = vals[p];
            const double2_t x = *reinterpret_cast<const double2_t *>(&Xs[(int)lcols[p] * KC + 2 * part]);
            acc.x = __builtin_fma(a, x.x, acc.x);
            acc.y = __builtin_fma(a, x.y, acc.y);
        }
        double *dst = Y + (int64_t)tv.t_rows[h.tr0 + i] * ldy + cidx;
        if (cidx + 1 < nc)
            *reinterpret_cast<double2_t *>(dst) = acc;
        else if (cidx < nc)
            *dst = acc.x;
    }
}

template <int KC>
__global__ __launch_bounds__(256) void k_spmm_tiled(TileView tv, const double *__restrict__ X, int ldx, const double *__restrict__ Xg, int ldg,
                                                    double *__restrict__ Y, int ldy, int nc, int64_t tiles_per_xcd, int nz_cap, int xs_doubles)
{
    extern __shared__ double smem[];
    constexpr int LPR = KC / 2;
    Tile h;
    if (!tile_of_block(tv, tiles_per_xcd, h)) return;
    // LDS carve-up (all 8-byte aligned): vals[nz_cap] | Xs[xs_doubles] | rp[264] (int32) | lcols[nz_cap] (uint16)
    double *vals = smem;
    double *Xs = vals + nz_cap;
    int32_t *rp = reinterpret_cast<int32_t *>(Xs + xs_doubles);
    uint16_t *lcols = reinterpret_cast<uint16_t *>(rp + 264);
    const int tid = threadIdx.x;
    const int part = tid % LPR;

    tile_csr_to_lds(tv, h, vals, lcols, rp);
    __syncthreads();

    for (int c0 = 0; c0 < nc; c0 += KC) {
        const int cidx = c0 + 2 * part;
        for (int idx = tid; idx < h.nf * LPR; idx += 256) {
            const int f = idx / LPR;
            const int32_t c = tv.fp[h.f0 + f];
            const double *src = (c < tv.m) ? (X + (int64_t)c * ldx) : (Xg + ((int64_t)c - tv.m) * ldg);
            double2_t v = (double2_t){0.0, 0.0};
            if (cidx + 1 < nc)
                v = *reinterpret_cast<const double2_t *>(src + cidx);
            else if (cidx < nc)
                v.x = src[cidx];
            *reinterpret_cast<double2_t *>(&Xs[(int)tv.fpos[h.f0 + f] * KC + 2 * part]) = v;
        }
        __syncthreads();
        tile_rows_from_lds<KC>(tv, h, vals, lcols, rp, Xs, Y, ldy, cidx, nc);
        __syncthreads();
    }
}

// Pipelined form of k_spmm_tiled: every thread keeps the source pointers of its NL staging slots in registers (the
// footprint is the same for every column chunk), the loads of chunk c+1 are in flight while chunk c is consumed from
// the other LDS buffer, one barrier per chunk.
template <int KC, int NL>
__global__ __launch_bounds__(256) void k_spmm_tiled_pipe(TileView tv, const double *__restrict__ X, int ldx, const double *__restrict__ Xg, int ldg,
                                                         double *__restrict__ Y, int ldy, int nc, int64_t tiles_per_xcd, int nz_cap, int xs_doubles)
{
    extern __shared__ double smem[];
    constexpr int LPR = KC / 2;
    Tile h;
    if (!tile_of_block(tv, tiles_per_xcd, h)) return;
    // LDS: vals[nz_cap] | Xs0[xs_doubles] | Xs1[xs_doubles] | rp[264] (int32) | lcols[nz_cap] (uint16)
    double *vals = smem;
    double *Xs0 = vals + nz_cap;
    int32_t *rp = reinterpret_cast<int32_t *>(Xs0 + 2 * (size_t)xs_doubles);
    uint16_t *lcols = reinterpret_cast<uint16_t *>(rp + 264);
    const int tid = threadIdx.x;
    const int part = tid % LPR;

    const double *srcp[NL];
    int dsto[NL];
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        const int idx = tid + 256 * i;
        srcp[i] = nullptr;
        dsto[i] = 0;
        if (idx < h.nf * LPR) {
            const int f = idx / LPR;
            const int32_t c = tv.fp[h.f0 + f];
            srcp[i] = ((c < tv.m) ? (X + (int64_t)c * ldx) : (Xg + ((int64_t)c - tv.m) * ldg)) + 2 * part;
            dsto[i] = (int)tv.fpos[h.f0 + f] * KC + 2 * part;
        }
    }
    // D column chunks are in flight in registers; chunk ci is written to LDS buffer (ci & 1) just before it is
    // consumed, and its register slot is refilled with chunk ci + D.  One barrier per chunk.
    constexpr int D = 4;
    double2_t stage[D][NL];
    const int nchunks = (nc + KC - 1) / KC;
#define RAILS_LOAD_CHUNK(SLOT, CI)                                                              \
    do {                                                                                        \
        const int c0__ = (CI)*KC;                                                               \
        const int cidx__ = c0__ + 2 * part;                                                     \
        _Pragma("unroll") for (int i = 0; i < NL; ++i)                                          \
        {                                                                                       \
            stage[SLOT][i] = (double2_t){0.0, 0.0};                                             \
            if (srcp[i]) {                                                                      \
                if (cidx__ + 1 < nc)                                                            \
                    stage[SLOT][i] = *reinterpret_cast<const double2_t *>(srcp[i] + c0__);      \
                else if (cidx__ < nc)                                                           \
                    stage[SLOT][i].x = srcp[i][c0__];                                           \
            }                                                                                   \
        }                                                                                       \
    } while (0)

#pragma unroll
    for (int d = 0; d < D; ++d)
        if (d < nchunks) RAILS_LOAD_CHUNK(d, d);
    tile_csr_to_lds(tv, h, vals, lcols, rp);

    for (int cbase = 0; cbase < nchunks; cbase += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int ci = cbase + d;
            if (ci < nchunks) {
                double *Xs = Xs0 + (size_t)(ci & 1) * xs_doubles;
#pragma unroll
                for (int i = 0; i < NL; ++i)
                    if (srcp[i]) *reinterpret_cast<double2_t *>(&Xs[dsto[i]]) = stage[d][i];
                if (ci + D < nchunks) RAILS_LOAD_CHUNK(d, ci + D);
                __syncthreads();
                tile_rows_from_lds<KC>(tv, h, vals, lcols, rp, Xs, Y, ldy, ci * KC + 2 * part, nc);
            }
        }
    }
#undef RAILS_LOAD_CHUNK
}

// Register-resident form: one tile row per slot of KC/2 lanes; the row's (val, footprint index) pairs are loaded
// into registers once per tile and reused for every column chunk, so the inner loop is ONE ds_read_b128 + 2 FMA per
// nonzero (the LDS-resident forms above spend three LDS reads per nonzero and are LDS-issue bound).  X chunks are
// double-buffered in LDS, the next chunk's global loads are in flight during the current chunk's arithmetic.
//
// V2 = double2 vectors per lane: V2 = 1 gives KC/2 lanes per row (KC = 8: 4 lanes x 16 B); V2 = 2 with KC = 16 keeps 4 lanes
// per row (64-row tiles) with 32 B per lane, i.e. whole 128-B lines per staged X row, twice the bytes in flight per
// workgroup at the same register cost for the row's CSR, and half as many barrier phases.  The two 64-B halves of an LDS
// row are swapped when bit 1 of the row position is set, so the four x-consecutive row slots a 16-lane group of a
// ds_read_b128 serves still fall into four different bank quarters.
// NS = column chunks in flight in registers per thread (2, or 1 where the registers do not allow two).
template <int KC, int NNZ, int NL, int V2, int NS>
__global__ __launch_bounds__(256) void k_spmm_tiled_reg(TileView tv, const double *__restrict__ X, int ldx, const double *__restrict__ Xg, int ldg,
                                                        double *__restrict__ Y, int ldy, int nc, int64_t tiles_per_xcd, int xs_doubles)
{
    // Every global load in this kernel is UNCONDITIONAL (clamped indices, duplicate staging slots, full-width chunks
    // guaranteed by the host): a load under a lane-dependent branch makes hipcc wait vmcnt(0) at the join, which
    // serialises the staging loads into dependent round trips (measured: 4 us per 14-KB chunk).
    extern __shared__ double smem[];
    constexpr int LPR = KC / (2 * V2); // compute lanes per row
    constexpr int SPR = KC / 2;        // 16-byte staging pieces per row
    static_assert(V2 == 1 || (V2 == 2 && KC == 16), "supported: one double2 per lane, or two with 16-column chunks");
    Tile h;
    if (!tile_of_block(tv, tiles_per_xcd, h)) return;
    const int64_t m = tv.m;
    const int tid = threadIdx.x;
    const int part = tid % LPR;
    const int slot = tid / LPR;
    const bool has_row = slot < h.nrows;
    const int rslot = has_row ? slot : 0; // idle slots shadow row 0 of the tile (never stored)

    // this slot's row: values and LDS offsets of its X rows, padded to NNZ entries with zero coefficients that alias
    // the row's own first entry (a non-finite value in an unrelated X row can never leak in)
    double a[NNZ];
    unsigned xo2[(NNZ + 1) / 2]; // two 16-bit LDS offsets (in doubles) per register: keeps the kernel at <= 128 VGPRs
    const int p0 = tv.t_rp[h.tr0 + h.t + rslot];
    const int cnt = tv.t_rp[h.tr0 + h.t + rslot + 1] - p0;
    {
        const int64_t base = h.z0 + p0;
        const int last = cnt > 0 ? cnt - 1 : 0;
#pragma unroll
        for (int u = 0; u < NNZ; ++u) {
            const int uu = u < last ? u : last;
            const double av = tv.t_val[base + uu];
            const unsigned lp = (unsigned)tv.t_lcol[base + uu];
            const unsigned off = lp * KC + 2 * part + (V2 == 2 ? ((lp >> 1) & 1u) * 8u : 0u); // vector 0; vector 1 is off ^ 8
            a[u] = (u < cnt) ? av : 0.0;
            if (u & 1)
                xo2[u / 2] |= off << 16;
            else
                xo2[u / 2] = off;
        }
    }
    const int64_t yrow = (int64_t)tv.t_rows[h.tr0 + rslot];

    // staging slots: slot indices past the footprint duplicate footprint row 0 (same bytes to the same LDS address).
    // Sources are kept as 32-bit element offsets (top bit: ghost buffer) and LDS targets as packed 16-bit offsets to
    // stay within the register budget of 3 waves per SIMD.
    unsigned soff[NL];
    unsigned dst2[(NL + 1) / 2];
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        int idx = tid + 256 * i;
        int f = idx / SPR;
        const int q = idx % SPR;
        f = f < h.nf ? f : 0;
        const int32_t c = tv.fp[h.f0 + f];
        const unsigned ghost = (c < m) ? 0u : 0x80000000u;
        const unsigned eo = ghost ? (unsigned)((int64_t)(c - m) * ldg) : (unsigned)((int64_t)c * ldx);
        soff[i] = (eo + 2 * q) | ghost;
        const unsigned lp = (unsigned)tv.fpos[h.f0 + f];
        const unsigned d = lp * KC + (V2 == 2 ? (((unsigned)(q / 4) ^ ((lp >> 1) & 1u)) * 8u + 2u * (q % 4)) : 2u * q);
        if (i & 1)
            dst2[i / 2] |= d << 16;
        else
            dst2[i / 2] = d;
    }
#define RAILS_SRC(i) (((soff[i] & 0x80000000u) ? Xg : X) + (soff[i] & 0x7fffffffu))
#define RAILS_DST(i) (((i)&1) ? (dst2[(i) / 2] >> 16) : (dst2[(i) / 2] & 0xffffu))
    // Two column chunks are in flight in registers per thread (Little's law: with one chunk in flight the kernel is bound
    // by bytes-in-flight x latency, ~41 KB per CU); chunk ci goes to LDS buffer (ci & 1) right before use and its
    // register set is refilled with chunk ci + 2.  Loads past the last chunk are clamped to it (unused).
    double2_t stage0[NL], stage1[NL], stage2[NL];
    const int nchunks = (nc + KC - 1) / KC;
    const int lastc = (nchunks - 1) * KC;
#pragma unroll
    for (int i = 0; i < NL; ++i) stage0[i] = *reinterpret_cast<const double2_t *>(RAILS_SRC(i));
    if (NS >= 2) {
        const int c1 = KC < lastc ? KC : lastc;
#pragma unroll
        for (int i = 0; i < NL; ++i) stage1[i] = *reinterpret_cast<const double2_t *>(RAILS_SRC(i) + c1);
    }
    if (NS >= 3) {
        const int c2 = 2 * KC < lastc ? 2 * KC : lastc;
#pragma unroll
        for (int i = 0; i < NL; ++i) stage2[i] = *reinterpret_cast<const double2_t *>(RAILS_SRC(i) + c2);
    }
#define RAILS_TILE_STEP(STAGE, CI)                                                                      \
    do {                                                                                                \
        const int ci__ = (CI);                                                                          \
        double *Xs = smem + (size_t)(ci__ & 1) * xs_doubles;                                            \
        _Pragma("unroll") for (int i = 0; i < NL; ++i) *reinterpret_cast<double2_t *>(&Xs[RAILS_DST(i)]) = STAGE[i]; \
        const int cn__ = (ci__ + NS) * KC < lastc ? (ci__ + NS) * KC : lastc;                           \
        _Pragma("unroll") for (int i = 0; i < NL; ++i) STAGE[i] = *reinterpret_cast<const double2_t *>(RAILS_SRC(i) + cn__); \
        __syncthreads();                                                                                \
        double2_t acc[V2];                                                                              \
        _Pragma("unroll") for (int v = 0; v < V2; ++v) acc[v] = (double2_t){0.0, 0.0};                  \
        _Pragma("unroll") for (int u = 0; u < NNZ; ++u)                                                 \
        {                                                                                               \
            const unsigned off = (u & 1) ? (xo2[u / 2] >> 16) : (xo2[u / 2] & 0xffffu);                 \
            _Pragma("unroll") for (int v = 0; v < V2; ++v)                                              \
            {                                                                                           \
                const double2_t x = *reinterpret_cast<const double2_t *>(&Xs[v ? (off ^ 8u) : off]);    \
                acc[v].x = __builtin_fma(a[u], x.x, acc[v].x);                                          \
                acc[v].y = __builtin_fma(a[u], x.y, acc[v].y);                                          \
            }                                                                                           \
        }                                                                                               \
        _Pragma("unroll") for (int v = 0; v < V2; ++v)                                                  \
        {                                                                                               \
            const int cidx = ci__ * KC + v * 2 * LPR + 2 * part;                                        \
            if (cnt == 0) acc[v] = (double2_t){0.0, 0.0};                                               \
            if (has_row) {                                                                              \
                double *dst = Y + yrow * ldy + cidx;                                                    \
                if (cidx + 1 < nc)                                                                      \
                    *reinterpret_cast<double2_t *>(dst) = acc[v];                                       \
                else if (cidx < nc)                                                                     \
                    *dst = acc[v].x;                                                                    \
            }                                                                                           \
        }                                                                                               \
    } while (0)
    if (NS == 3) {
        for (int ci = 0; ci < nchunks; ci += 3) {
            RAILS_TILE_STEP(stage0, ci);
            if (ci + 1 < nchunks) RAILS_TILE_STEP(stage1, ci + 1);
            if (ci + 2 < nchunks) RAILS_TILE_STEP(stage2, ci + 2);
        }
    } else if (NS == 2) {
        for (int ci = 0; ci < nchunks; ci += 2) {
            RAILS_TILE_STEP(stage0, ci);
            if (ci + 1 < nchunks) RAILS_TILE_STEP(stage1, ci + 1);
        }
    } else {
        for (int ci = 0; ci < nchunks; ++ci) RAILS_TILE_STEP(stage0, ci);
    }
#undef RAILS_TILE_STEP
#undef RAILS_SRC
#undef RAILS_DST
}

template <class T>
int upload(const T **dst, const std::vector<T> &src)
{
    size_t n = src.empty() ? 1 : src.size();
    T *d = nullptr;
    RAILS_HIP_CHECK(hipMalloc((void **)&d, n * sizeof(T)));
    *dst = d;
    if (!src.empty()) RAILS_HIP_CHECK(hipMemcpy(d, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return RAILS_OK;
}

// the operator's plan: built and uploaded by the first product that gets here (T->ok: worthwhile and fits)
int ensure_tile_cache(rails_csr *A, int kc)
{
    if (A->tiled) return RAILS_OK;
    rails_tile_cache *T = A->tiled = new rails_tile_cache();
    static const int env_rows = spmm_env("RAILS_SPMM_TILE_ROWS", 64), env_box = spmm_env("RAILS_SPMM_TILE_BOX", 1),
                     env_morton = spmm_env("RAILS_SPMM_TILE_MORTON", 1);
    const rails_tile_params prm = {env_rows, env_box != 0, env_morton != 0, kc};
    rails_tile_plan P;
    if (!rails_tile_plan_build(prm, A->m, A->h_rowptr.data(), A->h_col.data(), A->h_val.data(), A->max_row_nnz, P)) return RAILS_OK;
    TileView &v = T->v;
    v.m = A->m;
    v.ntiles = P.n_tiles;
    RAILS_TRY(upload(&v.t_rowptr, P.t_rowptr));
    RAILS_TRY(upload(&v.t_rows, P.t_rows));
    RAILS_TRY(upload(&v.t_nzptr, P.t_nzptr));
    RAILS_TRY(upload(&v.t_rp, P.t_rp));
    RAILS_TRY(upload(&v.t_val, P.t_val));
    RAILS_TRY(upload(&v.t_lcol, P.t_lcol));
    RAILS_TRY(upload(&v.fp_ptr, P.fp_ptr));
    RAILS_TRY(upload(&v.fp, P.fp));
    RAILS_TRY(upload(&v.fpos, P.fp_pos));
    T->max_fp = P.max_fp;
    T->max_nz = P.max_nz;
    T->max_pos = P.max_pos;
    T->tile_rows = P.max_rows;
    T->reuse = P.reuse;
    T->grid = P.grid;
    T->ok = true;
    return RAILS_OK;
}

// one product on the context's stream: what every launch below passes on
struct TileLaunch {
    rails_ctx *c;
    rails_tile_cache *T;
    const double *X, *Xg;
    double *Y;
    int ldx, ldg, ldy, nc;
    unsigned grid;
    int64_t tpx; // tiles per XCD (0: blocks in tile order)
};

template <int KC, int NNZ, int NL, int V2, int NS>
int launch_reg(const TileLaunch &L)
{
    rails_ctx *c = L.c;
    const int xs = L.T->max_pos * KC;
    const size_t lds = 2 * (size_t)xs * 8;
    RAILS_HIP_CHECK(hipFuncSetAttribute((const void *)k_spmm_tiled_reg<KC, NNZ, NL, V2, NS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    RAILS_LAUNCH((k_spmm_tiled_reg<KC, NNZ, NL, V2, NS>), dim3(L.grid), dim3(256), lds, c->stream, L.T->v, L.X, L.ldx, L.Xg, L.ldg, L.Y, L.ldy, L.nc,
                 L.tpx, xs);
    L.T->last = {3, KC, NNZ, NL, V2, NS};
    return RAILS_OK;
}

// chunks in flight in registers (RAILS_SPMM_TILE_NS, default 2: deeper pipeline at 2 waves/SIMD for long rows; 1: 16 fewer VGPRs,
// 3 waves/SIMD): two unless that needs more than 256 VGPRs (wide chunks with long rows and 8 staging slots)
template <int KC, int NNZ, int NL, int V2>
int launch_reg_ns(const TileLaunch &L, int env_ns)
{
    constexpr bool tight = (V2 == 2 && NNZ * 2 + NL * 8 > 100);
    if (tight || (env_ns == 1 && NNZ > 16)) return launch_reg<KC, NNZ, NL, V2, 1>(L);
    if (env_ns == 3 && V2 == 1 && NL == 4) return launch_reg<KC, NNZ, NL, V2, 3>(L);
    return launch_reg<KC, NNZ, NL, V2, 2>(L);
}

// register slots for the longest row (nnz4 = its entries in fours) and staging slots per thread for the largest footprint
template <int KC, int V2>
int launch_reg_for(const TileLaunch &L, int nnz4, int need_nl, int env_ns)
{
    if (nnz4 <= 2) return need_nl <= 4 ? launch_reg_ns<KC, 8, 4, V2>(L, env_ns) : launch_reg_ns<KC, 8, 8, V2>(L, env_ns);
    if (nnz4 <= 4) return need_nl <= 4 ? launch_reg_ns<KC, 16, 4, V2>(L, env_ns) : launch_reg_ns<KC, 16, 8, V2>(L, env_ns);
    if (nnz4 <= 7) return need_nl <= 4 ? launch_reg_ns<KC, 28, 4, V2>(L, env_ns) : launch_reg_ns<KC, 28, 8, V2>(L, env_ns);
    return need_nl <= 4 ? launch_reg_ns<KC, 32, 4, V2>(L, env_ns) : launch_reg_ns<KC, 32, 8, V2>(L, env_ns);
}

// the two LDS-resident forms (one signature): nl = 0 is k_spmm_tiled, 4 / 8 k_spmm_tiled_pipe with that many staging slots per thread
template <int KC>
int launch_lds(const TileLaunch &L, int nl)
{
    rails_ctx *c = L.c;
    const auto kern = nl == 0 ? k_spmm_tiled<KC> : nl == 4 ? k_spmm_tiled_pipe<KC, 4> : k_spmm_tiled_pipe<KC, 8>;
    const size_t lds = rails_tile_lds_bytes(L.T->max_nz, L.T->max_pos, KC, nl ? 2 : 1);
    RAILS_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    RAILS_LAUNCH(kern, dim3(L.grid), dim3(256), lds, c->stream, L.T->v, L.X, L.ldx, L.Xg, L.ldg, L.Y, L.ldy, L.nc, L.tpx, L.T->max_nz, L.T->max_pos * KC);
    L.T->last = {nl ? 2 : 1, KC, 0, nl, 0, 0};
    return RAILS_OK;
}

} // namespace

extern "C" int rails_csr_tile_stats(rails_csr *A, double *out)
{
    RAILS_REQUIRE(A && out, "rails_csr_tile_stats: null argument");
    for (int i = 0; i < 16; ++i) out[i] = 0.0;
    out[7] = (double)A->max_row_nnz;
    const rails_tile_cache *T = A->tiled;
    if (!T) return RAILS_OK;
    out[0] = 1.0;
    if (T->ok) {
        out[1] = 1.0;
        out[2] = T->grid ? 1.0 : 0.0;
        out[3] = (double)T->v.ntiles;
        out[4] = (double)T->tile_rows;
        out[5] = (double)T->max_fp;
        out[6] = (double)T->max_pos;
        out[8] = T->reuse;
    }
    const int last[6] = {T->last.kernel, T->last.kc, T->last.nnz, T->last.nl, T->last.v2, T->last.ns};
    for (int i = 0; i < 6; ++i) out[9 + i] = (double)last[i];
    return RAILS_OK;
}

int rails_spmm_tiled(rails_ctx *c, rails_csr *A, const double *X, int ldx, const double *Xg, int ldg, double *Y, int ldy, int nc, bool vec2,
                     int x_room, bool *done)
{
    *done = false;
    if (!vec2 || nc < 8 || A->nnz == 0 || A->m >= 0x7fffffffLL) return RAILS_OK;
    // the tile plan costs a host analysis of the whole matrix (~0.45 s per million rows): built on first use by a WIDE product
    // (warm start, the A*V benchmark) or when the kernel is asked for; the narrow in-loop products keep the row-gather kernel
    if (!A->tiled && nc < 64 && A->variant == 0) return RAILS_OK;
    static const int env_kc = spmm_env("RAILS_SPMM_TILE_KC", 8);
    const int KC = (env_kc == 16) ? 16 : 8;
    RAILS_TRY(ensure_tile_cache(A, KC));
    rails_tile_cache *T = A->tiled;
    if (!T->ok) return RAILS_OK;
    TileLaunch L = {c, T, X, Xg, Y, ldx, ldg, ldy, nc, 0u, 0};
    int64_t grid = T->v.ntiles;
    static const int xcd_aware = spmm_env("RAILS_SPMM_XCD", 1);
    if (xcd_aware && grid >= 64) {
        L.tpx = (grid + 7) / 8;
        grid = L.tpx * 8;
    }
    L.grid = (unsigned)grid;
    static const int env_reg = spmm_env("RAILS_SPMM_TILE_REG", 1);
    // the register-resident kernel reads whole KC-column chunks unconditionally: the padded row must have room for the
    // rounded-up last chunk, and ghost rows (stored with ld = nc) must be a whole number of chunks
    const bool full_width_ok = ((nc + KC - 1) / KC * KC <= x_room) && (A->n_ghost == 0 || nc % KC == 0);
    // wide chunks (16 columns, 4 lanes x 32 B per row) for wide panels; narrow panels keep two 8-column chunks in flight
    // (measured on MI355X: not faster than 8-column chunks -- 0.82 vs 0.79 ms on the 27-point stencil at nc = 128; both forms
    // move ~10 B/clk/CU through the load path, which is what bounds this kernel: profiles/r01_spmm_tiled_wide.md -- so it
    // is off unless asked for: operator variant 6 or RAILS_SPMM_TILE_WIDE=1)
    static const int env_wide = spmm_env("RAILS_SPMM_TILE_WIDE", 0);
    static const int env_ns = spmm_env("RAILS_SPMM_TILE_NS", 2);
    const bool wide = (env_wide || A->variant == 6) && nc >= 32 && ((nc + 15) / 16 * 16 <= x_room) && (A->n_ghost == 0 || nc % 16 == 0);
    const int KCr = wide ? 16 : KC, V2r = wide ? 2 : 1;
    const int lpr_r = KCr / (2 * V2r);
    const int need_nl_r = (T->max_fp * (KCr / 2) + 255) / 256;
    const int xs_r = T->max_pos * KCr;
    const size_t lds_reg = 2 * (size_t)xs_r * 8;
    if (env_reg && (wide || full_width_ok) && xs_r < 65536 && (int64_t)A->m * ldx < 0x7fffffffLL && (int64_t)(A->n_ghost + 1) * ldg < 0x7fffffffLL && T->tile_rows <= 256 / lpr_r && A->max_row_nnz <= 32 && need_nl_r <= 8 && lds_reg <= (size_t)RAILS_TILE_LDS_BUDGET) {
        const int nnz4 = (A->max_row_nnz + 3) / 4;
        if (wide)
            RAILS_TRY((launch_reg_for<16, 2>(L, nnz4, need_nl_r, env_ns)));
        else if (KC == 8)
            RAILS_TRY((launch_reg_for<8, 1>(L, nnz4, need_nl_r, env_ns)));
        else
            RAILS_TRY((launch_reg_for<16, 1>(L, nnz4, need_nl_r, env_ns)));
        A->last_kernel = "k_spmm_tiled_reg";
        *done = true;
        return RAILS_OK;
    }
    static const int env_pipe = spmm_env("RAILS_SPMM_TILE_PIPE", 1);
    const int need_nl = (T->max_fp * (KC / 2) + 255) / 256;
    const bool pipe = env_pipe && need_nl <= 8 && rails_tile_lds_bytes(T->max_nz, T->max_pos, KC, 2) <= (size_t)RAILS_TILE_LDS_BUDGET;
    const int nl = !pipe ? 0 : need_nl <= 4 ? 4 : 8;
    RAILS_TRY(KC == 8 ? launch_lds<8>(L, nl) : launch_lds<16>(L, nl));
    A->last_kernel = pipe ? "k_spmm_tiled_pipe" : "k_spmm_tiled";
    *done = true;
    return RAILS_OK;
}
