// dense_deferred.hip -- the chain of a block orthogonalisation on the device without the host in between: small results kept in slots
// of a device arena, and the first update and second projection of a block in one pass over the basis (dense_common.h has what the dense
// files share).
#include "dense_common.h"

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

// the fused pass as update_gram_choice has it: one of the sixteen instantiations
static int launch_update_gram(rails_ctx *c, const dense::UpdateGramChoice &u, double alpha, const double *X, int ldx, int k, const double *C, int r, const double *Y,
                              int ldy, double *Yo, int ldo, int r2, int64_t m)
{
    if (u.pipelined) {
        switch (u.key()) {
#define RAILS_CASE(NBW, NE)                                                                                                                \
    case dense::inst(NBW, NE):                                                                                                             \
        RAILS_LAUNCH((k_update_gram_p<NBW, NE>), dim3(u.grid), dim3(256), 0, c->stream, alpha, X, ldx, k, C, r, Y, ldy, Yo, ldo, r2, m, u.ntiles, c->ws); \
        break;
            RAILS_DENSE_UPDATE_GRAM_TABLE(RAILS_CASE)
#undef RAILS_CASE
        default: RAILS_REQUIRE(false, "rails_update_gram_deferred: no k_update_gram_p<%d, %d>", u.nbw, u.ne);
        }
    } else {
        switch (u.key()) {
#define RAILS_CASE(NBW, NE)                                                                                                                \
    case dense::inst(NBW, NE):                                                                                                             \
        RAILS_LAUNCH((k_update_gram<NBW, NE>), dim3(u.grid), dim3(256), 0, c->stream, alpha, X, ldx, k, C, r, Y, ldy, Yo, ldo, r2, m, u.ntiles, c->ws); \
        break;
            RAILS_DENSE_UPDATE_GRAM_TABLE(RAILS_CASE)
#undef RAILS_CASE
        default: RAILS_REQUIRE(false, "rails_update_gram_deferred: no k_update_gram<%d, %d>", u.nbw, u.ne);
        }
    }
    c->last_update_gram_form = u.pipelined ? 2 : 1;
    c->last_update_gram_nbw = u.nbw;
    return RAILS_OK;
}

DenseSwitch g_dense_update_gram_pipeline{"RAILS_UPDATE_GRAM_PIPELINE", 1};

extern "C" void rails_dense_set_update_gram_pipeline(int on) { g_dense_update_gram_pipeline.set(on); }

extern "C" int rails_dense_update_gram_pipeline(void) { return g_dense_update_gram_pipeline.get() ? 1 : 0; }

extern "C" int rails_dense_last_update_gram_form(const rails_ctx *c, int *form)
{
    RAILS_REQUIRE(c && form, "rails_dense_last_update_gram_form: null argument");
    *form = c->last_update_gram_form;
    return RAILS_OK;
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
        RAILS_TRY(upload_coefficients(c, C_host, ldc, k, r));
        dense::DenseSwitches sw;
        static const int fused_env = spmm_env("RAILS_FUSED_UPDATE_GRAM", 1);
        sw.fused_update_gram = fused_env;
        sw.tile_fit = g_dense_tile_fit.get();
        sw.update_gram_pipeline = g_dense_update_gram_pipeline.get();
        sw.num_cu = c->num_cu;
        const double *Xp = X->d + xc0;
        const double *Ypp = Y->d + yc0;
        double *Yop = Yout->d + oc0;
        // (16-byte loads of four columns at a time: aligned rows, and the columns between k and k rounded up to 4 are Y's own)
        const int k4 = (k + 3) & ~3;
        const bool rows_ok = dense::rows_vec_ok(Xp, X->ld) && (k4 == k || (X->d == Y->d && yc0 == xc0 + k && r >= k4 - k));
        const dense::UpdateGramChoice u = dense::update_gram_choice(X->m, k, r, r2, rows_ok, sw);
        if (u.fused) {
            RAILS_TRY(rails_ws_reserve(c, (size_t)u.grid * n * sizeof(double)));
            RAILS_TRY(launch_update_gram(c, u, alpha, Xp, X->ld, k, c->small, r, Ypp, Y->ld, Yop, Yout->ld, r2, X->m));
            RAILS_TRY(rails_reduce_partials(c, c->ws, (int64_t)u.grid, (int64_t)n, out));
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
