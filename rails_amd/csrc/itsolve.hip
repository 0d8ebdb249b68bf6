// itsolve.hip -- A^-1 X (or A^-T X) by an iteration that stays on the device, as a library object: the approximate inverse the reference
// allows for its inverse and extended Krylov projections (matlab/RAILSsolver.m:19-23, opts.Ainv: "This can be approximate") where a
// sparse LU (splu.hip) is latency-bound or cannot be formed at all.  Conjugate gradients for a definite operator of either sign,
// BiCGStab (right-preconditioned) for a general one, both with an optional Jacobi preconditioner; conjugate gradients also with a
// Chebyshev polynomial in the Jacobi-scaled operator ("poly_degree", cheb_coef.h), whose steps -- a product and its
// recurrence update -- are one kernel each for a stored CSR operator (k_cheb_step_csr); or, instead, with one V-cycle of smoothed-
// aggregation multigrid ("amg", amg_host.h for the set-up on the host, Run::vcycle below) that smooths with the
// same kernels and adds three of its own (k_amg_residual_csr, k_amg_prolong_add, k_amg_coarse_dense).
//
// Every column is a system of its own with its own scalars (rails_iter_col, iter_scalars.h) in a device block the object owns: no block
// method, no small matrix on the host.  The iteration runs on work panels of the object (ordinary panels, window at column 0, so the
// SpMM kernels see the layout they are tested on and the passes below always load 16 bytes); X's window is copied in, the result copied
// out.  Solves of more than RAILS_ITER_GROUP columns run in groups.  The host queues `check_every` iterations, reads one number back
// through pinned memory (how many columns are still active) and stops when that is zero or max_iterations have been queued; a column
// that has stopped gets zero coefficients from the scalar step, so what is queued after it leaves its x alone and the result does not
// depend on check_every.
//
// Passes: thread (tx, ty) of a block owns the column pair 2 tx, 2 tx + 1 and every TY-th row of its block's slab (k_colnorms2's shape,
// dense.hip), adds its rows in increasing order, the TY row classes meet in an LDS tree of fixed shape, the per-block partial sums go to
// the context workspace, and the one-workgroup kernel k_iter_scalars sums them over the blocks in a fixed order (iter_reduce) and then
// computes the scalars (iter_compute).  No floating-point atomics: two runs give the same bits.
//
// On a context that reduces (more than one rank, an all-reduce hook, a communicator) the two device functions are two kernels with an
// all-reduce of the sums between them (k_iter_reduce, rails_allreduce_dev, k_iter_compute): every rank holds the same scalars bit for bit,
// so every rank queues the same iterations and issues the same collectives.  A is then a row block with its ghost-row plan; the products
// exchange ghost rows inside rails_spmm, the fused polynomial step in its ghost-row form behind an exchange of the object's own.  What
// the ranks must agree on when the object is made is iter_agree.h.  DESIGN.md section 14, "On a row partition".
#include "rails_internal.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>

#include "amg_host.h"
#include "cheb_coef.h"
#include "iter_agree.h"
#include "iter_scalars.h"

namespace {

constexpr int RAILS_ITER_GROUP = 32; // columns per group: the widest panel every SpMM kernel takes in one chunk
// default of "poly_ratio" (hi / lo): the smallest worst case of products relative to plain CG over the table of DESIGN.md section 15
constexpr double RAILS_ITER_POLY_RATIO = 10.0;

typedef double it_v2 __attribute__((ext_vector_type(2)));

struct PassGeom {
    int ncw;     // columns of the group
    int ld;      // row stride of every work panel
    int tx_bits; // TX = 1 << tx_bits threads along the column pairs, TY = 256 / TX along the rows
    int64_t m, rows_per_slab;
};

enum { STEP_CG_INIT = 0, STEP_CG_ALPHA, STEP_CG_BETA, STEP_BI_INIT, STEP_BI_ALPHA, STEP_BI_OMEGA, STEP_BI_END };

__device__ __forceinline__ it_v2 ld2(const double *p) { return *reinterpret_cast<const it_v2 *>(p); }
__device__ __forceinline__ void st2(double *p, it_v2 v, bool has1)
{
    if (has1)
        *reinterpret_cast<it_v2 *>(p) = v;
    else
        p[0] = v.x; // the last column of an odd width: its neighbour is padding and stays as it is
}
// y + a x where a != 0, y itself where a == 0 (a stopped column: not even a non-finite x may reach y)
__device__ __forceinline__ it_v2 axpy_sel(it_v2 a, it_v2 x, it_v2 y)
{
    it_v2 o;
    o.x = a.x != 0.0 ? fma(a.x, x.x, y.x) : y.x;
    o.y = a.y != 0.0 ? fma(a.y, x.y, y.y) : y.y;
    return o;
}

// The shape every pass shares.  body(row, offset of the pair in a work panel, has1, acc) streams one row of one column pair and adds to
// acc[0 .. NQ); the partial sums of block b land in partial[(b * NQ + q) * ncw + column].
template <int NQ, class Body>
__device__ __forceinline__ void iter_pass(const PassGeom &g, double *__restrict__ partial, Body body)
{
    __shared__ double sh[NQ > 0 ? NQ : 1][256][2];
    const int TX = 1 << g.tx_bits, TY = 256 >> g.tx_bits;
    const int tx = threadIdx.x & (TX - 1), ty = threadIdx.x >> g.tx_bits;
    const int c = 2 * tx;
    const bool has0 = c < g.ncw, has1 = c + 1 < g.ncw;
    const int64_t r_begin = (int64_t)blockIdx.x * g.rows_per_slab;
    const int64_t r_end = r_begin + g.rows_per_slab < g.m ? r_begin + g.rows_per_slab : g.m;
    it_v2 acc[NQ > 0 ? NQ : 1];
#pragma unroll
    for (int q = 0; q < (NQ > 0 ? NQ : 1); ++q) acc[q] = (it_v2){0.0, 0.0};
    if (has0) {
#pragma unroll 4
        for (int64_t r = r_begin + ty; r < r_end; r += TY) body(r, r * g.ld + c, has1, acc);
    }
    if (NQ == 0) return;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        sh[q][threadIdx.x][0] = acc[q].x;
        sh[q][threadIdx.x][1] = acc[q].y;
    }
    __syncthreads();
    for (int half = TY >> 1; half > 0; half >>= 1) { // row class ty += row class ty + half: a tree of fixed shape
        if (ty < half) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                sh[q][threadIdx.x][0] += sh[q][threadIdx.x + (half << g.tx_bits)][0];
                sh[q][threadIdx.x][1] += sh[q][threadIdx.x + (half << g.tx_bits)][1];
            }
        }
        __syncthreads();
    }
    if (ty == 0 && has0) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            double *dst = partial + ((int64_t)blockIdx.x * NQ + q) * g.ncw + c;
            dst[0] = sh[q][tx][0];
            if (has1) dst[1] = sh[q][tx][1];
        }
    }
}

#define ITER_COEF(name, field)                                                                                                                 \
    const int cc__##name = 2 * (threadIdx.x & ((1 << g.tx_bits) - 1));                                                                          \
    const it_v2 name = {cc__##name < g.ncw ? cols[cc__##name].field : 0.0, cc__##name + 1 < g.ncw ? cols[cc__##name + 1].field : 0.0}

// CG start (r = b is in R): z = D^-1 r, p = z, x = 0; partial sums of r.z and r.r
template <bool JAC>
__global__ __launch_bounds__(256) void k_cg_init(PassGeom g, const double *__restrict__ dinv, const double *__restrict__ R, double *__restrict__ Z,
                                                 double *__restrict__ P, double *__restrict__ Xw, double *__restrict__ partial)
{
    iter_pass<2>(g, partial, [&](int64_t row, int64_t o, bool has1, it_v2 *acc) {
        const it_v2 r = ld2(R + o);
        it_v2 z = r;
        if (JAC) {
            z = r * dinv[row];
            st2(Z + o, z, has1);
        }
        st2(P + o, z, has1);
        st2(Xw + o, (it_v2){0.0, 0.0}, has1);
        acc[0] += r * z;
        acc[1] += r * r;
    });
}

// BiCGStab start (r = b is in R): r^ = r, x = p = v = 0; partial sums of r.r twice (rho = r^.r = b.b)
__global__ __launch_bounds__(256) void k_bi_init(PassGeom g, const double *__restrict__ R, double *__restrict__ RH, double *__restrict__ P,
                                                 double *__restrict__ V, double *__restrict__ Xw, double *__restrict__ partial)
{
    iter_pass<2>(g, partial, [&](int64_t, int64_t o, bool has1, it_v2 *acc) {
        const it_v2 r = ld2(R + o), zero = {0.0, 0.0};
        st2(RH + o, r, has1);
        st2(P + o, zero, has1);
        st2(V + o, zero, has1);
        st2(Xw + o, zero, has1);
        acc[0] += r * r;
        acc[1] += r * r;
    });
}

// per-column inner products of one or two panel pairs: a1.b1 [, a2.b2]
template <int NP>
__global__ __launch_bounds__(256) void k_iter_dots(PassGeom g, const double *__restrict__ A1, const double *__restrict__ B1, const double *A2,
                                                   const double *B2, double *__restrict__ partial)
{
    iter_pass<NP>(g, partial, [&](int64_t, int64_t o, bool, it_v2 *acc) {
        acc[0] += ld2(A1 + o) * ld2(B1 + o);
        if (NP == 2) acc[1] += ld2(A2 + o) * ld2(B2 + o);
    });
}

// CG: x += alpha p, r -= alpha q, z = D^-1 r; partial sums of r.z and r.r
template <bool JAC>
__global__ __launch_bounds__(256) void k_cg_update(PassGeom g, const rails_iter_col *__restrict__ cols, const double *__restrict__ dinv,
                                                   const double *__restrict__ P, const double *__restrict__ Q, double *__restrict__ Xw,
                                                   double *__restrict__ R, double *__restrict__ Z, double *__restrict__ partial)
{
    ITER_COEF(alpha, alpha);
    iter_pass<2>(g, partial, [&](int64_t row, int64_t o, bool has1, it_v2 *acc) {
        const it_v2 x = axpy_sel(alpha, ld2(P + o), ld2(Xw + o));
        const it_v2 r = axpy_sel(-alpha, ld2(Q + o), ld2(R + o));
        st2(Xw + o, x, has1);
        st2(R + o, r, has1);
        it_v2 z = r;
        if (JAC) {
            z = r * dinv[row];
            st2(Z + o, z, has1);
        }
        acc[0] += r * z;
        acc[1] += r * r;
    });
}

// CG: p = z + beta p (Z is R without the preconditioner)
__global__ __launch_bounds__(256) void k_cg_dir(PassGeom g, const rails_iter_col *__restrict__ cols, const double *__restrict__ Z, double *__restrict__ P)
{
    ITER_COEF(beta, beta);
    iter_pass<0>(g, nullptr, [&](int64_t, int64_t o, bool has1, it_v2 *) { st2(P + o, axpy_sel(beta, ld2(P + o), ld2(Z + o)), has1); });
}

// BiCGStab: p = r + beta (p - omega v), p^ = D^-1 p
template <bool JAC>
__global__ __launch_bounds__(256) void k_bi_dir(PassGeom g, const rails_iter_col *__restrict__ cols, const double *__restrict__ dinv,
                                                const double *__restrict__ R, const double *__restrict__ V, double *__restrict__ P,
                                                double *__restrict__ PH)
{
    ITER_COEF(beta, beta);
    ITER_COEF(omega, omega);
    iter_pass<0>(g, nullptr, [&](int64_t row, int64_t o, bool has1, it_v2 *) {
        const it_v2 p = axpy_sel(beta, axpy_sel(-omega, ld2(V + o), ld2(P + o)), ld2(R + o));
        st2(P + o, p, has1);
        if (JAC) st2(PH + o, p * dinv[row], has1);
    });
}

// BiCGStab: s = r - alpha v (kept in R), s^ = D^-1 s
template <bool JAC>
__global__ __launch_bounds__(256) void k_bi_s(PassGeom g, const rails_iter_col *__restrict__ cols, const double *__restrict__ dinv,
                                              const double *__restrict__ V, double *__restrict__ R, double *__restrict__ SH)
{
    ITER_COEF(alpha, alpha);
    iter_pass<0>(g, nullptr, [&](int64_t row, int64_t o, bool has1, it_v2 *) {
        const it_v2 s = axpy_sel(-alpha, ld2(V + o), ld2(R + o));
        st2(R + o, s, has1);
        if (JAC) st2(SH + o, s * dinv[row], has1);
    });
}

// BiCGStab: x += alpha p^ + omega s^, r = s - omega t; partial sums of r^.r and r.r.  Without the preconditioner PH is P and SH is R.
__global__ __launch_bounds__(256) void k_bi_update(PassGeom g, const rails_iter_col *__restrict__ cols, const double *PH, const double *SH,
                                                   const double *__restrict__ T, const double *__restrict__ RH, double *__restrict__ Xw, double *R,
                                                   double *__restrict__ partial)
{
    ITER_COEF(alpha, alpha);
    ITER_COEF(omega, omega);
    iter_pass<2>(g, partial, [&](int64_t, int64_t o, bool has1, it_v2 *acc) {
        const it_v2 x = axpy_sel(omega, ld2(SH + o), axpy_sel(alpha, ld2(PH + o), ld2(Xw + o)));
        const it_v2 r = axpy_sel(-omega, ld2(T + o), ld2(R + o));
        st2(Xw + o, x, has1);
        st2(R + o, r, has1);
        acc[0] += ld2(RH + o) * r;
        acc[1] += r * r;
    });
}

// ---- the Chebyshev polynomial preconditioner z = p_K(G A) G r (cheb_coef.h): G is the Jacobi diagonal's inverse (gvec) or the scalar gs
// = +-1; the coefficients are the same for every column and come as kernel arguments ----

__device__ __forceinline__ double cheb_g(const double *__restrict__ gvec, double gs, int64_t row) { return gvec ? gvec[row] : gs; }

// d = z = (g r) / theta
__global__ __launch_bounds__(256) void k_cheb_init(PassGeom g, const double *__restrict__ gvec, double gs, double theta, const double *__restrict__ R,
                                                   double *__restrict__ D, double *__restrict__ Z)
{
    iter_pass<0>(g, nullptr, [&](int64_t row, int64_t o, bool has1, it_v2 *) {
        const it_v2 d = (ld2(R + o) * cheb_g(gvec, gs, row)) / theta;
        st2(D + o, d, has1);
        st2(Z + o, d, has1);
    });
}

// the unfused step, after Q = A z: d = a d + b g (r - q), z += d
__global__ __launch_bounds__(256) void k_cheb_pass(PassGeom g, const double *__restrict__ gvec, double gs, double a, double b, const double *__restrict__ Q,
                                                   const double *__restrict__ R, double *__restrict__ D, double *__restrict__ Z)
{
    iter_pass<0>(g, nullptr, [&](int64_t row, int64_t o, bool has1, it_v2 *) {
        const it_v2 res = (ld2(R + o) - ld2(Q + o)) * cheb_g(gvec, gs, row);
        const it_v2 d = ld2(D + o) * a + res * b;
        st2(D + o, d, has1);
        st2(Z + o, ld2(Z + o) + d, has1);
    });
}

// The fused step for a stored CSR operator: t = (A Zin)_row by k_spmm_narrow's row gather (spmm.hip: LPR lanes own a row and two adjacent
// columns each, 64 rows per block, the block's (col, val) run staged in LDS, 32-bit byte offsets; one entry at a time for a block whose run
// is longer than the LDS buffer and for the lane of an odd last column), then in the same thread d = a d + b g (r - t) in place and
// Zout = Zin + d.  Zin and Zout are different panels: every block reads rows of Zin that other blocks own.  All panels are work panels of
// the object: window at column 0, one row stride, rows 16-byte aligned.  No atomics, no inner products.
//
// GHOST, a row-partitioned operator: column c >= m is row c - m of the operator's ghost buffer Zg (row stride ldg doubles), which the
// object fills before the step with the rows of Zin the neighbours own (rails_halo_exchange, an even number of columns, so that ghost rows
// are 16-byte aligned like panel rows) -- the select between two bases and two strides k_spmm_narrow<RPG, true, LPR> makes.  The epilogue
// is the same: local rows only.
#include "csr_row_gather.inc"

template <int RPG, int LPR, bool GHOST>
__global__ __launch_bounds__(256) void k_cheb_step_csr(int64_t m, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                       const double *__restrict__ val, const double *__restrict__ Zin, int ld, int nc, int64_t blocks_per_xcd,
                                                       const double *__restrict__ gvec, double gs, double a, double b, const double *__restrict__ R,
                                                       double *__restrict__ D, double *__restrict__ Zout, const double *__restrict__ Zg, int ldg)
{
    csr_row_gather<RPG, LPR, GHOST>(m, rowptr, col, val, Zin, ld, nc, blocks_per_xcd, Zg, ldg, [&](int64_t row, int64_t o, it_v2 acc, bool full) {
        // the epilogue on this thread's own two entries of the row (the pad column beside an odd last column is read, never written)
        const it_v2 res = (ld2(R + o) - acc) * cheb_g(gvec, gs, row);
        const it_v2 d = ld2(D + o) * a + res * b;
        st2(D + o, d, full);
        st2(Zout + o, ld2(Zin + o) + d, full);
    });
}

// ---- the multigrid cycle's own kernels.  All panels are work panels: window at column 0, one row stride ld, rows
// 16-byte aligned, a zeroed pad column beside an odd width ----

// Q = R - A Z by the fused step's row gather
template <int RPG, int LPR>
__global__ __launch_bounds__(256) void k_amg_residual_csr(int64_t m, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                          const double *__restrict__ val, const double *__restrict__ Z, int ld, int nc, int64_t blocks_per_xcd,
                                                          const double *__restrict__ R, double *__restrict__ Q)
{
    csr_row_gather<RPG, LPR, false>(m, rowptr, col, val, Z, ld, nc, blocks_per_xcd, nullptr, 0,
                                    [&](int64_t, int64_t o, it_v2 acc, bool full) { st2(Q + o, ld2(R + o) - acc, full); });
}

// the unfused residual, after Q = A Z: Q = R - Q
__global__ __launch_bounds__(256) void k_amg_residual_pass(PassGeom g, const double *__restrict__ R, double *__restrict__ Q)
{
    iter_pass<0>(g, nullptr, [&](int64_t, int64_t o, bool has1, it_v2 *) { st2(Q + o, ld2(R + o) - ld2(Q + o), has1); });
}

// Z += P Zc in the passes' thread layout (a pair of columns per thread): a gather over the row of P, its entries added in stored order.
// Rows of at most 8 entries -- all of them on a 2D grid -- load their entries and the rows of Zc they name first and add then; a longer
// row (3D, wide bands: 13 to 26 entries) takes a plain loop.  The same sum either way.  Zc has the row stride of Z.
__global__ __launch_bounds__(256) void k_amg_prolong_add(PassGeom g, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                         const double *__restrict__ val, const double *__restrict__ Zc, double *__restrict__ Z)
{
    iter_pass<0>(g, nullptr, [&](int64_t row, int64_t o, bool has1, it_v2 *) {
        const int c = (int)(o - row * g.ld);
        const int64_t p0 = rowptr[row], p1 = rowptr[row + 1];
        it_v2 acc = (it_v2){0.0, 0.0};
        if (p1 - p0 <= 8) {
            it_v2 x[8];
            double av[8];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (p0 + u < p1) { // nothing is read past the end of the row: an empty row reads nothing at all
                    av[u] = val[p0 + u];
                    x[u] = ld2(Zc + (int64_t)col[p0 + u] * g.ld + c);
                }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (p0 + u < p1) {
                    acc.x = __builtin_fma(av[u], x[u].x, acc.x);
                    acc.y = __builtin_fma(av[u], x[u].y, acc.y);
                }
        } else {
            for (int64_t q = p0; q < p1; ++q) {
                const it_v2 x = ld2(Zc + (int64_t)col[q] * g.ld + c);
                const double av = val[q];
                acc.x = __builtin_fma(av, x.x, acc.x);
                acc.y = __builtin_fma(av, x.y, acc.y);
            }
        }
        st2(Z + o, ld2(Z + o) + acc, has1);
    });
}

// Z = Ainv R on the last level: Ainv is n x n (n <= 1024), column-major; row i of the result adds Ainv(i, k) R(k, :) for k = 0 .. n - 1 in
// that order.  The passes' thread layout, no atomics.
__global__ __launch_bounds__(256) void k_amg_coarse_dense(PassGeom g, const double *__restrict__ Ainv, const double *__restrict__ R, double *__restrict__ Z)
{
    iter_pass<0>(g, nullptr, [&](int64_t row, int64_t o, bool has1, it_v2 *) {
        const int c = (int)(o - row * g.ld);
        it_v2 acc = (it_v2){0.0, 0.0};
        for (int64_t k = 0; k < g.m; ++k) {
            const double av = Ainv[row + k * g.m];
            const it_v2 x = ld2(R + k * g.ld + c);
            acc.x = __builtin_fma(av, x.x, acc.x);
            acc.y = __builtin_fma(av, x.y, acc.y);
        }
        st2(Z + o, acc, has1);
    });
}

// CG with the polynomial, start (r = b in R, z = p(A) r in Z): p = z, x = 0; partial sums of r.z and r.r
__global__ __launch_bounds__(256) void k_cg_init_poly(PassGeom g, const double *__restrict__ R, const double *__restrict__ Z, double *__restrict__ P,
                                                      double *__restrict__ Xw, double *__restrict__ partial)
{
    iter_pass<2>(g, partial, [&](int64_t, int64_t o, bool has1, it_v2 *acc) {
        const it_v2 r = ld2(R + o), z = ld2(Z + o);
        st2(P + o, z, has1);
        st2(Xw + o, (it_v2){0.0, 0.0}, has1);
        acc[0] += r * z;
        acc[1] += r * r;
    });
}

// sums[e] = sum over the blocks of partial[block][e], e < n <= 64, in a fixed order: 16 interleaved strands, then the strands 0..15
__device__ __forceinline__ void iter_reduce(const double *__restrict__ partial, int64_t nslab, int n, double *sums)
{
    __shared__ double sh[16][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    double s = 0.0;
    if (tx < n)
        for (int64_t t = ty; t < nslab; t += 16) s += partial[t * n + tx];
    sh[ty][tx] = s;
    __syncthreads();
    if (ty == 0) {
        double r = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) r += sh[k][tx];
        sums[tx] = tx < n ? r : 0.0;
    }
    __syncthreads();
}

// the scalar step of column j from the reduced sums (q0 = sums[j], q1 = sums[ncw + j])
__device__ __forceinline__ void iter_compute(int step, rails_iter_col &c, double q0, double q1, double tol2, int maxit, double sign)
{
    switch (step) {
    case STEP_CG_INIT: rails_iter_start(c, q1, q0, maxit); break;
    case STEP_CG_ALPHA: rails_iter_cg_alpha(c, q0, sign); break;
    case STEP_CG_BETA: rails_iter_cg_beta(c, q0, q1, tol2, maxit); break;
    case STEP_BI_INIT: rails_iter_start(c, q1, q0, maxit); break;
    case STEP_BI_ALPHA: rails_iter_bi_alpha(c, q0); break;
    case STEP_BI_OMEGA: rails_iter_bi_omega(c, q0, q1); break;
    default: rails_iter_bi_end(c, q0, q1, tol2, maxit); break;
    }
}

// the columns' scalar step from the reduced sums, then the count (thread 0 of the one workgroup)
__device__ __forceinline__ void iter_columns(int step, const double *sums, int ncw, int nq, rails_iter_col *cols, int32_t *status, double tol2, int maxit,
                                             double sign)
{
    if ((int)threadIdx.x < ncw) {
        rails_iter_col c = cols[threadIdx.x];
        iter_compute(step, c, sums[threadIdx.x], nq == 2 ? sums[ncw + threadIdx.x] : 0.0, tol2, maxit, sign);
        cols[threadIdx.x] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0 && (step == STEP_CG_INIT || step == STEP_BI_INIT || step == STEP_CG_BETA || step == STEP_BI_END)) {
        int active = 0, bad = 0;
        for (int j = 0; j < ncw; ++j) {
            active += (cols[j].flags & RAILS_ITER_ACTIVE) ? 1 : 0;
            bad += (cols[j].flags & RAILS_ITER_NONFINITE) ? 1 : 0;
        }
        status[0] = active;
        if (step == STEP_CG_INIT || step == STEP_BI_INIT) status[1] = bad;
    }
}

// one workgroup: reduce, compute, count.  status[0] = active columns, status[1] = columns whose right-hand side is not finite (start only)
__global__ __launch_bounds__(1024) void k_iter_scalars(int step, const double *__restrict__ partial, int64_t nslab, int ncw, int nq,
                                                       rails_iter_col *cols, int32_t *status, double tol2, int maxit, double sign)
{
    __shared__ double sums[64];
    iter_reduce(partial, nslab, nq * ncw, sums);
    iter_columns(step, sums, ncw, nq, cols, status, tol2, maxit, sign);
}

// The scalar step of a context that reduces (a row partition, an all-reduce hook, a communicator), in three stream-ordered steps:
// k_iter_reduce sums this rank's partial sums exactly as k_iter_scalars does and writes the nq * ncw <= 64 sums to a buffer of the
// object, rails_allreduce_dev adds them over the ranks, k_iter_compute goes on from there.  Every rank then computes from the same sums,
// so the columns' scalars, flags and the active count are the same bits on every rank.
__global__ __launch_bounds__(1024) void k_iter_reduce(const double *__restrict__ partial, int64_t nslab, int n, double *__restrict__ out)
{
    __shared__ double sums[64];
    iter_reduce(partial, nslab, n, sums);
    if ((int)threadIdx.x < n) out[threadIdx.x] = sums[threadIdx.x];
}

__global__ __launch_bounds__(64) void k_iter_compute(int step, const double *__restrict__ sums, int ncw, int nq, rails_iter_col *cols, int32_t *status,
                                                     double tol2, int maxit, double sign)
{
    iter_columns(step, sums, ncw, nq, cols, status, tol2, maxit, sign);
}

// CG: x r p q [z]; BiCGStab: x r p v(=Q) [p^(=Z)] r^ t [s^]; the polynomial: z, its direction d, the second z of the fused step's ping-pong
enum { W_X = 0, W_R, W_P, W_Q, W_Z, W_RH, W_T, W_SH, W_D, W_Z2, W_COUNT };

// The multigrid hierarchy on the device (amg_host.h builds it on the host).  Level 0 works in the object's own work panels (r = W_R, z =
// W_Z / W_Z2, d = W_D, q = W_Q) on the object's operator; the levels below own their operators and five panels of the same row stride;
// the last matrix is its dense inverse with two panels (none when there is no level: W_R and W_Z then).
enum { L_R = 0, L_Z, L_Z2, L_D, L_Q, L_COUNT };
struct AmgLevel {
    int64_t n = 0, nnz = 0;
    double hi = 0.0;
    rails_csr *A = nullptr; // level 0: the object's operator (not owned)
    rails_csr *P = nullptr, *R = nullptr;
    double *dinv = nullptr;
    rails_panel *w[L_COUNT] = {};
};
struct Amg {
    std::vector<AmgLevel> lv;
    int64_t n_coarse = 0, coarse_nnz = 0;
    double *Ainv = nullptr;
    rails_panel *rc = nullptr, *zc = nullptr;
    int cols = 0; // columns of the level panels
    double host_seconds = 0.0, upload_seconds = 0.0;
};

} // namespace

struct rails_iter {
    rails_ctx *ctx = nullptr;
    rails_csr *A = nullptr;
    int method = 0;
    int64_t m = 0;
    double *dinv = nullptr; // 1 / diagonal (null: no preconditioner available)
    double defsign = 1.0;   // -1 when every diagonal entry is known and negative (CG without the preconditioner, iter_scalars.h)
    double tol = 1e-10;
    int maxit = 1000, jacobi = 1, check_every = 8, strict = 0;
    rails_panel *w[W_COUNT] = {};
    int work_cols = 0;
    rails_iter_col *cols_dev = nullptr;
    int cols_cap = 0;
    int32_t *status_dev = nullptr;
    void *pinned = nullptr;
    size_t pinned_bytes = 0;
    std::vector<rails_iter_col> last; // the columns of the last solve
    // statistics: last solve, totals
    long last_dots = 0, last_launches = 0, last_products = 0;
    // the Chebyshev polynomial preconditioner (cheb_coef.h): degree 0 is off
    int poly_degree = 0, poly_fused = 1;
    double poly_ratio = RAILS_ITER_POLY_RATIO, eig_max = 0.0;
    double hi_jacobi = 0.0, hi_plain = 0.0; // Gershgorin bounds on D^-1 A and on +-A from the host CSR arrays (0: none)
    long last_poly = 0, last_fused = 0;
    // a context that reduces (rails_allreduce_dev does something on it): the scalar step in three parts around an all-reduce of `sums_dev`
    bool reduces = false;
    double *sums_dev = nullptr; // 64 doubles
    long last_allreduces = 0, last_halo = 0; // all-reduces of the last call; ghost-row exchanges the object issued itself (fused steps)
    // the multigrid preconditioner ("amg"): off by default; the hierarchy is built on first use (rails_iter_amg_setup)
    int amg = 0, amg_degree = 1, amg_coarse = RAILS_AMG_COARSE;
    double amg_ratio = 4.0, amg_theta = RAILS_AMG_THETA;
    Amg *hier = nullptr;
    long last_cycles = 0, last_cycle_products = 0, last_cycle_launches = 0; // of the last call: cycles, and the products and launches inside them
    double tot_solves = 0, tot_iterations = 0, tot_flagged = 0, tot_products = 0, tot_columns = 0;
};

namespace {

void release_work(rails_iter *it)
{
    for (rails_panel *&p : it->w) {
        rails_panel_destroy(p);
        p = nullptr;
    }
    it->work_cols = 0;
}

void amg_release_panels(Amg *H)
{
    for (AmgLevel &L : H->lv)
        for (rails_panel *&p : L.w) {
            rails_panel_destroy(p);
            p = nullptr;
        }
    rails_panel_destroy(H->rc);
    rails_panel_destroy(H->zc);
    H->rc = H->zc = nullptr;
    H->cols = 0;
}

// drops the hierarchy (a changed "amg_theta" or "amg_coarse", a rebuild, the end of the object)
void amg_release(rails_iter *it)
{
    Amg *H = it->hier;
    if (!H) return;
    if (it->ctx) hipStreamSynchronize(it->ctx->stream);
    amg_release_panels(H);
    for (size_t l = 0; l < H->lv.size(); ++l) {
        AmgLevel &L = H->lv[l];
        if (l > 0) rails_csr_destroy(L.A);
        rails_csr_destroy(L.P);
        rails_csr_destroy(L.R);
        hipFree(L.dinv);
    }
    hipFree(H->Ainv);
    delete H;
    it->hier = nullptr;
}

// the level panels follow the work panels: the same columns, so the same row stride; they grow only when a wider group arrives
int amg_grow(rails_ctx *c, rails_iter *it)
{
    Amg *H = it->hier;
    if (H->cols == it->work_cols) return RAILS_OK;
    amg_release_panels(H);
    for (size_t l = 1; l < H->lv.size(); ++l)
        for (rails_panel *&p : H->lv[l].w) RAILS_TRY(rails_panel_create(c, H->lv[l].n, it->work_cols, &p)); // (zeroed: the pad column is)
    if (!H->lv.empty()) {
        RAILS_TRY(rails_panel_create(c, H->n_coarse, it->work_cols, &H->rc));
        RAILS_TRY(rails_panel_create(c, H->n_coarse, it->work_cols, &H->zc));
    }
    H->cols = it->work_cols;
    return RAILS_OK;
}

// What the multigrid preconditioner refuses, by reason.  "amg" cannot be on without having passed here (rails_iter_set is the gate, and it
// holds the polynomial off afterwards), so a solve needs no check of its own; rails_iter_amg_setup, which may be called with "amg" off,
// checks again.  A sparse right-hand side or a rectangular operator never gets this far: rails_iter_create refuses them.
int amg_check(const rails_iter *it, const char *who)
{
    const rails_csr *A = it->A;
    RAILS_REQUIRE(it->method == RAILS_ITER_CG, "%s: \"amg\" on a BiCGStab object: the multigrid preconditioner is for conjugate gradients (a symmetric definite operator)", who);
    RAILS_REQUIRE(it->poly_degree == 0, "%s: \"amg\" together with poly_degree %d: one preconditioner at a time", who, it->poly_degree);
    RAILS_REQUIRE(A->kind != rails_csr::CALLBACK, "%s: \"amg\" needs the entries of the matrix: the operator is a callback", who);
    RAILS_REQUIRE(A->kind != rails_csr::LU && A->kind != rails_csr::ITER, "%s: \"amg\" needs the entries of the matrix: the operator is an LU or an iterative solve", who);
    RAILS_REQUIRE(!it->reduces && A->n_ghost == 0 && A->n_send == 0,
                  "%s: \"amg\" on a context that reduces (more than one rank, an all-reduce hook or a communicator): the multigrid preconditioner is single GPU", who);
    RAILS_REQUIRE(it->m < ((int64_t)1 << 24), "%s: \"amg\" on %lld rows: the multigrid preconditioner takes fewer than 2^24", who, (long long)it->m);
    return RAILS_OK;
}

bool uses_panel(const rails_iter *it, int which)
{
    const bool jac = it->dinv != nullptr;
    if (which == W_D || which == W_Z2) return it->poly_degree > 0 || it->amg;
    if (which == W_Z && (it->poly_degree > 0 || it->amg)) return true;
    if (it->method == RAILS_ITER_CG) return which == W_X || which == W_R || which == W_P || which == W_Q || (which == W_Z && jac);
    return which == W_X || which == W_R || which == W_P || which == W_Q || which == W_RH || which == W_T || ((which == W_Z || which == W_SH) && jac);
}

// `also`: panels (bits 1 << W_...) wanted beside those the method uses (rails_iter_precondition)
int grow_work(rails_ctx *c, rails_iter *it, int cols, unsigned also = 0)
{
    bool missing = false; // a setting made after the last solve may ask for a panel that is not there yet
    for (int k = 0; k < W_COUNT; ++k) missing = missing || ((uses_panel(it, k) || (also >> k & 1)) && !it->w[k]);
    if (cols <= it->work_cols && !missing) return RAILS_OK;
    cols = std::max(cols, it->work_cols);
    for (int k = 0; k < W_COUNT; ++k) also |= it->w[k] ? 1u << k : 0u;
    release_work(it);
    for (int k = 0; k < W_COUNT; ++k)
        if (uses_panel(it, k) || (also >> k & 1)) {
            RAILS_TRY(rails_panel_create(c, it->m, cols, &it->w[k]));
            RAILS_HIP_CHECK(hipMemsetAsync(it->w[k]->d, 0, (size_t)it->m * it->w[k]->ld * sizeof(double), c->stream));
        }
    it->work_cols = cols;
    return RAILS_OK;
}

int grow_cols(rails_ctx *c, rails_iter *it, int nc)
{
    if (nc > it->cols_cap) {
        RAILS_HIP_CHECK(hipStreamSynchronize(c->stream));
        if (it->cols_dev) RAILS_HIP_CHECK(hipFree(it->cols_dev));
        it->cols_dev = nullptr;
        it->cols_cap = 0;
        const int cap = (nc + 31) / 32 * 32;
        RAILS_HIP_CHECK(hipMalloc((void **)&it->cols_dev, (size_t)cap * sizeof(rails_iter_col)));
        it->cols_cap = cap;
        c->n_dev_alloc++;
    }
    const size_t want = 64 + (size_t)it->cols_cap * sizeof(rails_iter_col);
    if (want > it->pinned_bytes) {
        RAILS_HIP_CHECK(hipStreamSynchronize(c->stream));
        if (it->pinned) RAILS_HIP_CHECK(hipHostFree(it->pinned));
        it->pinned = nullptr;
        it->pinned_bytes = 0;
        RAILS_HIP_CHECK(hipHostMalloc(&it->pinned, want, hipHostMallocDefault));
        it->pinned_bytes = want;
    }
    return RAILS_OK;
}

struct Run {
    rails_ctx *c;
    rails_iter *it;
    int trans;
    PassGeom g;
    int64_t nslab;
    rails_iter_col *cols;
    bool jac;
    double tol2;
    // the polynomial: degree (0: off), theta and the coefficient pairs, whether its steps run on the fused kernel
    int K = 0;
    bool fused = false, ghost = false; // ghost: the fused step in its ghost-row form, with an exchange of the object's own before it
    double theta = 1.0, ca[RAILS_CHEB_MAX_DEGREE], cb[RAILS_CHEB_MAX_DEGREE];
    bool amg = false; // the multigrid cycle is the preconditioner (K is 0 then)

    double *d(int k) const { return it->w[k]->d; }
    int scalars(int step, int nq)
    {
        // (with the polynomial r.z carries the sign of the operator itself, as with Jacobi)
        const double sign = (jac || K > 0 || amg) ? 1.0 : it->defsign;
        if (!it->reduces) {
            RAILS_LAUNCH(k_iter_scalars, dim3(1), dim3(1024), 0, c->stream, step, c->ws, nslab, g.ncw, nq, cols, it->status_dev, tol2, it->maxit, sign);
            it->last_launches++;
            return RAILS_OK;
        }
        RAILS_LAUNCH(k_iter_reduce, dim3(1), dim3(1024), 0, c->stream, c->ws, nslab, nq * g.ncw, it->sums_dev);
        RAILS_TRY(rails_allreduce_dev(c, it->sums_dev, (size_t)(nq * g.ncw)));
        it->last_allreduces++;
        RAILS_LAUNCH(k_iter_compute, dim3(1), dim3(64), 0, c->stream, step, it->sums_dev, g.ncw, nq, cols, it->status_dev, tol2, it->maxit, sign);
        it->last_launches += 2;
        return RAILS_OK;
    }
    int product(int from, int to)
    {
        it->last_products++;
        return rails_spmm(c, it->A, it->method == RAILS_ITER_CG ? 0 : trans, it->w[from], 0, g.ncw, it->w[to], 0); // CG: a symmetric operator
    }
    int dots(int np, int a1, int b1, int a2, int b2)
    {
        RAILS_TRY(rails_ws_reserve(c, (size_t)nslab * 2 * g.ncw * sizeof(double)));
        if (np == 1)
            RAILS_LAUNCH((k_iter_dots<1>), dim3((unsigned)nslab), dim3(256), 0, c->stream, g, d(a1), d(b1), d(a1), d(b1), c->ws);
        else
            RAILS_LAUNCH((k_iter_dots<2>), dim3((unsigned)nslab), dim3(256), 0, c->stream, g, d(a1), d(b1), d(a2), d(b2), c->ws);
        it->last_launches++;
        it->last_dots += np * g.ncw;
        return RAILS_OK;
    }
#define ITER_PASS_LAUNCH(kernel_jac, kernel_plain, ...)                                                                                      \
    do {                                                                                                                                     \
        RAILS_TRY(rails_ws_reserve(c, (size_t)nslab * 2 * g.ncw * sizeof(double)));                                                          \
        if (jac)                                                                                                                             \
            RAILS_LAUNCH(kernel_jac, dim3((unsigned)nslab), dim3(256), 0, c->stream, __VA_ARGS__);                                          \
        else                                                                                                                                 \
            RAILS_LAUNCH(kernel_plain, dim3((unsigned)nslab), dim3(256), 0, c->stream, __VA_ARGS__);                                        \
        it->last_launches++;                                                                                                                 \
    } while (0)

    // W_Z = p_K(G A) G W_R (K = 0: G W_R).  The fused steps read one z panel and write the other, and start in the one that makes the
    // last of them write W_Z; the unfused ones work in W_Z with A z in W_Q.
    int polynomial()
    {
        const double *gvec = jac ? it->dinv : nullptr;
        const double gs = it->defsign;
        const dim3 grid((unsigned)nslab), block(256);
        int zin = (fused && (K & 1)) ? W_Z2 : W_Z;
        RAILS_LAUNCH(k_cheb_init, grid, block, 0, c->stream, g, gvec, gs, theta, d(W_R), d(W_D), d(zin));
        it->last_launches++;
        it->last_poly++;
        const rails_csr *A = it->A;
        const int64_t bpx = ((it->m + 63) / 64 + 7) / 8;
        for (int k = 0; k < K; ++k) {
            if (!fused) {
                RAILS_TRY(product(W_Z, W_Q));
                RAILS_LAUNCH(k_cheb_pass, grid, block, 0, c->stream, g, gvec, gs, ca[k], cb[k], d(W_Q), d(W_R), d(W_D), d(W_Z));
                it->last_launches++;
                continue;
            }
            const int zout = zin == W_Z ? W_Z2 : W_Z;
            if (ghost) {
                // one exchange per step, as the unfused step's rails_spmm makes one: ranks that choose differently stay in step.  An even
                // number of columns, so that ghost rows are as aligned as panel rows: at an odd width the panel's column ncw travels too.
                // That is the pad column (zeroed at allocation, never written) when the group is as wide as the panels, and a column a
                // wider group has used otherwise; on the receiving side nobody reads it, since the lane of an odd last column takes its
                // one-entry path -- what it holds reaches no result, as with the pair loads of every pass (section 14's last test)
                const int nce = (g.ncw + 1) & ~1;
                RAILS_TRY(rails_halo_exchange(c, it->A, d(zin), g.ld, nce));
                it->last_halo++;
                if (g.ncw <= 16)
                    RAILS_LAUNCH((k_cheb_step_csr<2, 8, true>), dim3((unsigned)(bpx * 8)), block, 0, c->stream, it->m, A->rowptr, A->col, A->val, d(zin), g.ld,
                                 g.ncw, bpx, gvec, gs, ca[k], cb[k], d(W_R), d(W_D), d(zout), A->ext, nce);
                else
                    RAILS_LAUNCH((k_cheb_step_csr<4, 16, true>), dim3((unsigned)(bpx * 8)), block, 0, c->stream, it->m, A->rowptr, A->col, A->val, d(zin), g.ld,
                                 g.ncw, bpx, gvec, gs, ca[k], cb[k], d(W_R), d(W_D), d(zout), A->ext, nce);
            } else if (g.ncw <= 16)
                RAILS_LAUNCH((k_cheb_step_csr<2, 8, false>), dim3((unsigned)(bpx * 8)), block, 0, c->stream, it->m, A->rowptr, A->col, A->val, d(zin), g.ld, g.ncw, bpx,
                             gvec, gs, ca[k], cb[k], d(W_R), d(W_D), d(zout), nullptr, 0);
            else
                RAILS_LAUNCH((k_cheb_step_csr<4, 16, false>), dim3((unsigned)(bpx * 8)), block, 0, c->stream, it->m, A->rowptr, A->col, A->val, d(zin), g.ld, g.ncw, bpx,
                             gvec, gs, ca[k], cb[k], d(W_R), d(W_D), d(zout), nullptr, 0);
            it->last_launches++;
            it->last_products++;
            it->last_fused++;
            zin = zout;
        }
        return RAILS_OK;
    }
    // ---- the multigrid V-cycle: W_Z = M W_R.  Down: smooth from zero, residual, restrict; the dense inverse at
    // the bottom; up: prolong and correct, smooth from z.  Nothing in here synchronises, allocates or reads back.
    rails_panel *lpanel(int l, int which) const
    {
        static const int own[L_COUNT] = {W_R, W_Z, W_Z2, W_D, W_Q};
        return l == 0 ? it->w[own[which]] : it->hier->lv[(size_t)l].w[which];
    }
    double *lp(int l, int which) const { return lpanel(l, which)->d; }
    // a kernel on the shared row gather over level L's matrix: 64 rows per block, the blocks dealt over the 8 XCDs; its 8-lane form up to
    // 16 columns, its 16-lane form above.  `rest` is what follows the gather's own arguments.
    template <class K8, class K16, class... Rest>
    void launch_gather(K8 k8, K16 k16, const AmgLevel &L, const double *zin, Rest... rest)
    {
        const int64_t bpx = ((L.n + 63) / 64 + 7) / 8;
        if (g.ncw <= 16)
            RAILS_LAUNCH(k8, dim3((unsigned)(bpx * 8)), dim3(256), 0, c->stream, L.n, L.A->rowptr, L.A->col, L.A->val, zin, g.ld, g.ncw, bpx, rest...);
        else
            RAILS_LAUNCH(k16, dim3((unsigned)(bpx * 8)), dim3(256), 0, c->stream, L.n, L.A->rowptr, L.A->col, L.A->val, zin, g.ld, g.ncw, bpx, rest...);
    }
    // the passes' geometry on n rows (set_group's rule)
    void level_geom(int64_t n, PassGeom *lg, int64_t *slabs) const
    {
        const int TY = 256 >> g.tx_bits;
        int64_t ns = std::max<int64_t>(1, std::min<int64_t>(1024, n / ((int64_t)TY * 8)));
        const int64_t rps = (n + ns - 1) / ns;
        *slabs = (n + rps - 1) / rps;
        *lg = PassGeom{g.ncw, g.ld, g.tx_bits, n, rps};
    }
    void count_cycle(long launches, long products)
    {
        it->last_launches += launches;
        it->last_cycle_launches += launches;
        it->last_products += products;
        it->last_cycle_products += products;
    }
    // one smoother step on level l: d = a d + b g (r - A z), z += d; *z names the panel that holds z and follows the fused step's ping-pong
    int smooth_step(int l, bool lfused, const PassGeom &lg, int64_t slabs, double a, double b, int *z)
    {
        const AmgLevel &L = it->hier->lv[(size_t)l];
        if (!lfused) {
            RAILS_TRY(rails_spmm(c, L.A, 0, lpanel(l, *z), 0, g.ncw, lpanel(l, L_Q), 0));
            RAILS_LAUNCH(k_cheb_pass, dim3((unsigned)slabs), dim3(256), 0, c->stream, lg, L.dinv, 1.0, a, b, lp(l, L_Q), lp(l, L_R), lp(l, L_D), lp(l, *z));
            count_cycle(1, 1);
            return RAILS_OK;
        }
        const int zout = *z == L_Z ? L_Z2 : L_Z;
        launch_gather(k_cheb_step_csr<2, 8, false>, k_cheb_step_csr<4, 16, false>, L, lp(l, *z), (const double *)L.dinv, 1.0, a, b, (const double *)lp(l, L_R), lp(l, L_D),
                      lp(l, zout), (const double *)nullptr, 0);
        count_cycle(1, 1);
        it->last_fused++;
        *z = zout;
        return RAILS_OK;
    }
    int vcycle()
    {
        Amg &H = *it->hier;
        const int nl = (int)H.lv.size(), S = it->amg_degree;
        int zat[RAILS_AMG_MAX_LEVELS];
        bool lfused[RAILS_AMG_MAX_LEVELS];
        double th[RAILS_AMG_MAX_LEVELS], a[9], b[9];
        it->last_cycles++;
        for (int l = 0; l < nl; ++l) {
            const AmgLevel &L = H.lv[(size_t)l];
            PassGeom lg;
            int64_t slabs;
            level_geom(L.n, &lg, &slabs);
            RAILS_REQUIRE(rails_cheb_coef(L.hi / it->amg_ratio, L.hi, S, &th[l], a, b), "rails_iter: no smoother of degree %d on [%g, %g] (level %d)", S, L.hi / it->amg_ratio, L.hi, l);
            lfused[l] = it->poly_fused && rails_cheb_fused_eligible(true, 0, L.n, g.ld);
            // every fused step moves z to the other panel, and there are 2 S + 1 of them: the top level starts where its last one writes W_Z
            zat[l] = lfused[l] ? L_Z2 : L_Z;
            RAILS_LAUNCH(k_cheb_init, dim3((unsigned)slabs), dim3(256), 0, c->stream, lg, L.dinv, 1.0, th[l], lp(l, L_R), lp(l, L_D), lp(l, zat[l]));
            count_cycle(1, 0);
            for (int k = 0; k < S; ++k) RAILS_TRY(smooth_step(l, lfused[l], lg, slabs, a[k], b[k], &zat[l]));
            if (lfused[l]) {
                launch_gather(k_amg_residual_csr<2, 8>, k_amg_residual_csr<4, 16>, L, lp(l, zat[l]), (const double *)lp(l, L_R), lp(l, L_Q));
            } else {
                RAILS_TRY(rails_spmm(c, L.A, 0, lpanel(l, zat[l]), 0, g.ncw, lpanel(l, L_Q), 0));
                RAILS_LAUNCH(k_amg_residual_pass, dim3((unsigned)slabs), dim3(256), 0, c->stream, lg, lp(l, L_R), lp(l, L_Q));
            }
            count_cycle(1, 1);
            RAILS_TRY(rails_spmm(c, L.R, 0, lpanel(l, L_Q), 0, g.ncw, l + 1 < nl ? lpanel(l + 1, L_R) : H.rc, 0)); // r_{l+1} = P' q
            count_cycle(0, 1);
        }
        {
            PassGeom lg;
            int64_t slabs;
            level_geom(H.n_coarse, &lg, &slabs);
            RAILS_LAUNCH(k_amg_coarse_dense, dim3((unsigned)slabs), dim3(256), 0, c->stream, lg, H.Ainv, nl ? H.rc->d : d(W_R), nl ? H.zc->d : d(W_Z));
            count_cycle(1, 0);
        }
        for (int l = nl - 1; l >= 0; --l) {
            const AmgLevel &L = H.lv[(size_t)l];
            PassGeom lg;
            int64_t slabs;
            level_geom(L.n, &lg, &slabs);
            const double *below = l + 1 < nl ? lp(l + 1, zat[l + 1]) : H.zc->d;
            RAILS_LAUNCH(k_amg_prolong_add, dim3((unsigned)slabs), dim3(256), 0, c->stream, lg, L.P->rowptr, L.P->col, L.P->val, below, lp(l, zat[l]));
            count_cycle(1, 1);
            // the post-smoother from z, the adjoint of the pre-smoother: one step with (a, b) = (0, 1 / theta) -- d is finite, k_cheb_init wrote
            // it whatever S is -- then S steps with the recurrence's coefficients (recomputed: a and b above held the last level's)
            rails_cheb_coef(L.hi / it->amg_ratio, L.hi, S, &th[l], a, b);
            RAILS_TRY(smooth_step(l, lfused[l], lg, slabs, 0.0, 1.0 / th[l], &zat[l]));
            for (int k = 0; k < S; ++k) RAILS_TRY(smooth_step(l, lfused[l], lg, slabs, a[k], b[k], &zat[l]));
        }
        return RAILS_OK; // (zat[0] is L_Z again: an odd number of fused steps from L_Z2, or no move at all)
    }
    int precondition() { return amg ? vcycle() : polynomial(); }
    int start()
    {
        if (it->method == RAILS_ITER_CG && (K > 0 || amg)) {
            RAILS_TRY(precondition());
            RAILS_TRY(rails_ws_reserve(c, (size_t)nslab * 2 * g.ncw * sizeof(double)));
            RAILS_LAUNCH(k_cg_init_poly, dim3((unsigned)nslab), dim3(256), 0, c->stream, g, d(W_R), d(W_Z), d(W_P), d(W_X), c->ws);
            it->last_launches++;
            it->last_dots += 2 * g.ncw;
            return scalars(STEP_CG_INIT, 2);
        }
        if (it->method == RAILS_ITER_CG) {
            ITER_PASS_LAUNCH((k_cg_init<true>), (k_cg_init<false>), g, it->dinv, d(W_R), jac ? d(W_Z) : nullptr, d(W_P), d(W_X), c->ws);
            it->last_dots += 2 * g.ncw;
            return scalars(STEP_CG_INIT, 2);
        }
        ITER_PASS_LAUNCH(k_bi_init, k_bi_init, g, d(W_R), d(W_RH), d(W_P), d(W_Q), d(W_X), c->ws);
        it->last_dots += 2 * g.ncw;
        return scalars(STEP_BI_INIT, 2);
    }
    int iteration()
    {
        if (it->method == RAILS_ITER_CG && (K > 0 || amg)) {
            // the update without its own z (its partial sums are overwritten below), the polynomial, then r.z and r.r in the layout
            // the scalar step reads; K products in a row without an inner product, a scalar kernel or a read-back between them
            RAILS_TRY(product(W_P, W_Q));
            RAILS_TRY(dots(1, W_P, W_Q, W_P, W_Q));
            RAILS_TRY(scalars(STEP_CG_ALPHA, 1));
            RAILS_LAUNCH((k_cg_update<false>), dim3((unsigned)nslab), dim3(256), 0, c->stream, g, cols, it->dinv, d(W_P), d(W_Q), d(W_X), d(W_R), nullptr, c->ws);
            it->last_launches++;
            RAILS_TRY(precondition());
            RAILS_TRY(dots(2, W_R, W_Z, W_R, W_R));
            RAILS_TRY(scalars(STEP_CG_BETA, 2));
            RAILS_LAUNCH(k_cg_dir, dim3((unsigned)nslab), dim3(256), 0, c->stream, g, cols, d(W_Z), d(W_P));
            it->last_launches++;
            return RAILS_OK;
        }
        if (it->method == RAILS_ITER_CG) {
            const int z = jac ? W_Z : W_R;
            RAILS_TRY(product(W_P, W_Q));
            RAILS_TRY(dots(1, W_P, W_Q, W_P, W_Q));
            RAILS_TRY(scalars(STEP_CG_ALPHA, 1));
            ITER_PASS_LAUNCH((k_cg_update<true>), (k_cg_update<false>), g, cols, it->dinv, d(W_P), d(W_Q), d(W_X), d(W_R), jac ? d(W_Z) : nullptr, c->ws);
            it->last_dots += 2 * g.ncw;
            RAILS_TRY(scalars(STEP_CG_BETA, 2));
            ITER_PASS_LAUNCH(k_cg_dir, k_cg_dir, g, cols, d(z), d(W_P));
            return RAILS_OK;
        }
        const int ph = jac ? W_Z : W_P, sh = jac ? W_SH : W_R;
        ITER_PASS_LAUNCH((k_bi_dir<true>), (k_bi_dir<false>), g, cols, it->dinv, d(W_R), d(W_Q), d(W_P), jac ? d(W_Z) : nullptr);
        RAILS_TRY(product(ph, W_Q)); // v = A p^
        RAILS_TRY(dots(1, W_RH, W_Q, W_RH, W_Q));
        RAILS_TRY(scalars(STEP_BI_ALPHA, 1));
        ITER_PASS_LAUNCH((k_bi_s<true>), (k_bi_s<false>), g, cols, it->dinv, d(W_Q), d(W_R), jac ? d(W_SH) : nullptr);
        RAILS_TRY(product(sh, W_T)); // t = A s^
        RAILS_TRY(dots(2, W_T, W_R, W_T, W_T));
        RAILS_TRY(scalars(STEP_BI_OMEGA, 2));
        ITER_PASS_LAUNCH(k_bi_update, k_bi_update, g, cols, d(ph), d(sh), d(W_T), d(W_RH), d(W_X), d(W_R), c->ws);
        it->last_dots += 2 * g.ncw;
        return scalars(STEP_BI_END, 2);
    }
#undef ITER_PASS_LAUNCH
};

// the upper end of the polynomial's interval: "eig_max", else the Gershgorin bound that goes with the preconditioner in effect (0: none)
double poly_hi(const rails_iter *it)
{
    if (it->eig_max > 0.0) return it->eig_max;
    return (it->jacobi && it->dinv) ? it->hi_jacobi : it->hi_plain;
}

// degree, interval and coefficients of a run; the work panels must be there (the fused kernel's rule looks at their row stride)
int poly_setup(Run &run, const char *who)
{
    rails_iter *it = run.it;
    run.K = it->poly_degree;
    run.fused = false;
    run.theta = 1.0;
    if (run.K == 0) return RAILS_OK;
    const double hi = poly_hi(it);
    RAILS_REQUIRE(hi > 0.0 && rails_iter_finite(hi),
                  "%s: poly_degree %d needs an upper bound on the spectrum: the operator keeps no CSR arrays on the host to take one from, set \"eig_max\"", who, run.K);
    RAILS_REQUIRE(rails_cheb_coef(hi / it->poly_ratio, hi, run.K, &run.theta, run.ca, run.cb), "%s: no polynomial of degree %d on [%g, %g]", who, run.K,
                  hi / it->poly_ratio, hi);
    const rails_csr *A = it->A;
    const bool stored = A->kind == rails_csr::STORED && !A->rect && A->rowptr && A->col && A->val;
    // an operator that exchanges (rows to send or ghost rows to receive: rails_spmm's own condition, so that a step issues an exchange in
    // the fused form exactly when it does in the unfused one -- a rank that only sends, or only receives, takes part; a rank whose plan is
    // empty issues none in either form) takes the ghost-row form; its ghost buffer's row stride is the group's width rounded up to even,
    // at most RAILS_ITER_GROUP
    run.ghost = A->n_ghost > 0 || A->n_send > 0;
    if (run.ghost)
        run.fused = it->poly_fused && rails_cheb_fused_ghost_eligible(stored, it->m, A->n_ghost, it->w[W_Z]->ld, RAILS_ITER_GROUP);
    else
        run.fused = it->poly_fused && rails_cheb_fused_eligible(stored, A->n_ghost, it->m, it->w[W_Z]->ld);
    return RAILS_OK;
}

// the passes' geometry for a group of w columns
void set_group(Run &run, int w)
{
    const rails_iter *it = run.it;
    const int pairs = (w + 1) / 2;
    int tx_bits = 0;
    while ((1 << tx_bits) < pairs) ++tx_bits; // <= 4
    const int TY = 256 >> tx_bits;
    // slabs of at least 8 rows per thread, at most 1024 of them (k_colnorms2's rule)
    int64_t nslab = std::max<int64_t>(1, std::min<int64_t>(1024, it->m / ((int64_t)TY * 8)));
    const int64_t rps = (it->m + nslab - 1) / nslab;
    nslab = (it->m + rps - 1) / rps;
    run.g = PassGeom{w, it->w[W_R]->ld, tx_bits, it->m, rps};
    run.nslab = nslab;
}

} // namespace

extern "C" void rails_iter_destroy(rails_iter *it)
{
    if (!it) return;
    if (it->ctx) {
        hipSetDevice(it->ctx->device);
        hipStreamSynchronize(it->ctx->stream);
    }
    amg_release(it);
    release_work(it);
    hipFree(it->dinv);
    hipFree(it->cols_dev);
    hipFree(it->status_dev);
    hipFree(it->sums_dev);
    if (it->pinned) hipHostFree(it->pinned);
    delete it;
}

namespace {

// The gather of iter_agree.h: this rank's slot of a zeroed vector of nranks slots, one sum all-reduce, the whole vector back on the host.
int gather_slots(rails_ctx *c, const double *mine, std::vector<double> &all)
{
    const int nr = std::max(1, c->nranks), n = nr * RAILS_AGREE_SLOT;
    RAILS_REQUIRE(c->rank >= 0 && c->rank < nr, "rails_iter_create: rank %d of %d", c->rank, nr);
    all.assign((size_t)n, 0.0);
    std::copy(mine, mine + RAILS_AGREE_SLOT, all.begin() + (size_t)c->rank * RAILS_AGREE_SLOT);
    double *dev = nullptr;
    RAILS_HIP_CHECK(hipMalloc((void **)&dev, (size_t)n * sizeof(double)));
    int rc = RAILS_OK;
    hipError_t e = hipMemcpyAsync(dev, all.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream); // (the source is pageable host memory)
    if (e == hipSuccess) rc = rails_allreduce_dev(c, dev, (size_t)n);
    if (e == hipSuccess && rc == RAILS_OK) e = hipMemcpyAsync(all.data(), dev, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && rc == RAILS_OK) e = rails_stream_sync(c);
    hipFree(dev);
    if (rc != RAILS_OK) return rc;
    RAILS_HIP_CHECK(e);
    return RAILS_OK;
}

} // namespace

// On a context that reduces, create is a collective call (one all-reduce).  Refusals that every rank reaches alike -- the method, the
// context, a partition without a hook or communicator -- come before it; what only this rank can see (its block's shape, a zero in the
// diagonal it was given) travels through it, so that every rank refuses and none is left waiting.
extern "C" int rails_iter_create(rails_ctx *c, rails_csr *A, int method, const double *diag_host, rails_iter **out)
{
    if (c) hipSetDevice(c->device);
    RAILS_REQUIRE(c && A && out, "rails_iter_create: null argument");
    RAILS_REQUIRE(method == RAILS_ITER_CG || method == RAILS_ITER_BICGSTAB, "rails_iter_create: method %d is neither RAILS_ITER_CG nor RAILS_ITER_BICGSTAB", method);
    RAILS_REQUIRE(c == A->ctx, "rails_iter_create: the operator belongs to another context");
    RAILS_REQUIRE(c->nranks <= 1 || c->allreduce || c->rccl,
                  "rails_iter_create: the context is row-partitioned but has neither an all-reduce hook nor a communicator: without one this object is single GPU only");
    const bool reduces = c->nranks > 1 || c->allreduce || c->rccl; // rails_allreduce_dev's own condition
    const int64_t m = A->m;
    // square: globally, for a stored row block whose halo plan is set (rails_csr_set_halo: m + n_ghost == ncols_ext)
    const bool ghosted = reduces && A->kind == rails_csr::STORED && !A->rect && A->ncols_ext > m && A->n_ghost == A->ncols_ext - m;
    char refusal[192] = "";
    if (A->rect || A->kind == rails_csr::SPRHS || (A->ncols_ext != m && !ghosted))
        snprintf(refusal, sizeof refusal, "rails_iter_create: the operator is rectangular (%lld x %lld)", (long long)m, (long long)rails_csr_cols(A));
    else if (m < 1)
        snprintf(refusal, sizeof refusal, "rails_iter_create: an operator without rows");
    const bool host_csr = !refusal[0] && A->kind == rails_csr::STORED && (int64_t)A->h_rowptr.size() == m + 1 && (int64_t)A->h_val.size() == A->h_rowptr[m];
    std::vector<double> dinv;
    if (refusal[0]) {
    } else if (diag_host) {
        dinv.assign(diag_host, diag_host + m);
        for (int64_t i = 0; i < m && !refusal[0]; ++i)
            if (!(dinv[i] != 0.0 && rails_iter_finite(dinv[i]))) snprintf(refusal, sizeof refusal, "rails_iter_create: diagonal entry %lld is %g", (long long)i, dinv[i]);
    } else if (host_csr) {
        // the CSR diagonal, when every entry of it is stored and nonzero; otherwise no preconditioner
        dinv.assign((size_t)m, 0.0);
        bool ok = true;
        for (int64_t i = 0; i < m && ok; ++i) {
            bool found = false;
            for (int64_t q = A->h_rowptr[i]; q < A->h_rowptr[i + 1]; ++q)
                if (A->h_col[q] == i) {
                    dinv[i] += A->h_val[q];
                    found = true;
                }
            ok = found && dinv[i] != 0.0 && rails_iter_finite(dinv[i]);
        }
        if (!ok) dinv.clear();
    }
    if (refusal[0] && !reduces) {
        rails_set_error("%s", refusal);
        return RAILS_EINVAL;
    }
    if (refusal[0]) dinv.clear();
    bool negative = !dinv.empty();
    for (double &v : dinv) {
        negative = negative && v < 0.0;
        v = 1.0 / v;
    }
    double defsign = negative ? -1.0 : 1.0, hi_plain = 0.0, hi_jacobi = 0.0;
    if (host_csr) {
        // the polynomial preconditioner's upper bounds (two numbers; used only with "poly_degree" above 0).  A row block's rows hold their
        // ghost columns' entries: the local row sums are complete
        hi_plain = rails_cheb_gershgorin(m, A->h_rowptr.data(), A->h_val.data(), nullptr);
        if (!dinv.empty()) hi_jacobi = rails_cheb_gershgorin(m, A->h_rowptr.data(), A->h_val.data(), dinv.data());
    }
    if (reduces) {
        double mine[RAILS_AGREE_SLOT];
        rails_iter_agree_fill(mine, refusal[0] ? RAILS_AGREE_REFUSED : dinv.empty() ? RAILS_AGREE_NO_DIAG : RAILS_AGREE_DIAG, negative, hi_plain, hi_jacobi);
        std::vector<double> all;
        RAILS_TRY(gather_slots(c, mine, all));
        const rails_iter_agreed ag = rails_iter_agree(all.data(), std::max(1, c->nranks));
        if (ag.refused) {
            rails_set_error("%s", refusal[0] ? refusal : "rails_iter_create: another rank refused its arguments");
            return RAILS_EINVAL;
        }
        if (!ag.jacobi) dinv.clear();
        defsign = ag.defsign;
        hi_plain = ag.hi_plain;
        hi_jacobi = ag.hi_jacobi;
    }
    rails_iter *it = new rails_iter;
    it->ctx = c;
    it->A = A;
    it->method = method;
    it->m = m;
    it->reduces = reduces;
    it->defsign = defsign;
    it->hi_plain = hi_plain;
    it->hi_jacobi = hi_jacobi;
    hipError_t e = hipMalloc((void **)&it->status_dev, 16 * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemset(it->status_dev, 0, 16 * sizeof(int32_t));
    if (e == hipSuccess && !dinv.empty()) {
        e = hipMalloc((void **)&it->dinv, (size_t)m * sizeof(double));
        if (e == hipSuccess) e = hipMemcpy(it->dinv, dinv.data(), (size_t)m * sizeof(double), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess && reduces) {
        e = hipMalloc((void **)&it->sums_dev, 64 * sizeof(double));
        if (e == hipSuccess) e = hipMemset(it->sums_dev, 0, 64 * sizeof(double));
    }
    if (e != hipSuccess) {
        rails_set_error("rails_iter_create: device allocation or upload failed: %s", hipGetErrorString(e));
        rails_iter_destroy(it);
        return RAILS_EHIP;
    }
    *out = it;
    return RAILS_OK;
}

extern "C" int rails_iter_set(rails_iter *it, const char *name, double value)
{
    RAILS_REQUIRE(it && name, "rails_iter_set: null argument");
    RAILS_REQUIRE(rails_iter_finite(value), "rails_iter_set: %s = %g", name, value);
    const std::string n(name);
    if (n == "tolerance") {
        RAILS_REQUIRE(value >= 0.0, "rails_iter_set: tolerance %g", value);
        it->tol = value;
    } else if (n == "max_iterations") {
        RAILS_REQUIRE(value >= 0.0 && value <= 1e9, "rails_iter_set: max_iterations %g", value);
        it->maxit = (int)value;
    } else if (n == "jacobi")
        it->jacobi = value != 0.0;
    else if (n == "check_every") {
        RAILS_REQUIRE(value >= 1.0 && value <= 1e9, "rails_iter_set: check_every %g", value);
        it->check_every = (int)value;
    } else if (n == "strict")
        it->strict = value != 0.0;
    else if (n == "poly_degree") {
        RAILS_REQUIRE(value >= 0.0 && value <= RAILS_CHEB_MAX_DEGREE && value == std::floor(value), "rails_iter_set: poly_degree %g is not a whole number in 0 .. %d", value,
                      RAILS_CHEB_MAX_DEGREE);
        RAILS_REQUIRE(value == 0.0 || !it->amg, "rails_iter_set: poly_degree %g together with \"amg\": one preconditioner at a time", value);
        RAILS_REQUIRE(value == 0.0 || it->method == RAILS_ITER_CG,
                      "rails_iter_set: poly_degree %g on a BiCGStab object: the polynomial preconditioner is for conjugate gradients (a real spectrum)", value);
        it->poly_degree = (int)value;
    } else if (n == "poly_ratio") {
        RAILS_REQUIRE(value > 1.0, "rails_iter_set: poly_ratio %g is not above 1", value);
        it->poly_ratio = value;
    } else if (n == "eig_max") {
        RAILS_REQUIRE(value >= 0.0, "rails_iter_set: eig_max %g", value);
        it->eig_max = value;
    } else if (n == "poly_fused")
        it->poly_fused = value != 0.0;
    else if (n == "amg") {
        if (value != 0.0) RAILS_TRY(amg_check(it, "rails_iter_set"));
        it->amg = value != 0.0;
    } else if (n == "amg_degree") {
        RAILS_REQUIRE(value >= 0.0 && value <= 8.0 && value == std::floor(value), "rails_iter_set: amg_degree %g is not a whole number in 0 .. 8", value);
        it->amg_degree = (int)value;
    } else if (n == "amg_ratio") {
        RAILS_REQUIRE(value > 1.0, "rails_iter_set: amg_ratio %g is not above 1", value);
        it->amg_ratio = value;
    } else if (n == "amg_theta") {
        RAILS_REQUIRE(value >= 0.0 && value < 1.0, "rails_iter_set: amg_theta %g is not in [0, 1)", value);
        if (value != it->amg_theta) amg_release(it);
        it->amg_theta = value;
    } else if (n == "amg_coarse") {
        RAILS_REQUIRE(value >= 1.0 && value <= RAILS_AMG_MAX_COARSE && value == std::floor(value), "rails_iter_set: amg_coarse %g is not a whole number in 1 .. %d", value,
                      RAILS_AMG_MAX_COARSE);
        if ((int)value != it->amg_coarse) amg_release(it);
        it->amg_coarse = (int)value;
    } else {
        rails_set_error("rails_iter_set: no setting named '%s' (tolerance, max_iterations, jacobi, check_every, strict, poly_degree, poly_ratio, eig_max, poly_fused, amg, amg_degree, "
                        "amg_ratio, amg_theta, amg_coarse)", name);
        return RAILS_EINVAL;
    }
    return RAILS_OK;
}

// Builds (or rebuilds) the multigrid hierarchy from the CSR arrays the operator's handle keeps on the host and uploads it: the level operators, P and R = P' as rectangular operators, the inverse diagonals, the dense inverse.
extern "C" int rails_iter_amg_setup(rails_ctx *c, rails_iter *it)
{
    if (c) hipSetDevice(c->device);
    RAILS_REQUIRE(c && it, "rails_iter_amg_setup: null argument");
    RAILS_REQUIRE(c == it->ctx, "rails_iter_amg_setup: the object belongs to another context");
    RAILS_TRY(amg_check(it, "rails_iter_amg_setup"));
    amg_release(it);
    rails_csr *A = it->A;
    const int64_t m = it->m;
    // the CSR arrays every stored handle keeps on the host (rails_csr_create); a handle without them would need a copy back from the device
    RAILS_REQUIRE((int64_t)A->h_rowptr.size() == m + 1 && (int64_t)A->h_val.size() == A->h_rowptr[m] && A->h_col.size() == A->h_val.size(),
                  "rails_iter_amg_setup: the operator keeps no CSR arrays on the host to build the hierarchy from");
    const int64_t *rowptr = A->h_rowptr.data();
    const int32_t *col = A->h_col.data();
    const double *val = A->h_val.data();
    const auto t0 = std::chrono::steady_clock::now();
    rails_amg_hierarchy h;
    RAILS_TRY(rails_amg_build_host(m, rowptr, col, val, it->amg_theta, it->amg_coarse, &h));
    const auto t1 = std::chrono::steady_clock::now();
    Amg *H = new Amg;
    it->hier = H; // (released by amg_release, also when an upload below fails)
    H->n_coarse = h.coarse.n_rows;
    H->coarse_nnz = h.coarse.nnz();
    H->lv.resize(h.levels.size());
    int rc = RAILS_OK;
    hipError_t e = hipSuccess;
    for (size_t l = 0; l < h.levels.size() && rc == RAILS_OK && e == hipSuccess; ++l) {
        const rails_amg_level &S = h.levels[l];
        AmgLevel &L = H->lv[l];
        L.n = S.A.n_rows;
        L.nnz = S.A.nnz();
        L.hi = S.hi;
        if (l == 0)
            L.A = A;
        else
            rc = rails_csr_create(c, L.n, L.n, S.A.rowptr.data(), S.A.col.data(), S.A.val.data(), &L.A);
        if (rc == RAILS_OK) rc = rails_csr_create_rect(c, S.P.n_rows, S.P.n_cols, S.P.rowptr.data(), S.P.col.data(), S.P.val.data(), &L.P);
        if (rc == RAILS_OK) rc = rails_csr_create_rect(c, S.R.n_rows, S.R.n_cols, S.R.rowptr.data(), S.R.col.data(), S.R.val.data(), &L.R);
        if (rc == RAILS_OK) e = hipMalloc((void **)&L.dinv, (size_t)L.n * sizeof(double));
        if (rc == RAILS_OK && e == hipSuccess) e = hipMemcpy(L.dinv, S.dinv.data(), (size_t)L.n * sizeof(double), hipMemcpyHostToDevice);
    }
    if (rc == RAILS_OK && e == hipSuccess) e = hipMalloc((void **)&H->Ainv, h.coarse_inv.size() * sizeof(double));
    if (rc == RAILS_OK && e == hipSuccess) e = hipMemcpy(H->Ainv, h.coarse_inv.data(), h.coarse_inv.size() * sizeof(double), hipMemcpyHostToDevice);
    if (rc != RAILS_OK || e != hipSuccess) {
        if (rc == RAILS_OK) rails_set_error("rails_iter_amg_setup: device allocation or upload failed: %s", hipGetErrorString(e));
        amg_release(it);
        return rc != RAILS_OK ? rc : RAILS_EHIP;
    }
    H->host_seconds = std::chrono::duration<double>(t1 - t0).count();
    H->upload_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
    return RAILS_OK;
}

// The hierarchy by its matrices, the last (dense) one included: rows, entries and the Gershgorin bound hi of the smoother's interval (0 for
// the last) of matrix l in rows[l], nnz[l], hi[l], l < n.  Two more entries where cap allows: [n] the last call's cycles, the products
// inside them (with A_l, P and R) and the launches of the object's own kernels inside them; [n + 1] the set-up's host time and its upload
// time in microseconds, and in hi[n + 1] the operator complexity (the entries of all matrices over those of the first).  Returns n, 0
// when no hierarchy has been built; at most cap entries are written.
extern "C" int rails_iter_amg_info(const rails_iter *it, int64_t *rows, int64_t *nnz, double *hi, int cap)
{
    RAILS_REQUIRE(it && cap >= 0, "rails_iter_amg_info: bad argument");
    const Amg *H = it->hier;
    if (!H) return 0;
    const int n = (int)H->lv.size() + 1;
    double total = (double)H->coarse_nnz;
    for (const AmgLevel &L : H->lv) total += (double)L.nnz;
    for (int l = 0; l < n + 2 && l < cap; ++l) {
        int64_t r, z;
        double v;
        if (l < n - 1) {
            r = H->lv[(size_t)l].n;
            z = H->lv[(size_t)l].nnz;
            v = H->lv[(size_t)l].hi;
        } else if (l == n - 1) {
            r = H->n_coarse;
            z = H->coarse_nnz;
            v = 0.0;
        } else if (l == n) {
            r = it->last_cycles;
            z = it->last_cycle_products;
            v = (double)it->last_cycle_launches;
        } else {
            r = (int64_t)(H->host_seconds * 1e6);
            z = (int64_t)(H->upload_seconds * 1e6);
            v = total / (double)(H->lv.empty() ? H->coarse_nnz : H->lv[0].nnz);
        }
        if (rows) rows[l] = r;
        if (nnz) nnz[l] = z;
        if (hi) hi[l] = v;
    }
    return n;
}

namespace {

// before a solve or an application with "amg" on: the hierarchy when there is none yet, the level panels at the work panels' width
int amg_prepare(rails_ctx *c, rails_iter *it)
{
    if (!it->hier) RAILS_TRY(rails_iter_amg_setup(c, it));
    return amg_grow(c, it);
}

} // namespace

extern "C" int rails_iter_solve(rails_ctx *c, rails_iter *it, int trans, const rails_panel *X, int xc0, int nc, rails_panel *Y, int yc0)
{
    if (c) hipSetDevice(c->device);
    rails_slow_guard slow__(c, "rails_iter_solve", nc, it ? it->m : 0);
    RAILS_REQUIRE(c && it && X && Y, "rails_iter_solve: null argument");
    RAILS_REQUIRE(c == it->ctx, "rails_iter_solve: the object belongs to another context");
    // Collective on a context that reduces.  The rule that keeps the ranks from deadlocking: every decision that changes how many
    // collectives are issued -- a refusal, the group loop, the number of iterations queued, the early exit, the non-finite right-hand side's
    // RAILS_EINVAL -- is a function of the arguments and settings every rank passes alike (nc, trans, max_iterations, check_every) and of
    // all-reduced data (the columns' scalars and the counts in `status`, the same bits on every rank), never of this rank's rows.
    RAILS_REQUIRE(!trans || (it->A->n_ghost == 0 && it->A->n_send == 0 && it->A->ncols_ext == it->A->m),
                  "rails_iter_solve: the transposed solve of a row-partitioned operator (ghost rows) is not available: rails_spmm's transposed product is single GPU");
    RAILS_REQUIRE(X->m == it->m && Y->m == it->m, "rails_iter_solve: the operator has %lld rows, X %lld, Y %lld", (long long)it->m, (long long)X->m,
                  (long long)Y->m);
    RAILS_REQUIRE(xc0 >= 0 && nc >= 0 && xc0 + nc <= X->cap && yc0 >= 0 && yc0 + nc <= Y->cap, "rails_iter_solve: column windows outside the panels");
    if (X->d == Y->d) RAILS_REQUIRE(xc0 + nc <= yc0 || yc0 + nc <= xc0, "rails_iter_solve: X and Y windows alias");
    it->last_dots = it->last_launches = it->last_products = it->last_poly = it->last_fused = it->last_allreduces = it->last_halo = 0;
    it->last_cycles = it->last_cycle_products = it->last_cycle_launches = 0;
    it->last.clear();
    if (nc == 0) return RAILS_OK;
    RAILS_TRY(grow_work(c, it, std::min(nc, RAILS_ITER_GROUP)));
    if (it->amg) RAILS_TRY(amg_prepare(c, it));
    RAILS_TRY(grow_cols(c, it, nc));
    int32_t *status = (int32_t *)it->pinned;
    Run run;
    run.c = c;
    run.it = it;
    run.trans = trans ? 1 : 0;
    run.jac = it->jacobi && it->dinv;
    run.tol2 = it->tol * it->tol;
    RAILS_TRY(poly_setup(run, "rails_iter_solve"));
    run.amg = it->amg != 0;
    for (int g0 = 0; g0 < nc; g0 += RAILS_ITER_GROUP) {
        const int w = std::min(RAILS_ITER_GROUP, nc - g0);
        set_group(run, w);
        run.cols = it->cols_dev + g0;
        RAILS_TRY(rails_panel_copy(c, X, xc0 + g0, w, it->w[W_R], 0));
        RAILS_TRY(run.start());
        for (int queued = 0, first = 1;; first = 0) {
            const int n = std::max(0, std::min(it->check_every, it->maxit - queued));
            for (int k = 0; k < n; ++k) RAILS_TRY(run.iteration());
            queued += n;
            RAILS_HIP_CHECK(hipGetLastError());
            RAILS_HIP_CHECK(hipMemcpyAsync(status, it->status_dev, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
            RAILS_HIP_CHECK(rails_stream_sync(c));
            if (first && status[1] > 0) {
                rails_set_error("rails_iter_solve: %d column(s) of the right-hand side in columns [%d, %d) are not finite", (int)status[1], g0, g0 + w);
                return RAILS_EINVAL;
            }
            if (status[0] == 0 || queued >= it->maxit) break;
        }
        RAILS_TRY(rails_panel_copy(c, it->w[W_X], 0, w, Y, yc0 + g0));
    }
    rails_iter_col *host_cols = (rails_iter_col *)((char *)it->pinned + 64);
    RAILS_HIP_CHECK(hipMemcpyAsync(host_cols, it->cols_dev, (size_t)nc * sizeof(rails_iter_col), hipMemcpyDeviceToHost, c->stream));
    RAILS_HIP_CHECK(rails_stream_sync(c));
    it->last.assign(host_cols, host_cols + nc);
    int flagged = 0;
    for (const rails_iter_col &col : it->last) {
        it->tot_iterations += col.iter;
        flagged += (col.flags & RAILS_ITER_CONVERGED) ? 0 : 1;
    }
    it->tot_solves += 1;
    it->tot_columns += nc;
    it->tot_flagged += flagged;
    it->tot_products += it->last_products;
    if (flagged && it->strict) {
        rails_set_error("rails_iter_solve: %d of %d columns did not reach the tolerance %g (strict)", flagged, nc, it->tol);
        return RAILS_ENOCONV;
    }
    return RAILS_OK;
}

// Y = p_K(G A) G X, the preconditioner the CG solve applies to its residual, on its own: a fixed linear approximate inverse.  K = 0: G X.
extern "C" int rails_iter_precondition(rails_ctx *c, rails_iter *it, const rails_panel *X, int xc0, int nc, rails_panel *Y, int yc0)
{
    if (c) hipSetDevice(c->device);
    RAILS_REQUIRE(c && it && X && Y, "rails_iter_precondition: null argument");
    RAILS_REQUIRE(c == it->ctx, "rails_iter_precondition: the object belongs to another context");
    RAILS_REQUIRE(X->m == it->m && Y->m == it->m, "rails_iter_precondition: the operator has %lld rows, X %lld, Y %lld", (long long)it->m, (long long)X->m,
                  (long long)Y->m);
    RAILS_REQUIRE(xc0 >= 0 && nc >= 0 && xc0 + nc <= X->cap && yc0 >= 0 && yc0 + nc <= Y->cap, "rails_iter_precondition: column windows outside the panels");
    if (X->d == Y->d) RAILS_REQUIRE(xc0 + nc <= yc0 || yc0 + nc <= xc0, "rails_iter_precondition: X and Y windows alias");
    it->last_dots = it->last_launches = it->last_products = it->last_poly = it->last_fused = it->last_allreduces = it->last_halo = 0; // the counters count this call
    it->last_cycles = it->last_cycle_products = it->last_cycle_launches = 0;
    if (nc == 0) return RAILS_OK;
    unsigned want = 1u << W_R | 1u << W_Z | 1u << W_D;
    if (it->poly_degree > 0 || it->amg) want |= 1u << W_Z2 | 1u << W_Q;
    RAILS_TRY(grow_work(c, it, std::min(nc, RAILS_ITER_GROUP), want));
    if (it->amg) RAILS_TRY(amg_prepare(c, it));
    Run run;
    run.c = c;
    run.it = it;
    run.trans = 0;
    run.jac = it->jacobi && it->dinv;
    run.tol2 = 0.0;
    run.cols = nullptr;
    RAILS_TRY(poly_setup(run, "rails_iter_precondition"));
    run.amg = it->amg != 0;
    for (int g0 = 0; g0 < nc; g0 += RAILS_ITER_GROUP) {
        const int w = std::min(RAILS_ITER_GROUP, nc - g0);
        set_group(run, w);
        RAILS_TRY(rails_panel_copy(c, X, xc0 + g0, w, it->w[W_R], 0));
        RAILS_TRY(run.precondition());
        RAILS_TRY(rails_panel_copy(c, it->w[W_Z], 0, w, Y, yc0 + g0));
    }
    RAILS_HIP_CHECK(hipGetLastError());
    return RAILS_OK;
}

// info[0] most iterations of a column in the last solve, [1] inner products of the last solve (per column and quantity), [2] kernel
// launches of the library's own passes in it, [3] its columns that did not converge (any flag but converged), [4] those of them that
// broke down, [5] worst relative residual of the recurrence, [6] work-panel columns, [7] products with A in the last solve; totals since
// creation: [8] solves, [9] columns, [10] iterations summed over the columns, [11] flagged columns, [12] products with A; the polynomial
// preconditioner: [13] its applications in the last solve, [14] launches of the fused step kernel in it, [15] hi and [16] lo of the
// interval in use (0 with degree 0); a context that reduces: [17] all-reduces issued in the last call (per group of columns CG 1 at the start
// and 2 per queued iteration, BiCGStab 1 and 3; the polynomial adds none), [18] ghost-row exchanges the object issued itself (one before
// every fused step in its ghost-row form; those inside rails_spmm are not counted).  [7] counts every product, those inside the fused step
// included.
extern "C" int rails_iter_stats(const rails_iter *it, double *info, int cap)
{
    RAILS_REQUIRE(it && info && cap >= 0, "rails_iter_stats: bad argument");
    double most = 0, unconv = 0, broke = 0, worst = 0;
    for (const rails_iter_col &c : it->last) {
        most = std::max(most, (double)c.iter);
        if (!(c.flags & RAILS_ITER_CONVERGED)) unconv += 1;
        if (c.flags & RAILS_ITER_BREAKDOWN) broke += 1;
        const double rel = c.bb > 0.0 ? std::sqrt(c.rr / c.bb) : 0.0;
        if (!(rel <= worst)) worst = rel; // a NaN shows
    }
    const double hi = it->poly_degree > 0 ? poly_hi(it) : 0.0;
    const double v[19] = {most, (double)it->last_dots, (double)it->last_launches, unconv, broke, worst, (double)it->work_cols, (double)it->last_products,
                          it->tot_solves, it->tot_columns, it->tot_iterations, it->tot_flagged, it->tot_products,
                          (double)it->last_poly, (double)it->last_fused, hi, hi / it->poly_ratio, (double)it->last_allreduces, (double)it->last_halo};
    const int k = std::min(cap, 19);
    for (int i = 0; i < k; ++i) info[i] = v[i];
    return k;
}

// per column of the last solve: iterations, relative residual of the recurrence, flags (RAILS_ITER_* of iter_scalars.h: 2 converged,
// 4 stopped at max_iterations, 8 breakdown, 16 non-finite).  Returns the number of columns of the last solve; at most cap are written.
extern "C" int rails_iter_columns(const rails_iter *it, int32_t *iterations, double *relres, int32_t *flags, int cap)
{
    RAILS_REQUIRE(it && cap >= 0, "rails_iter_columns: bad argument");
    const int n = (int)it->last.size();
    for (int j = 0; j < std::min(n, cap); ++j) {
        const rails_iter_col &c = it->last[j];
        if (iterations) iterations[j] = c.iter;
        if (relres) relres[j] = c.bb > 0.0 ? std::sqrt(c.rr / c.bb) : 0.0;
        if (flags) flags[j] = c.flags;
    }
    return n;
}

extern "C" int rails_csr_create_iter(rails_ctx *c, rails_iter *it, rails_csr **out)
{
    RAILS_REQUIRE(c && it && out, "rails_csr_create_iter: null argument");
    RAILS_REQUIRE(c == it->ctx, "rails_csr_create_iter: the object belongs to another context");
    rails_csr *A = new rails_csr();
    A->ctx = c;
    A->m = it->m;
    A->ncols_ext = it->m;
    A->kind = rails_csr::ITER;
    A->delegate = it;
    A->last_kernel = it->method == RAILS_ITER_CG ? "iter_cg" : "iter_bicgstab";
    *out = A;
    return RAILS_OK;
}
