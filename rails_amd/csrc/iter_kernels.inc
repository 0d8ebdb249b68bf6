// iter_kernels.inc -- the device code of the iterative A^-1 operator, included by itsolve.hip inside its anonymous namespace (one translation
// unit, as with lanczos_pass.inc and dense_gram.inc): the shape every pass shares, the passes of CG and BiCGStab, the Chebyshev sweep
// (init, unfused pass, the fused step on the shared row gather of csr_row_gather.inc), the multigrid cycle's own kernels, the scalar
// step, the block forms of the passes that apply the preconditioner when it is block Jacobi and, at the end, the block multigrid cycle's kernels.  PassGeom is iter_geom.h's rails_pass_geom; itsolve.hip's head comment says what the passes are.
typedef double it_v2 __attribute__((ext_vector_type(2)));

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
template <int NQ>
__device__ __forceinline__ void iter_pass_sums(const PassGeom &g, double *__restrict__ partial, const it_v2 *acc);

template <int NQ, class Body>
__device__ __forceinline__ void iter_pass(const PassGeom &g, double *__restrict__ partial, Body body)
{
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
    iter_pass_sums<NQ>(g, partial, acc);
}

// The end of a pass that sums: the TY row classes' NQ sums per column meet in an LDS tree of fixed shape, and row class 0 writes the
// block's partial sums.  Shared by the point form above and the block form (iter_pass_block).
template <int NQ>
__device__ __forceinline__ void iter_pass_sums(const PassGeom &g, double *__restrict__ partial, const it_v2 *acc)
{
    __shared__ double sh[NQ > 0 ? NQ : 1][256][2];
    const int TX = 1 << g.tx_bits, TY = 256 >> g.tx_bits;
    const int tx = threadIdx.x & (TX - 1), ty = threadIdx.x >> g.tx_bits;
    const int c = 2 * tx;
    const bool has0 = c < g.ncw, has1 = c + 1 < g.ncw;
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

// ---- the multigrid cycle's own kernels (DESIGN.md section 16).  All panels are work panels: window at column 0, one row stride ld, rows
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

// ---- block Jacobi (DESIGN.md section 18): z = G r with G the inverses of the b x b diagonal blocks, ginv[block][i][j] row-major, in the
// passes that apply dinv[row] in the point form.  RAILS_BJ_TABLE is the list of block sizes compiled; the launching switches of itsolve.hip
// expand from it. ----
#define RAILS_BJ_TABLE(X) X(2) X(3) X(4) X(5) X(6) X(7) X(8)

struct bj_row {
    it_v2 r, aux; // the row's entry of the vector G applies to, and what else the pass formed from its loads (k_cg_update_bj: x)
};

// The block form of iter_pass.  A thread owns a column pair and every TY-th BLOCK row of its block's slab (g.rows_per_slab is a multiple
// of B, rails_iter_pass_geom_block).  For one block row it calls load(offset) for the B rows -- every load of the pass is in there, and it
// stores nothing -- then forms z_i = sum_j G[i][j] r_j (TRANS: G[j][i]), one accumulator from +0 and one fma per j, j ascending, and
// calls emit(offset, has1, row i's loads, z_i, acc) for the stores and the sums.  The trip count of the row loop is the same for every
// thread of the block and the loads are unconditional (lanczos_pass.inc's rule): a thread past the slab's last block row loads that last
// block row again and emits nothing.  All lanes of a row class read the inverse block at one address.
template <int B, int NQ, bool TRANS, class Load, class Emit>
__device__ __forceinline__ void iter_pass_block(const PassGeom &g, const double *__restrict__ ginv, double *__restrict__ partial, Load load, Emit emit)
{
    const int TX = 1 << g.tx_bits, TY = 256 >> g.tx_bits;
    const int tx = threadIdx.x & (TX - 1), ty = threadIdx.x >> g.tx_bits;
    const int c = 2 * tx;
    const bool has0 = c < g.ncw, has1 = c + 1 < g.ncw;
    const int64_t nb = g.m / B, bps = g.rows_per_slab / B;
    const int64_t b_begin = (int64_t)blockIdx.x * bps;
    const int64_t b_end = b_begin + bps < nb ? b_begin + bps : nb;
    it_v2 acc[NQ > 0 ? NQ : 1];
#pragma unroll
    for (int q = 0; q < (NQ > 0 ? NQ : 1); ++q) acc[q] = (it_v2){0.0, 0.0};
    if (has0) {
        for (int64_t base = b_begin; base < b_end; base += TY) {
            const bool live = base + ty < b_end;
            const int64_t br = live ? base + ty : b_end - 1;
            const int64_t o = br * B * g.ld + c;
            const double *__restrict__ gb = ginv + br * (B * B);
            bj_row in[B];
#pragma unroll
            for (int i = 0; i < B; ++i) in[i] = load(o + (int64_t)i * g.ld);
#pragma unroll
            for (int i = 0; i < B; ++i) {
                it_v2 z = (it_v2){0.0, 0.0};
#pragma unroll
                for (int j = 0; j < B; ++j) {
                    const double v = TRANS ? gb[j * B + i] : gb[i * B + j];
                    z.x = __builtin_fma(v, in[j].r.x, z.x);
                    z.y = __builtin_fma(v, in[j].r.y, z.y);
                }
                if (live) emit(o + (int64_t)i * g.ld, has1, in[i], z, acc);
            }
        }
    }
    if (NQ == 0) return;
    iter_pass_sums<NQ>(g, partial, acc);
}

// k_cg_init<true> with blocks: z = G r, p = z, x = 0; partial sums of r.z and r.r
template <int B>
__global__ __launch_bounds__(256) void k_cg_init_bj(PassGeom g, const double *__restrict__ ginv, const double *__restrict__ R, double *__restrict__ Z,
                                                    double *__restrict__ P, double *__restrict__ Xw, double *__restrict__ partial)
{
    iter_pass_block<B, 2, false>(
        g, ginv, partial, [&](int64_t o) { return bj_row{ld2(R + o), (it_v2){0.0, 0.0}}; },
        [&](int64_t o, bool has1, const bj_row &in, it_v2 z, it_v2 *acc) {
            st2(Z + o, z, has1);
            st2(P + o, z, has1);
            st2(Xw + o, (it_v2){0.0, 0.0}, has1);
            acc[0] += in.r * z;
            acc[1] += in.r * in.r;
        });
}

// k_cg_update<true> with blocks: x += alpha p, r -= alpha q, z = G r; partial sums of r.z and r.r
template <int B>
__global__ __launch_bounds__(256) void k_cg_update_bj(PassGeom g, const rails_iter_col *__restrict__ cols, const double *__restrict__ ginv,
                                                      const double *__restrict__ P, const double *__restrict__ Q, double *__restrict__ Xw,
                                                      double *__restrict__ R, double *__restrict__ Z, double *__restrict__ partial)
{
    ITER_COEF(alpha, alpha);
    iter_pass_block<B, 2, false>(
        g, ginv, partial, [&](int64_t o) { return bj_row{axpy_sel(-alpha, ld2(Q + o), ld2(R + o)), axpy_sel(alpha, ld2(P + o), ld2(Xw + o))}; },
        [&](int64_t o, bool has1, const bj_row &in, it_v2 z, it_v2 *acc) {
            st2(Xw + o, in.aux, has1);
            st2(R + o, in.r, has1);
            st2(Z + o, z, has1);
            acc[0] += in.r * z;
            acc[1] += in.r * in.r;
        });
}

// k_bi_dir<true> with blocks: p = r + beta (p - omega v), p^ = G p (TRANS: G')
template <int B, bool TRANS>
__global__ __launch_bounds__(256) void k_bi_dir_bj(PassGeom g, const rails_iter_col *__restrict__ cols, const double *__restrict__ ginv,
                                                   const double *__restrict__ R, const double *__restrict__ V, double *__restrict__ P,
                                                   double *__restrict__ PH)
{
    ITER_COEF(beta, beta);
    ITER_COEF(omega, omega);
    iter_pass_block<B, 0, TRANS>(
        g, ginv, nullptr, [&](int64_t o) { return bj_row{axpy_sel(beta, axpy_sel(-omega, ld2(V + o), ld2(P + o)), ld2(R + o)), (it_v2){0.0, 0.0}}; },
        [&](int64_t o, bool has1, const bj_row &in, it_v2 z, it_v2 *) {
            st2(P + o, in.r, has1);
            st2(PH + o, z, has1);
        });
}

// k_bi_s<true> with blocks: s = r - alpha v (kept in R), s^ = G s (TRANS: G')
template <int B, bool TRANS>
__global__ __launch_bounds__(256) void k_bi_s_bj(PassGeom g, const rails_iter_col *__restrict__ cols, const double *__restrict__ ginv,
                                                 const double *__restrict__ V, double *__restrict__ R, double *__restrict__ SH)
{
    ITER_COEF(alpha, alpha);
    iter_pass_block<B, 0, TRANS>(
        g, ginv, nullptr, [&](int64_t o) { return bj_row{axpy_sel(-alpha, ld2(V + o), ld2(R + o)), (it_v2){0.0, 0.0}}; },
        [&](int64_t o, bool has1, const bj_row &in, it_v2 z, it_v2 *) {
            st2(R + o, in.r, has1);
            st2(SH + o, z, has1);
        });
}

// Z = G R: the preconditioner on its own (rails_iter_precondition with block Jacobi in effect)
template <int B>
__global__ __launch_bounds__(256) void k_bj_apply(PassGeom g, const double *__restrict__ ginv, const double *__restrict__ R, double *__restrict__ Z)
{
    iter_pass_block<B, 0, false>(
        g, ginv, nullptr, [&](int64_t o) { return bj_row{ld2(R + o), (it_v2){0.0, 0.0}}; },
        [&](int64_t o, bool has1, const bj_row &, it_v2 z, it_v2 *) { st2(Z + o, z, has1); });
}

// ---- the block multigrid cycle (DESIGN.md section 19): the Chebyshev sweep with G the inverses of the diagonal blocks of a block-CSR
// level matrix.  The fused step and the residual run on the block-row body k_spmm_bsr runs on (bsr_row_gather.inc): the lanes that own a
// block row hold all B rows of A z for their two columns, so G (r - A z) is register-local.  Instantiations and launching switches expand
// from RAILS_BSR_TABLE (bsr_choice.h) and RAILS_BJ_TABLE; which step a level takes is block_amg_choice.h's. ----
#include "bsr_row_gather.inc"

// The step's epilogue for one block row and one column pair at offset o (row stride ld) of the work panels, from t = (A Zin) of the B
// rows: u_j = R_j - t_j; then row by row w_i = sum_j G[i][j] u_j (one accumulator from +0, one fma per j, j ascending: iter_pass_block's
// rule), d_i = fma(a, D_i, b w_i) stored in place, Zout_i = Zin_i + d_i.  gb: the block's inverse, every lane of a group at one address.
// The fused step and the unfused pass both end here.
template <int B>
__device__ __forceinline__ void cheb_block_epilogue(const double *__restrict__ gb, it_v2 (&t)[B], const double *__restrict__ R, double *__restrict__ D,
                                                    const double *Zin, double *Zout, int64_t o, int64_t ld, double a, double b, bool full)
{
#pragma unroll
    for (int j = 0; j < B; ++j) t[j] = ld2(R + o + j * ld) - t[j];
#pragma unroll
    for (int i = 0; i < B; ++i) {
        it_v2 w = (it_v2){0.0, 0.0};
#pragma unroll
        for (int j = 0; j < B; ++j) {
            const double v = gb[i * B + j];
            w.x = __builtin_fma(v, t[j].x, w.x);
            w.y = __builtin_fma(v, t[j].y, w.y);
        }
        const it_v2 dold = ld2(D + o + i * ld);
        it_v2 d;
        d.x = __builtin_fma(a, dold.x, b * w.x);
        d.y = __builtin_fma(a, dold.y, b * w.y);
        st2(D + o + i * ld, d, full);
        st2(Zout + o + i * ld, ld2(Zin + o + i * ld) + d, full);
    }
}

// the accumulators of the shared body as the pair at the lane's own column: the lane of an odd last column holds its column's value in .y
// (.x for a panel of one column); its second entry is the pad column's, read and never written
template <int B>
__device__ __forceinline__ void bsr_own_pair(const bsr_v2 (&acc)[B], bool full, bool one, it_v2 (&t)[B])
{
#pragma unroll
    for (int r = 0; r < B; ++r) {
        t[r].x = (full || one) ? acc[r].x : acc[r].y;
        t[r].y = acc[r].y;
    }
}

// The fused step on a block-CSR level matrix.  Zin and Zout are different panels (every workgroup reads rows of Zin that others own); all
// panels are work panels: window at column 0, one row stride, rows 16-byte aligned, a pad column beside an odd width.
template <int B, int LPR>
__global__ __launch_bounds__(rails_bsr_threads(B)) void k_cheb_step_bsr(int64_t mb, const int64_t *__restrict__ browptr, const int32_t *__restrict__ bcol,
                                                                        const double *__restrict__ bval, const double *__restrict__ Zin, int ld, int nc, int rpg,
                                                                        int64_t blocks_per_xcd, const double *__restrict__ ginv, double a, double b,
                                                                        const double *__restrict__ R, double *__restrict__ D, double *__restrict__ Zout)
{
    bsr_row_gather<B, LPR>(mb, browptr, bcol, bval, Zin, ld, nc, rpg, blocks_per_xcd, [&](int64_t brow, int cb, const bsr_v2 (&acc)[B], bool full, bool one) {
        it_v2 t[B];
        bsr_own_pair<B>(acc, full, one, t);
        cheb_block_epilogue<B>(ginv + brow * (B * B), t, R, D, Zin, Zout, brow * B * (int64_t)ld + cb, ld, a, b, full);
    });
}

// Q = R - A Z on the shared body
template <int B, int LPR>
__global__ __launch_bounds__(rails_bsr_threads(B)) void k_amg_residual_bsr(int64_t mb, const int64_t *__restrict__ browptr, const int32_t *__restrict__ bcol,
                                                                           const double *__restrict__ bval, const double *__restrict__ Z, int ld, int nc, int rpg,
                                                                           int64_t blocks_per_xcd, const double *__restrict__ R, double *__restrict__ Q)
{
    bsr_row_gather<B, LPR>(mb, browptr, bcol, bval, Z, ld, nc, rpg, blocks_per_xcd, [&](int64_t brow, int cb, const bsr_v2 (&acc)[B], bool full, bool one) {
        it_v2 t[B];
        bsr_own_pair<B>(acc, full, one, t);
        const int64_t o = brow * B * (int64_t)ld + cb;
#pragma unroll
        for (int r = 0; r < B; ++r) st2(Q + o + r * (int64_t)ld, ld2(R + o + r * (int64_t)ld) - t[r], full);
    });
}

// d = z = (G r) / theta, the sweep's start with blocks
template <int B>
__global__ __launch_bounds__(256) void k_cheb_init_bj(PassGeom g, const double *__restrict__ ginv, double theta, const double *__restrict__ R, double *__restrict__ D,
                                                      double *__restrict__ Z)
{
    iter_pass_block<B, 0, false>(
        g, ginv, nullptr, [&](int64_t o) { return bj_row{ld2(R + o), (it_v2){0.0, 0.0}}; },
        [&](int64_t o, bool has1, const bj_row &, it_v2 z, it_v2 *) {
            const it_v2 d = z / theta;
            st2(D + o, d, has1);
            st2(Z + o, d, has1);
        });
}

// The unfused step with blocks, after Q = A Z: iter_pass_block's walk over the block rows of a slab (the same trip count for every thread
// of the block, a thread past the slab's last block row loads that block row again and stores nothing), its loads those of the B rows of
// Q, then the fused step's own epilogue, in place in Z.
template <int B>
__global__ __launch_bounds__(256) void k_cheb_pass_bj(PassGeom g, const double *__restrict__ ginv, double a, double b, const double *__restrict__ Q,
                                                      const double *__restrict__ R, double *__restrict__ D, double *__restrict__ Z)
{
    const int TX = 1 << g.tx_bits, TY = 256 >> g.tx_bits;
    const int tx = threadIdx.x & (TX - 1), ty = threadIdx.x >> g.tx_bits;
    const int c = 2 * tx;
    if (c >= g.ncw) return;
    const bool has1 = c + 1 < g.ncw;
    const int64_t nb = g.m / B, bps = g.rows_per_slab / B;
    const int64_t b_begin = (int64_t)blockIdx.x * bps;
    const int64_t b_end = b_begin + bps < nb ? b_begin + bps : nb;
    for (int64_t base = b_begin; base < b_end; base += TY) {
        const bool live = base + ty < b_end;
        const int64_t br = live ? base + ty : b_end - 1;
        const int64_t o = br * B * g.ld + c;
        it_v2 t[B];
#pragma unroll
        for (int i = 0; i < B; ++i) t[i] = ld2(Q + o + (int64_t)i * g.ld);
        if (live) cheb_block_epilogue<B>(ginv + br * (B * B), t, R, D, Z, Z, o, g.ld, a, b, has1);
    }
}
