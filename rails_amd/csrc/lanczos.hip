// lanczos.hip -- fused residual Lanczos (src/LyapunovSolver.hpp:367-447) for gfx950.
//
// Lanczos on the implicit symmetric operator  R = AV T MV^T + MV T AV^T + B B^T  (MV == V when
// M = I).  The reference makes 4 passes over the m x k panels per step (V^T q, AV Z, AV^T q, V Z)
// plus B, alpha, beta and axpy passes.  Here ONE pass over P = [AV MV B] does a whole step:
//
//   with c = P^T q_i known (from the previous pass):   g = [T c_MV ; T c_AV ; c_B]
//        alpha_i = q_i^T R q_i = c_AV.g_AV + c_MV.g_MV + c_B.c_B           (no pass needed)
//   pass i, per row:   r = P_row . g - alpha_i q_i - beta_{i-1} q_{i-1}     (= un-normalised q_{i+1})
//                      c' += P_row * r ;  rr += r*r                          (row-local, same pass)
//   then               beta_i = sqrt(rr),  c_{next} = c' / beta_i.
//
// HBM traffic per step = (2k + p + ~4) * m * 8 bytes: the compulsory single read of the panels.
// The Lanczos vectors live in a column-major side buffer (one contiguous vector per step) so the
// per-row scalar traffic is coalesced.  alpha, beta and the breakdown test (beta < 1e-14,
// :419-426) stay on the device; the host reads H back once at the end.
#include "rails_internal.h"

#include "lanczos_plan.h"

#include <algorithm>
#include <cmath>

struct rails_lanczos_state {
    double *Qc = nullptr; // (L+2) vectors of length mpad, column-major
    size_t qc_bytes = 0;
    int64_t m = 0, mpad = 0;
    int steps = 0;
    int L = 0;
    double *small = nullptr; // T, coefficients, reduced sums, state, alphas, betas
    size_t small_bytes = 0;
    int last_nch = 0, last_unroll = 0, last_nblocks = 0; // what the last run launched (rails_lanczos_last_launch)
};

// one state per context: the Lanczos vectors of the context's last run (several contexts may live in one process,
// e.g. one per thread in the single-GPU rank emulation of tests/test_gpu_partition.py)
static rails_lanczos_state &lz_state(rails_ctx *c)
{
    if (!c->lz) c->lz = new rails_lanczos_state();
    return *static_cast<rails_lanczos_state *>(c->lz);
}

namespace {

typedef double v2f64 __attribute__((ext_vector_type(2)));

template <int CTRL>
__device__ __forceinline__ double dpp_f64(double x)
{
    int lo = __double2loint(x), hi = __double2hiint(x);
    lo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xF, 0xF, false);
    hi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double readlane_f64(double x, int lane)
{
    int lo = __builtin_amdgcn_readlane(__double2loint(x), lane);
    int hi = __builtin_amdgcn_readlane(__double2hiint(x), lane);
    return __hiloint2double(hi, lo);
}

// 64-lane sum, result uniform; fixed association: quads, 8s, 16s by DPP, then the four rows.
__device__ __forceinline__ double wave_sum(double x)
{
    x += dpp_f64<0xB1>(x);  // quad_perm [1,0,3,2]
    x += dpp_f64<0x4E>(x);  // quad_perm [2,3,0,1]
    x += dpp_f64<0x141>(x); // row_half_mirror
    x += dpp_f64<0x140>(x); // row_mirror
    double s0 = readlane_f64(x, 0), s1 = readlane_f64(x, 16), s2 = readlane_f64(x, 32), s3 = readlane_f64(x, 48);
    return (s0 + s1) + (s2 + s3);
}

struct LzArgs {
    const double *AV;
    int ldav;
    const double *MV;
    int ldmv;
    const double *B;
    int ldb;
    int k, p;
    int av_room, mv_room, b_room; // doubles readable from the window start to the end of the padded row
    int64_t m, mpad;
    double *Qc;
    int step;             // -1 = init pass (r := raw q_0)
    const double *coef;   // [k (for AV) | k (for MV) | p (for B)]
    const double *state;  // the slots of lz::State
    double *partial;      // [nblocks][2k+p+1]
};

// B as a sparse right-hand side (rails_sprhs): the CSR form of B for the pass, g_B = coef + 2k (p doubles, read-only for the pass)
struct LzSparse {
    const int64_t *rowptr;
    const int32_t *col;
    const double *val;
    const double *gB;
};
struct LzNoSparse {
};

// B's part of the rows of one 64-row group, sum_q B_val[q] g_B[B_col[q]], row row0 + l in lane l.  Rows of at most RAILS_SPRHS_SHORT
// entries are summed by their own lane, entry by entry; a longer row by the whole wave, 64 strands and wave_sum.  The loads are
// unconditional (masked lanes read entry 0, which exists whenever a loop runs), the loop bounds wave-uniform.
__device__ __forceinline__ double sparse_rows(const LzSparse &sp, int64_t row0, int nrows, int lane)
{
    const int64_t rl = row0 + (lane < nrows ? lane : 0);
    const int64_t s0 = sp.rowptr[rl];
    const int len = lane < nrows ? (int)(sp.rowptr[rl + 1] - s0) : 0;
    const int lshort = len <= RAILS_SPRHS_SHORT ? len : 0;
    double sB = 0.0;
    for (int t = 0; __builtin_amdgcn_ballot_w64(t < lshort) != 0; t += 4) { // four entries in flight, added in their order
        double v[4], gv[4];
        int32_t ci[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t idx = t + u < lshort ? s0 + t + u : 0;
            v[u] = sp.val[idx];
            ci[u] = sp.col[idx];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) gv[u] = sp.gB[ci[u]];
#pragma unroll
        for (int u = 0; u < 4; ++u) sB = t + u < lshort ? __builtin_fma(v[u], gv[u], sB) : sB;
    }
    uint64_t longs = __builtin_amdgcn_ballot_w64(len > RAILS_SPRHS_SHORT);
    while (longs != 0) {
        const int l = __builtin_ctzll(longs);
        longs &= longs - 1;
        const int n = __builtin_amdgcn_readlane(len, l);
        const int64_t b = ((int64_t)__builtin_amdgcn_readlane((int)(s0 >> 32), l) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)s0, l);
        double acc = 0.0;
        for (int e0 = 0; e0 < n; e0 += 64) {
            const bool on = e0 + lane < n;
            const int64_t idx = on ? b + e0 + lane : 0;
            const double v = sp.val[idx];
            const double gv = sp.gB[sp.col[idx]];
            acc = on ? __builtin_fma(v, gv, acc) : acc;
        }
        const double tot = wave_sum(acc);
        sB = lane == l ? tot : sB;
    }
    return sB;
}
__device__ __forceinline__ double sparse_rows(const LzNoSparse &, int64_t, int, int) { return 0.0; }

// lane l owns column pairs (2(l+64c), 2(l+64c)+1), c < NCH, of AV and of MV, and pair l of B.  The body is lanczos_pass.inc, shared with
// the sparse form below.
template <int NCH, int U>
__global__ __launch_bounds__(256) void k_lanczos_pass(LzArgs a)
{
    constexpr bool SP = false;
    const LzNoSparse sp{};
#include "lanczos_pass.inc"
}

// the pass of rails_resid_lanczos_sparse: partials of 2k + 1 entries [c'_AV | c'_MV | rr]
template <int NCH, int U>
__global__ __launch_bounds__(256) void k_lanczos_pass_sparse(LzArgs a, LzSparse sp)
{
    constexpr bool SP = true;
#include "lanczos_pass.inc"
}

// out[e] = sum over the blocks' partials, fixed order (16 interleaved strands, then strands 0..15); LAST_AT: the last entry (rr) goes to
// out[last_at] instead, behind the p entries of c'_B that the partials of the sparse form do not hold
template <bool LAST_AT>
__device__ __forceinline__ void lz_reduce_body(const double *__restrict__ partial, int nblocks, int n, double *__restrict__ out, int last_at)
{
    __shared__ double sh[16][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int e = blockIdx.x * 64 + tx;
    double s = 0.0;
    if (e < n)
        for (int t = ty; t < nblocks; t += 16) s += partial[(int64_t)t * n + e];
    sh[ty][tx] = s;
    __syncthreads();
    if (ty == 0 && e < n) {
        double r = 0.0;
#pragma unroll
        for (int g = 0; g < 16; ++g) r += sh[g][tx];
        out[(LAST_AT && e == n - 1) ? last_at : e] = r;
    }
}

__global__ __launch_bounds__(1024) void k_lz_reduce(const double *__restrict__ partial, int nblocks, int n, double *__restrict__ out)
{
    lz_reduce_body<false>(partial, nblocks, n, out, 0);
}

__global__ __launch_bounds__(1024) void k_lz_reduce_last_at(const double *__restrict__ partial, int nblocks, int n, double *__restrict__ out,
                                                            int last_at)
{
    lz_reduce_body<true>(partial, nblocks, n, out, last_at);
}

// c'_B = B'r over the transposed CSR form, balanced by nonzeros, no atomics (rails_internal.h: rails_sprhs).  Blocks [0, nshort): one
// thread per transposed row of at most RAILS_SPRHS_SHORT entries, summed in order into out[row]; the blocks behind them: one wave per item
// of a long row, 64 strands and wave_sum into item_partial.  k_sprhs_bt_long then adds a long row's items, again 64 strands and wave_sum.
struct LzBt {
    const int64_t *t_rowptr;
    const int32_t *t_col;
    const double *t_val;
    int p, nshort;
    const int64_t *item_beg;
    const int32_t *item_len;
    int64_t n_items;
    const int32_t *long_row;
    const int64_t *long_item0;
    int64_t n_long;
    double *item_partial;
    const double *r;     // the vector of this pass (m entries at least)
    double *out;         // sums + 2k
    const double *state; // [lz::DONE]: the run has stopped
};

__global__ __launch_bounds__(256) void k_sprhs_bt(LzBt b)
{
    if (b.state[lz::DONE] != 0.0) return;
    if ((int)blockIdx.x < b.nshort) {
        const int j = blockIdx.x * 256 + threadIdx.x;
        if (j >= b.p) return;
        const int64_t q0 = b.t_rowptr[j], q1 = b.t_rowptr[j + 1];
        if (q1 - q0 > RAILS_SPRHS_SHORT) return;
        double s = 0.0;
        for (int64_t q = q0; q < q1; ++q) s = __builtin_fma(b.t_val[q], b.r[b.t_col[q]], s);
        b.out[j] = s;
        return;
    }
    const int lane = threadIdx.x & 63;
    const int64_t item = ((int64_t)blockIdx.x - b.nshort) * 4 + (threadIdx.x >> 6);
    if (item >= b.n_items) return; // wave-uniform
    const int64_t beg = b.item_beg[item];
    const int n = b.item_len[item];
    double acc = 0.0;
    for (int e0 = 0; e0 < n; e0 += 64) {
        const bool on = e0 + lane < n;
        const int64_t q = on ? beg + e0 + lane : beg;
        const double v = b.t_val[q];
        const double x = b.r[b.t_col[q]];
        acc = on ? __builtin_fma(v, x, acc) : acc;
    }
    const double tot = wave_sum(acc);
    if (lane == 0) b.item_partial[item] = tot;
}

__global__ __launch_bounds__(256) void k_sprhs_bt_long(LzBt b)
{
    if (b.state[lz::DONE] != 0.0) return;
    const int lane = threadIdx.x & 63;
    const int64_t l = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (l >= b.n_long) return; // wave-uniform
    const int64_t i0 = b.long_item0[l], i1 = b.long_item0[l + 1];
    double acc = 0.0;
    for (int64_t i = i0 + lane; i < i1; i += 64) acc += b.item_partial[i];
    const double tot = wave_sum(acc);
    if (lane == 0) b.out[b.long_row[l]] = tot;
}

// One block.  sums = [c'_AV (k) | c'_MV (k) | c'_B (p) | rr] (already all-reduced).
// Writes the coefficients for the next pass, alpha/beta bookkeeping and the breakdown flag.
__global__ __launch_bounds__(1024) void k_lz_small(const double *__restrict__ sums, const double *__restrict__ T, int k, int p, int step,
                                                   double *__restrict__ coef, double *__restrict__ state, double *__restrict__ alphas,
                                                   double *__restrict__ betas)
{
    __shared__ double sh[1024];
    __shared__ double part1[4][256], part2[4][256];
    if (state[lz::DONE] != 0.0) return;
    const int tid = threadIdx.x;
    const int jr = tid & 255, q = tid >> 8; // output row within a group of 256, quarter of the inner index
    const double rr = sums[2 * k + p];
    const double beta = sqrt(rr);
    const bool init = step < 0;
    if (!init && beta < 1e-14) { // src/LyapunovSolver.hpp:419-426
        if (tid == 0) {
            betas[step] = beta;
            state[lz::DONE] = 1.0;
            state[lz::STEPS] = (double)(step + 1);
        }
        return;
    }
    const double inv = 1.0 / beta;
    // g_AV = T (c_MV * inv),  g_MV = T (c_AV * inv),  g_B = c_B * inv; the inner index is split over 4 strands that
    // are summed in a fixed order
    const int l0 = (int)(((int64_t)k * q) / 4), l1 = (int)(((int64_t)k * (q + 1)) / 4);
    for (int j0 = 0; j0 < k; j0 += 256) {
        const int j = j0 + jr;
        double s1 = 0.0, s2 = 0.0;
        if (j < k)
            for (int l = l0; l < l1; ++l) {
                const double t = T[j + (int64_t)l * k];
                s1 = __builtin_fma(t, sums[k + l] * inv, s1);
                s2 = __builtin_fma(t, sums[l] * inv, s2);
            }
        part1[q][jr] = s1;
        part2[q][jr] = s2;
        __syncthreads();
        if (q == 0 && j < k) {
            coef[j] = ((part1[0][jr] + part1[1][jr]) + part1[2][jr]) + part1[3][jr];
            coef[k + j] = ((part2[0][jr] + part2[1][jr]) + part2[2][jr]) + part2[3][jr];
        }
        __syncthreads();
    }
    for (int j = tid; j < p; j += 1024) coef[2 * k + j] = sums[2 * k + j] * inv;
    __threadfence_block();
    __syncthreads();
    // alpha_next = c_AV.g_AV + c_MV.g_MV + c_B.c_B
    double part = 0.0;
    for (int j = tid; j < k; j += 1024) {
        part = __builtin_fma(sums[j] * inv, coef[j], part);
        part = __builtin_fma(sums[k + j] * inv, coef[k + j], part);
    }
    for (int j = tid; j < p; j += 1024) {
        double cbv = sums[2 * k + j] * inv;
        part = __builtin_fma(cbv, cbv, part);
    }
    sh[tid] = part;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if (tid < s) sh[tid] += sh[tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        const double alpha_next = sh[0];
        state[lz::ALPHA] = alpha_next;
        state[lz::BETA_PREV] = init ? 0.0 : beta;
        state[lz::INV_BETA] = inv;
        alphas[step + 1] = alpha_next;
        if (!init) {
            betas[step] = beta;
            state[lz::STEPS] = (double)(step + 1);
        }
    }
}

// Out[row, oc0 + j] = sum_l Qc[l][row] * S[l + j*lds],  j < w (<= 16 per launch chunk)
__global__ __launch_bounds__(256) void k_lz_vectors(const double *__restrict__ Qc, int64_t mpad, int64_t m, int steps,
                                                    const double *__restrict__ S, int lds, int w, double *__restrict__ Out, int ldo)
{
    extern __shared__ double Ss[]; // steps x 16
    for (int idx = threadIdx.x; idx < steps * 16; idx += blockDim.x) {
        int l = idx / 16, j = idx % 16;
        Ss[idx] = (j < w) ? S[l + (int64_t)j * lds] : 0.0;
    }
    __syncthreads();
    int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= m) return;
    double acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.0;
    for (int l = 0; l < steps; ++l) {
        double q = Qc[(int64_t)l * mpad + row];
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = __builtin_fma(q, Ss[l * 16 + j], acc[j]);
    }
    double *o = Out + row * ldo;
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if (j < w) o[j] = acc[j];
}

__global__ void k_lz_random(double *__restrict__ q, int64_t m, int64_t mpad, uint64_t seed, uint64_t stream, int64_t row0);

__device__ __forceinline__ uint64_t sm64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__global__ void k_lz_random(double *__restrict__ q, int64_t m, int64_t mpad, uint64_t seed, uint64_t stream, int64_t row0)
{
    uint64_t hs = sm64(seed ^ sm64(stream * 0xD1342543DE82EF95ull + 0x632BE59BD9B4E019ull));
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < mpad; r += (int64_t)gridDim.x * blockDim.x) {
        double v = 0.0;
        if (r < m) {
            uint64_t h = sm64(hs ^ sm64((uint64_t)(row0 + r) * 0x9E3779B97F4A7C15ull + 1));
            double u = (double)(h >> 11) * (1.0 / 9007199254740992.0);
            v = 2.0 * u - 1.0;
        }
        q[r] = v;
    }
}

// ------------------------------------------------------------------------------------------------------------ the host side ---
// What a call decides without computing is lanczos_plan.h's.  Below: the stages of a run, in the order lz_stages takes them.

// the pass kernels: one row per row of lz::kPass, both forms of each.  The occupancy query and the launch both go through this table.
struct PassKernels {
    void (*sparse)(LzArgs, LzSparse);
    void (*dense)(LzArgs);
};
#define RAILS_LZ_PASS_KERNELS(N, U) {k_lanczos_pass_sparse<N, U>, k_lanczos_pass<N, U>},
const PassKernels kPassKernels[lz::kPassCount] = {RAILS_LZ_PASS_TABLE(RAILS_LZ_PASS_KERNELS)};
#undef RAILS_LZ_PASS_KERNELS

// one call of any of the three forms (what does not apply to a form is null or 0)
struct LzCall {
    lz::Form form;
    const rails_panel *AV;
    int avc0;
    const rails_panel *MV;
    int mvc0;
    int k;
    const double *T;
    int ldt;
    const rails_panel *B; // DenseB, StartOnly
    int bc0;
    int p;
    const rails_sprhs *SR; // SparseB
    int L;
    double *H;
    int ldh;
    int *steps_out;
    double *start_sums; // StartOnly
};

// ---- stage 1: the checks (lanczos_plan.h: lz::check).  Nothing is read through a pointer before the null check has seen it.
int lz_check(const rails_ctx *c, const LzCall &q)
{
    const bool sparse = q.form == lz::Form::SparseB;
    lz::Call s;
    s.form = q.form;
    s.have_inputs = c && q.AV && q.MV && (sparse ? q.SR != nullptr : q.B != nullptr);
    s.have_outputs = q.H && q.steps_out;
    s.have_T = q.T != nullptr;
    s.k = q.k, s.p = q.p, s.L = q.L, s.ldh = q.ldh, s.ldt = q.ldt;
    s.avc0 = q.avc0, s.mvc0 = q.mvc0, s.bc0 = q.bc0;
    if (s.have_inputs) {
        s.av_cap = q.AV->cap, s.mv_cap = q.MV->cap, s.b_cap = sparse ? 0 : q.B->cap;
        s.av_m = q.AV->m, s.mv_m = q.MV->m, s.b_m = sparse ? q.SR->m : q.B->m;
    }
    const lz::Verdict v = lz::check(s);
    RAILS_REQUIRE(v.ok, "%s", v.text);
    return RAILS_OK;
}

// ---- stage 2: the plan
int lz_unroll_setting() // RAILS_LZ_UNROLL, read once per process
{
    static const int u = lz::unroll_setting(getenv("RAILS_LZ_UNROLL"));
    return u;
}

// blocks of a pass kernel that fit a CU at once: a query, nothing is launched.  false: the query failed.
bool lz_occupancy(int pass, bool sparse, int *occ)
{
    *occ = 0;
    const void *kernel = sparse ? (const void *)kPassKernels[pass].sparse : (const void *)kPassKernels[pass].dense;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(occ, kernel, 256, 0) == hipSuccess;
}

int lz_plan(const rails_ctx *c, const LzCall &q, lz::Plan *pl)
{
    lz::plan_pass(*pl, q.k, lz_unroll_setting());
    RAILS_REQUIRE(pl->pass >= 0, "rails_resid_lanczos: no pass kernel <%d, %d>: not in the table of instantiations", pl->nch, pl->unroll);
    int occ = 0;
    const bool ok = lz_occupancy(pl->pass, q.form == lz::Form::SparseB, &occ);
    *pl = lz::plan(q.form, q.AV->m, q.k, q.p, q.L, c->num_cu, lz_unroll_setting(), ok, occ);
    return RAILS_OK;
}

// ---- stage 3: the buffers
// One of the state's two device buffers, made to hold `need` bytes by allocating `alloc` of them.  The stream is synchronised before the
// old buffer is freed.  A failed allocation leaves no buffer: pointer null, size 0.  (Neither buffer counts in n_dev_alloc.)
int lz_grow(rails_ctx *c, double **buf, size_t *bytes, size_t need, size_t alloc)
{
    if (need <= *bytes) return RAILS_OK;
    RAILS_HIP_CHECK(rails_stream_sync(c));
    double *old = *buf;
    *buf = nullptr;
    *bytes = 0;
    if (old) RAILS_HIP_CHECK(hipFree(old));
    const hipError_t e = hipMalloc((void **)buf, alloc);
    if (e != hipSuccess) {
        *buf = nullptr;
        rails_set_error("rails_resid_lanczos: hipMalloc(%zu) failed: %s", alloc, hipGetErrorString(e));
        return RAILS_ENOMEM;
    }
    *bytes = alloc;
    return RAILS_OK;
}

// the Lanczos vectors at their exact size, the small block at twice its need (L varies from trip to trip), the blocks' partial sums
int lz_reserve(rails_ctx *c, rails_lanczos_state &S, const lz::Plan &pl)
{
    S.steps = 0; // the vectors of the run before are given up, whatever happens below
    RAILS_TRY(lz_grow(c, &S.Qc, &S.qc_bytes, pl.vector_bytes, pl.vector_bytes));
    RAILS_TRY(lz_grow(c, &S.small, &S.small_bytes, pl.small.total * sizeof(double), 2 * pl.small.total * sizeof(double)));
    RAILS_TRY(rails_ws_reserve(c, pl.ws_bytes));
    S.m = pl.m;
    S.mpad = pl.mpad;
    S.L = pl.L;
    S.last_nch = pl.nch;
    S.last_unroll = pl.unroll;
    S.last_nblocks = pl.nblocks;
    return RAILS_OK;
}

// ---- stage 4: T and zeros into the small block, the raw q_0 into Lanczos vector 0
int lz_begin(rails_ctx *c, const rails_lanczos_state &S, const LzCall &q, const lz::Plan &pl)
{
    // rails_pinned_begin_write without rails_pinned_end_write: the upload out of the pinned buffer needs no event of its own, because
    // every path from here (lz_read_start, lz_read_H, an error return aside) synchronises the stream before the call returns
    RAILS_TRY(rails_pinned_begin_write(c, pl.pinned_bytes));
    if (pl.form != lz::Form::StartOnly && q.k) { // T -> device (contiguous k x k)
        for (int j = 0; j < q.k; ++j) memcpy(c->pinned + (size_t)j * q.k, q.T + (size_t)j * q.ldt, sizeof(double) * q.k);
        RAILS_HIP_CHECK(hipMemcpyAsync(S.small + pl.small.T, c->pinned, (size_t)q.k * q.k * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    RAILS_HIP_CHECK(hipMemsetAsync(S.small + pl.small.coef, 0, pl.small.cleared() * sizeof(double), c->stream));
    // start vector: Q.random() consumes one RNG stream (src/LyapunovSolver.hpp:374)
    const uint64_t stream = c->next_stream++;
    RAILS_LAUNCH(k_lz_random, dim3(pl.random_grid), dim3(256), 0, c->stream, S.Qc, pl.m, pl.mpad, c->seed, stream, c->row0);
    return RAILS_OK;
}

// ---- stage 5: the kernels' arguments, each struct filled here and nowhere else
LzArgs lz_args(const rails_ctx *c, const rails_lanczos_state &S, const LzCall &q, const lz::Plan &pl)
{
    const bool sparse = pl.form == lz::Form::SparseB;
    LzArgs a{};
    a.AV = q.AV->d + q.avc0;
    a.ldav = q.AV->ld;
    a.MV = q.MV->d + q.mvc0;
    a.ldmv = q.MV->ld;
    a.B = sparse ? nullptr : q.B->d + q.bc0;
    a.ldb = sparse ? 0 : q.B->ld;
    a.k = pl.k;
    a.p = sparse ? 0 : pl.p;
    a.av_room = q.AV->ld - q.avc0;
    a.mv_room = q.MV->ld - q.mvc0;
    a.b_room = sparse ? 0 : q.B->ld - q.bc0;
    a.m = pl.m;
    a.mpad = pl.mpad;
    a.Qc = S.Qc;
    a.step = -1;
    a.coef = S.small + pl.small.coef;
    a.state = S.small + pl.small.state;
    a.partial = c->ws;
    return a;
}

LzSparse lz_sparse(const rails_sprhs *SR, const double *gB)
{
    LzSparse sp{};
    sp.rowptr = SR->B->rowptr;
    sp.col = SR->B->col;
    sp.val = SR->B->val;
    sp.gB = gB;
    return sp;
}

LzBt lz_bt(const rails_sprhs *SR, const lz::BtGrids &g, double *out, const double *state)
{
    LzBt bt{};
    bt.t_rowptr = SR->Bt->rowptr;
    bt.t_col = SR->Bt->col;
    bt.t_val = SR->Bt->val;
    bt.p = SR->p;
    bt.nshort = g.nshort;
    bt.item_beg = SR->item_beg;
    bt.item_len = SR->item_len;
    bt.n_items = SR->n_items;
    bt.long_row = SR->long_row;
    bt.long_item0 = SR->long_item0;
    bt.n_long = SR->n_long;
    bt.item_partial = SR->item_partial;
    bt.r = nullptr; // per step: the vector the pass has just written
    bt.out = out;
    bt.state = state;
    return bt;
}

// ---- stage 6: the steps.  Per step: the pass, the reduction of its partials (sparse form: and c'_B = B'r from the vector the pass has
// just written, the raw q_0 at the start), the all-reduce, and -- but for the start-only form -- k_lz_small.
int lz_steps(rails_ctx *c, const rails_lanczos_state &S, const LzCall &q, const lz::Plan &pl)
{
    const bool sparse = pl.form == lz::Form::SparseB;
    const PassKernels &pass = kPassKernels[pl.pass];
    double *dT = S.small + pl.small.T, *dcoef = S.small + pl.small.coef, *dsums = S.small + pl.small.sums, *dstate = S.small + pl.small.state;
    LzArgs a = lz_args(c, S, q, pl);
    LzSparse sp{};
    LzBt bt{};
    lz::BtGrids g;
    if (sparse) {
        g = lz::bt_grids(pl.p, q.SR->n_items, q.SR->n_long);
        sp = lz_sparse(q.SR, dcoef + 2 * pl.k);
        bt = lz_bt(q.SR, g, dsums + 2 * pl.k, dstate);
    }
    for (int step = -1; step < pl.last_step; ++step) {
        a.step = step;
        if (sparse) {
            RAILS_LAUNCH(pass.sparse, dim3(pl.nblocks), dim3(256), 0, c->stream, a, sp);
            RAILS_LAUNCH(k_lz_reduce_last_at, dim3(pl.partial_grid), dim3(1024), 0, c->stream, c->ws, pl.nblocks, pl.npart, dsums, pl.ncoef - 1);
            bt.r = S.Qc + (size_t)(step + 1) * pl.mpad;
            if (g.bt > 0) RAILS_LAUNCH(k_sprhs_bt, dim3((unsigned)g.bt), dim3(256), 0, c->stream, bt);
            if (g.bt_long > 0) RAILS_LAUNCH(k_sprhs_bt_long, dim3((unsigned)g.bt_long), dim3(256), 0, c->stream, bt);
        } else {
            RAILS_LAUNCH(pass.dense, dim3(pl.nblocks), dim3(256), 0, c->stream, a);
            RAILS_LAUNCH(k_lz_reduce, dim3(pl.partial_grid), dim3(1024), 0, c->stream, c->ws, pl.nblocks, pl.npart, dsums);
        }
        RAILS_TRY(rails_allreduce_dev(c, dsums, (size_t)pl.ncoef));
        if (pl.form == lz::Form::StartOnly) break;
        RAILS_LAUNCH(k_lz_small, dim3(1), dim3(1024), 0, c->stream, dsums, dT, pl.k, pl.p, step, dcoef, dstate, S.small + pl.small.alphas,
                     S.small + pl.small.betas);
    }
    RAILS_HIP_CHECK(hipGetLastError());
    return RAILS_OK;
}

// ---- stage 7, start-only form: [AV^T q0 | MV^T q0 | B^T q0 | q0^T q0], q0 kept (raw) as Lanczos vector 0
int lz_read_start(rails_ctx *c, rails_lanczos_state &S, const lz::Plan &pl, double *sums_host)
{
    RAILS_TRY(rails_pinned_reserve(c, pl.start_pinned_bytes));
    RAILS_HIP_CHECK(hipMemcpyAsync(c->pinned, S.small + pl.small.sums, (size_t)pl.ncoef * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    RAILS_HIP_CHECK(rails_stream_sync(c));
    memcpy(sums_host, c->pinned, (size_t)pl.ncoef * sizeof(double));
    S.steps = 1;
    c->n_lanczos_start++;
    return RAILS_OK;
}

// ---- stage 7, the other forms: state, alphas and betas in one copy (lz::SmallBlock keeps them together), H from them
int lz_read_H(rails_ctx *c, rails_lanczos_state &S, const lz::Plan &pl, double *H_host, int ldh, int *steps_out)
{
    const lz::SmallBlock &b = pl.small;
    RAILS_HIP_CHECK(hipMemcpyAsync(c->pinned, S.small + b.state, b.read_back() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    RAILS_HIP_CHECK(rails_stream_sync(c));
    const int steps = lz::assemble_H(H_host, ldh, pl.L, c->pinned, c->pinned + (b.alphas - b.state), c->pinned + (b.betas - b.state));
    S.steps = steps;
    c->n_lanczos++;
    *steps_out = steps;
    return RAILS_OK;
}

int lz_stages(rails_ctx *c, const LzCall &q)
{
    RAILS_TRY(lz_check(c, q));
    lz::Plan pl;
    RAILS_TRY(lz_plan(c, q, &pl));
    rails_lanczos_state &S = lz_state(c);
    RAILS_TRY(lz_reserve(c, S, pl));
    RAILS_TRY(lz_begin(c, S, q, pl));
    RAILS_TRY(lz_steps(c, S, q, pl));
    if (pl.form == lz::Form::StartOnly) return lz_read_start(c, S, pl, q.start_sums);
    return lz_read_H(c, S, pl, q.H, q.ldh, q.steps_out);
}

} // namespace

extern "C" int rails_resid_lanczos(rails_ctx *c, const rails_panel *AV, int avc0, const rails_panel *MV, int mvc0, int k,
                                   const double *T_host, int ldt, const rails_panel *B, int bc0, int p, int L, double *H_host,
                                   int ldh, int *steps_out)
{
    if (c) hipSetDevice(c->device); // allocations and launches go to the context's device whatever the caller's current device is
    return lz_stages(c, LzCall{lz::Form::DenseB, AV, avc0, MV, mvc0, k, T_host, ldt, B, bc0, p, nullptr, L, H_host, ldh, steps_out, nullptr});
}

extern "C" int rails_resid_lanczos_sparse(rails_ctx *c, const rails_panel *AV, int avc0, const rails_panel *MV, int mvc0, int k,
                                          const double *T_host, int ldt, const rails_sprhs *SR, int L, double *H_host, int ldh, int *steps_out)
{
    if (c) hipSetDevice(c->device); // allocations and launches go to the context's device whatever the caller's current device is
    RAILS_REQUIRE(c && SR, "rails_resid_lanczos_sparse: null argument");
    RAILS_REQUIRE(c == SR->ctx && c->nranks == 1 && !c->rccl, "rails_resid_lanczos_sparse: single GPU only, on the context the right-hand side was made on");
    return lz_stages(c, LzCall{lz::Form::SparseB, AV, avc0, MV, mvc0, k, T_host, ldt, nullptr, 0, SR->p, SR, L, H_host, ldh, steps_out, nullptr});
}

extern "C" int rails_lanczos_start(rails_ctx *c, const rails_panel *AV, int avc0, const rails_panel *MV, int mvc0, int k,
                                   const rails_panel *B, int bc0, int p, double *sums_host)
{
    if (c) hipSetDevice(c->device); // allocations and launches go to the context's device whatever the caller's current device is
    RAILS_REQUIRE(sums_host, "rails_lanczos_start: null output");
    return lz_stages(c, LzCall{lz::Form::StartOnly, AV, avc0, MV, mvc0, k, nullptr, 0, B, bc0, p, nullptr, 1, nullptr, 0, nullptr, sums_host});
}

extern "C" int rails_lanczos_vectors(rails_ctx *c, const double *S_host, int lds, int w, rails_panel *Out, int oc0)
{
    if (c) hipSetDevice(c->device); // allocations and launches go to the context's device whatever the caller's current device is
    RAILS_REQUIRE(c && Out, "rails_lanczos_vectors: null argument");
    rails_lanczos_state &S = lz_state(c);
    RAILS_REQUIRE(S.Qc && S.steps > 0, "rails_lanczos_vectors: no Lanczos run to take vectors from");
    RAILS_REQUIRE(w >= 0 && oc0 >= 0 && oc0 + w <= Out->cap, "rails_lanczos_vectors: columns [%d,%d) outside capacity %d", oc0, oc0 + w,
                  Out->cap);
    RAILS_REQUIRE(Out->m == S.m, "rails_lanczos_vectors: row mismatch %lld vs %lld", (long long)Out->m, (long long)S.m);
    RAILS_REQUIRE(w == 0 || (S_host && lds >= S.steps), "rails_lanczos_vectors: bad coefficient matrix");
    if (w == 0 || S.m == 0) return RAILS_OK;
    const int steps = S.steps;
    const lz::VectorsPlan v = lz::vectors_plan(S.m, steps, w);
    RAILS_TRY(rails_small_reserve(c, v.s_bytes));
    // rails_pinned_begin_write without rails_pinned_end_write: the stream is synchronised below, before this function returns, so the
    // upload out of the pinned buffer needs no event of its own
    RAILS_TRY(rails_pinned_begin_write(c, v.s_bytes));
    for (int j = 0; j < w; ++j) memcpy(c->pinned + (size_t)j * steps, S_host + (size_t)j * lds, sizeof(double) * steps);
    RAILS_HIP_CHECK(hipMemcpyAsync(c->small, c->pinned, v.s_bytes, hipMemcpyHostToDevice, c->stream));
    for (int ch = 0; ch < v.nchunks; ++ch) {
        const int j0 = v.first(ch);
        RAILS_LAUNCH(k_lz_vectors, dim3(v.grid), dim3(256), lz::vectors_lds_bytes(steps), c->stream, S.Qc, S.mpad, S.m, steps,
                     c->small + (size_t)j0 * steps, steps, v.width(ch), Out->d + oc0 + j0, Out->ld);
    }
    RAILS_HIP_CHECK(hipGetLastError());
    RAILS_HIP_CHECK(rails_stream_sync(c));
    return RAILS_OK;
}

extern "C" int rails_lanczos_last_launch(rails_ctx *c, int *nch, int *unroll, int *nblocks)
{
    RAILS_REQUIRE(c && nch && unroll && nblocks, "rails_lanczos_last_launch: null argument");
    const rails_lanczos_state &S = lz_state(c);
    RAILS_REQUIRE(S.last_nblocks > 0, "rails_lanczos_last_launch: no Lanczos run on this context");
    *nch = S.last_nch;
    *unroll = S.last_unroll;
    *nblocks = S.last_nblocks;
    return RAILS_OK;
}

extern "C" int rails_lanczos_release(rails_ctx *c)
{
    if (!c || !c->lz) return RAILS_OK;
    rails_lanczos_state *S = static_cast<rails_lanczos_state *>(c->lz);
    rails_stream_sync(c);
    if (S->Qc) hipFree(S->Qc);
    if (S->small) hipFree(S->small);
    delete S;
    c->lz = nullptr;
    return RAILS_OK;
}
