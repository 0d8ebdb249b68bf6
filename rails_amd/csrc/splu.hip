// splu.hip -- A^-1 X (or A^-T X) from the factors of a host sparse LU, Pr A Pc = L U (scipy's SuperLU), as a library object: the
// A^-1 r products of RAILS' inverse and extended Krylov projections (matlab/RAILSsolver.m:7-24,288-314,520-530) and the operator
// Sinv of a Schur complement (matlab/RAILSschur.m:60-64), x -> (A^-1 E x)[rows] with E putting x on `rows` and zeros elsewhere.
//
// A solve is two level-scheduled triangular sweeps over a workspace panel of n rows that the object owns:
//   forward   A^-1: L z = Pr E x;  A^-T: U' z = Pc' E x   -- the right-hand side is gathered from X inside this sweep (in_map)
//   backward  A^-1: U y = z;       A^-T: L' y = z        -- and the result is scattered to Y inside this one (out_pos)
// so there are no separate permutation passes.  Levels of a triangle (rows whose dependencies are all in earlier levels) are sorted
// on the host at creation; a row is gathered by a group of RAILS_LU_LANES lanes.  Levels of more than RAILS_LU_NARROW rows get a
// launch of their own, a group per row and column.
// Runs of consecutive narrower levels -- most levels of a banded or 2D factor -- are split over COLUMNS: workgroup g owns column
// g of the panel and walks every level of the run for it, with a barrier between levels.  A solve of nc columns so occupies nc CUs,
// and no workgroup ever waits on another one's data.  Every entry of the result is computed by the same sequence of operations in
// either kind of launch, so column j of a wide solve is bitwise the one-column solve of column j.  Memory-bound gathers: no
// matrix cores.  (The older sptrsv.hip walks narrow runs with one workgroup for all columns; it stays as it is for the Schur
// operator's A11 solve.)
#include "rails_internal.h"

#include <algorithm>
#include <vector>

namespace {

constexpr int RAILS_LU_NARROW = 1024; // widest level a column-split run takes (rows)
constexpr int RAILS_LU_LANES = 16;    // lanes that share one row: a factor row of a 2D problem holds tens of entries, gathered at once

struct LuTri {
    int64_t n = 0, nnz = 0;
    int unit = 0;
    int64_t *rowptr = nullptr; // device CSR without the diagonal
    int32_t *col = nullptr;
    double *val = nullptr;
    double *diag = nullptr; // diagonal entry per row (null for a unit triangle)
    int32_t *order = nullptr;
    int64_t *level_ptr_dev = nullptr;
    std::vector<int64_t> level_ptr;
    // launch plan: {first level, last level + 1, threads per workgroup (0: a wide level of its own)}
    struct Seg {
        int l0, l1, threads;
    };
    std::vector<Seg> segs;
};

} // namespace

struct rails_lu {
    rails_ctx *ctx = nullptr;
    int64_t n = 0, m_sub = 0;
    LuTri tri[4];                 // 0 L, 1 U (A^-1);  2 U' (lower), 3 L' (upper) (A^-T)
    int32_t *in_map[2] = {};      // [trans]: forward row j takes X row in_map[j] (-1: zero)
    int32_t *out_pos[2] = {};     // [trans]: backward row j goes to Y row out_pos[j] (-1: nowhere)
    double *work = nullptr;       // n x work_ld
    int work_ld = 0;
    long last_launches = 0;
};

namespace {

// one row of a triangle for one column, by a group of RAILS_LU_LANES lanes: lane j gathers entries j, j + LANES, ... of the row, the
// partial sums meet in a fixed butterfly, lane 0 finishes the row.  Both kernels call this with whole groups, so every entry of the
// result is computed by the same operations in the same order whichever kernel and width (bitwise column independence).
template <bool FIRST, bool LAST>
__device__ __forceinline__ void lu_row(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, const double *__restrict__ val,
                                       const double *__restrict__ diag, const int32_t *__restrict__ in_map, const int32_t *__restrict__ out_pos,
                                       int32_t row, int c, int lane, const double *__restrict__ X, int ldx, double *W, int ldw, double *__restrict__ Y, int ldy)
{
    double part = 0.0;
    for (int64_t q = rowptr[row] + lane; q < rowptr[row + 1]; q += RAILS_LU_LANES) part = fma(val[q], W[(int64_t)col[q] * ldw + c], part);
    for (int off = RAILS_LU_LANES / 2; off > 0; off /= 2) part += __shfl_xor(part, off, RAILS_LU_LANES);
    if (lane != 0) return;
    double acc;
    if (FIRST) {
        const int32_t src = in_map[row];
        acc = src >= 0 ? X[(int64_t)src * ldx + c] : 0.0;
    } else
        acc = W[(int64_t)row * ldw + c];
    acc -= part;
    if (diag) acc = acc / diag[row];
    W[(int64_t)row * ldw + c] = acc;
    if (LAST) {
        const int32_t dst = out_pos[row];
        if (dst >= 0) Y[(int64_t)dst * ldy + c] = acc;
    }
}

// one level, a group of lanes per (row, column)
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(256) void k_lu_level(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, const double *__restrict__ val,
                                                  const double *__restrict__ diag, const int32_t *__restrict__ order, int64_t r0, int64_t r1,
                                                  const int32_t *__restrict__ in_map, const int32_t *__restrict__ out_pos, const double *__restrict__ X,
                                                  int ldx, double *W, int ldw, double *__restrict__ Y, int ldy, int nc)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t g = t / RAILS_LU_LANES;
    const int64_t r = r0 + g / nc;
    if (r >= r1) return; // whole groups leave together
    lu_row<FIRST, LAST>(rowptr, col, val, diag, in_map, out_pos, order[r], (int)(g % nc), (int)(t % RAILS_LU_LANES), X, ldx, W, ldw, Y, ldy);
}

// levels l0 .. l1 - 1 for column blockIdx.x.  What a level writes the next one reads in the same workgroup: all its waves run on one CU
// and share its L1, and the barrier (a workgroup-scope release and acquire) orders the loads after the stores of the level before.
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(1024) void k_lu_run(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, const double *__restrict__ val,
                                                 const double *__restrict__ diag, const int32_t *__restrict__ order, const int64_t *__restrict__ level_ptr,
                                                 int l0, int l1, const int32_t *__restrict__ in_map, const int32_t *__restrict__ out_pos,
                                                 const double *__restrict__ X, int ldx, double *W, int ldw, double *__restrict__ Y, int ldy)
{
    const int c = blockIdx.x;
    const int lane = threadIdx.x % RAILS_LU_LANES, groups = blockDim.x / RAILS_LU_LANES;
    for (int l = l0; l < l1; ++l) {
        const int64_t r0 = level_ptr[l], r1 = level_ptr[l + 1];
        for (int64_t r = r0 + threadIdx.x / RAILS_LU_LANES; r < r1; r += groups)
            lu_row<FIRST, LAST>(rowptr, col, val, diag, in_map, out_pos, order[r], c, lane, X, ldx, W, ldw, Y, ldy);
        __syncthreads();
    }
}

// level analysis of a triangle given in host CSR without its diagonal (dval: the diagonal, null for a unit triangle), upload
int tri_create(rails_ctx *c, LuTri &T, int64_t n, bool lower, const std::vector<int64_t> &rp, const std::vector<int32_t> &ci,
               const std::vector<double> &va, const std::vector<double> *dval)
{
    std::vector<int32_t> level(n, 0);
    int32_t nlev = 0;
    for (int64_t s = 0; s < n; ++s) {
        const int64_t i = lower ? s : n - 1 - s;
        int32_t lv = 0;
        for (int64_t q = rp[i]; q < rp[i + 1]; ++q) lv = std::max(lv, level[ci[q]] + 1);
        level[i] = lv;
        nlev = std::max(nlev, lv + 1);
    }
    T.n = n;
    T.nnz = rp[n];
    T.unit = dval ? 0 : 1;
    T.level_ptr.assign((size_t)nlev + 1, 0);
    for (int64_t i = 0; i < n; ++i) T.level_ptr[level[i] + 1]++;
    for (int32_t l = 0; l < nlev; ++l) T.level_ptr[l + 1] += T.level_ptr[l];
    std::vector<int32_t> order(n);
    {
        std::vector<int64_t> fill(T.level_ptr.begin(), T.level_ptr.end() - 1);
        for (int64_t i = 0; i < n; ++i) order[fill[level[i]]++] = (int32_t)i;
    }
    for (int l = 0; l < nlev;) {
        const int64_t w = T.level_ptr[l + 1] - T.level_ptr[l];
        if (w > RAILS_LU_NARROW) {
            T.segs.push_back({l, l + 1, 0});
            ++l;
            continue;
        }
        int l1 = l;
        int64_t widest = 0;
        while (l1 < nlev && T.level_ptr[l1 + 1] - T.level_ptr[l1] <= RAILS_LU_NARROW) {
            widest = std::max(widest, T.level_ptr[l1 + 1] - T.level_ptr[l1]);
            ++l1;
        }
        T.segs.push_back({l, l1, (int)std::min<int64_t>(1024, (widest * RAILS_LU_LANES + 63) / 64 * 64)});
        l = l1;
    }
    auto up = [&](void **dst, const void *src, size_t bytes) -> int {
        *dst = nullptr;
        if (bytes == 0) return RAILS_OK;
        RAILS_HIP_CHECK(hipMalloc(dst, bytes));
        RAILS_HIP_CHECK(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
        return RAILS_OK;
    };
    RAILS_TRY(up((void **)&T.rowptr, rp.data(), (size_t)(n + 1) * sizeof(int64_t)));
    RAILS_TRY(up((void **)&T.col, ci.data(), ci.size() * sizeof(int32_t)));
    RAILS_TRY(up((void **)&T.val, va.data(), va.size() * sizeof(double)));
    if (dval) RAILS_TRY(up((void **)&T.diag, dval->data(), (size_t)n * sizeof(double)));
    RAILS_TRY(up((void **)&T.order, order.data(), (size_t)n * sizeof(int32_t)));
    RAILS_TRY(up((void **)&T.level_ptr_dev, T.level_ptr.data(), T.level_ptr.size() * sizeof(int64_t)));
    return RAILS_OK;
}

void tri_free(LuTri &T)
{
    hipFree(T.rowptr);
    hipFree(T.col);
    hipFree(T.val);
    hipFree(T.diag);
    hipFree(T.order);
    hipFree(T.level_ptr_dev);
}

// host CSR of a triangle without its diagonal (kept apart in *diag when diag != null; a unit triangle's stored diagonal must be 1)
int split_tri(const char *name, int64_t n, const int64_t *rowptr, const int32_t *col, const double *val, bool lower, bool unit, std::vector<int64_t> &rp,
              std::vector<int32_t> &ci, std::vector<double> &va, std::vector<double> *diag)
{
    RAILS_REQUIRE(rowptr && rowptr[0] == 0 && rowptr[n] >= 0 && (rowptr[n] == 0 || (col && val)), "rails_lu_create: bad arrays of %s", name);
    rp.assign((size_t)n + 1, 0);
    if (diag) diag->assign((size_t)n, 0.0);
    for (int64_t i = 0; i < n; ++i) {
        RAILS_REQUIRE(rowptr[i + 1] >= rowptr[i], "rails_lu_create: row pointers of %s decrease at row %lld", name, (long long)i);
        for (int64_t q = rowptr[i]; q < rowptr[i + 1]; ++q) {
            const int32_t j = col[q];
            RAILS_REQUIRE(j >= 0 && j < n && (lower ? j <= i : j >= i), "rails_lu_create: entry (%lld, %d) of %s is outside its triangle", (long long)i, j, name);
            if (j == i) {
                if (unit)
                    RAILS_REQUIRE(val[q] == 1.0, "rails_lu_create: %s has unit diagonal but stores %g in row %lld", name, val[q], (long long)i);
                else
                    (*diag)[i] += val[q];
                continue;
            }
            ci.push_back(j);
            va.push_back(val[q]);
        }
        rp[i + 1] = (int64_t)ci.size();
        if (diag) RAILS_REQUIRE((*diag)[i] != 0.0, "rails_lu_create: zero on the diagonal of %s in row %lld", name, (long long)i);
    }
    return RAILS_OK;
}

void transpose_csr(int64_t n, const std::vector<int64_t> &rp, const std::vector<int32_t> &ci, const std::vector<double> &va, std::vector<int64_t> &tp,
                   std::vector<int32_t> &tc, std::vector<double> &tv)
{
    tp.assign((size_t)n + 1, 0);
    for (int32_t j : ci) tp[j + 1]++;
    for (int64_t i = 0; i < n; ++i) tp[i + 1] += tp[i];
    tc.resize(ci.size());
    tv.resize(va.size());
    std::vector<int64_t> fill(tp.begin(), tp.end() - 1);
    for (int64_t i = 0; i < n; ++i)
        for (int64_t q = rp[i]; q < rp[i + 1]; ++q) {
            const int64_t d = fill[ci[q]]++;
            tc[d] = (int32_t)i;
            tv[d] = va[q];
        }
}

// a solve is a first sweep (gathers from X) and a last one (scatters to Y): the only two forms of the kernels that are built
int sweep(rails_ctx *c, rails_lu *lu, const LuTri &T, bool first, const int32_t *in_map, const int32_t *out_pos, const double *X, int ldx, double *Y, int ldy,
          int nc)
{
    double *W = lu->work;
    const int ldw = lu->work_ld;
    for (const LuTri::Seg &s : T.segs) {
#define RAILS_LU_LAUNCH(F, L)                                                                                                                    \
    do {                                                                                                                                         \
        if (s.threads == 0) {                                                                                                                    \
            const int64_t work = (T.level_ptr[s.l0 + 1] - T.level_ptr[s.l0]) * nc * RAILS_LU_LANES;                                              \
            RAILS_LAUNCH((k_lu_level<F, L>), dim3((unsigned)((work + 255) / 256)), dim3(256), 0, c->stream, T.rowptr, T.col, T.val, T.diag,     \
                         T.order, T.level_ptr[s.l0], T.level_ptr[s.l0 + 1], in_map, out_pos, X, ldx, W, ldw, Y, ldy, nc);                       \
        } else                                                                                                                                   \
            RAILS_LAUNCH((k_lu_run<F, L>), dim3((unsigned)nc), dim3(s.threads), 0, c->stream, T.rowptr, T.col, T.val, T.diag, T.order,          \
                         T.level_ptr_dev, s.l0, s.l1, in_map, out_pos, X, ldx, W, ldw, Y, ldy);                                                 \
    } while (0)
        if (first)
            RAILS_LU_LAUNCH(true, false);
        else
            RAILS_LU_LAUNCH(false, true);
#undef RAILS_LU_LAUNCH
        lu->last_launches++;
    }
    return RAILS_OK;
}

} // namespace

extern "C" void rails_lu_destroy(rails_lu *lu)
{
    if (!lu) return;
    if (lu->ctx) {
        hipSetDevice(lu->ctx->device);
        hipStreamSynchronize(lu->ctx->stream);
    }
    for (LuTri &T : lu->tri) tri_free(T);
    for (int t = 0; t < 2; ++t) {
        hipFree(lu->in_map[t]);
        hipFree(lu->out_pos[t]);
    }
    hipFree(lu->work);
    delete lu;
}

extern "C" int rails_lu_create(rails_ctx *c, int64_t n, const int64_t *L_rowptr, const int32_t *L_col, const double *L_val, const int64_t *U_rowptr,
                               const int32_t *U_col, const double *U_val, const int32_t *perm_r, const int32_t *perm_c, const int32_t *rows, int64_t m_sub,
                               rails_lu **out)
{
    if (c) hipSetDevice(c->device);
    RAILS_REQUIRE(c && out && perm_r && perm_c && n >= 1 && n < ((int64_t)1 << 31), "rails_lu_create: bad argument");
    RAILS_REQUIRE(c->nranks == 1 && !c->rccl, "rails_lu_create: single GPU only (the context has a partition or a communicator)");
    if (!rows) m_sub = n;
    RAILS_REQUIRE(m_sub >= 1 && m_sub <= n, "rails_lu_create: %lld rows of a system of order %lld", (long long)m_sub, (long long)n);
    // permutations and the restriction
    std::vector<int32_t> iperm_r(n, -1), iperm_c(n, -1), sub(n, -1);
    for (int64_t i = 0; i < n; ++i) {
        RAILS_REQUIRE(perm_r[i] >= 0 && perm_r[i] < n && iperm_r[perm_r[i]] < 0, "rails_lu_create: perm_r is not a permutation");
        RAILS_REQUIRE(perm_c[i] >= 0 && perm_c[i] < n && iperm_c[perm_c[i]] < 0, "rails_lu_create: perm_c is not a permutation");
        iperm_r[perm_r[i]] = (int32_t)i;
        iperm_c[perm_c[i]] = (int32_t)i;
    }
    for (int64_t k = 0; k < m_sub; ++k) {
        const int32_t i = rows ? rows[k] : (int32_t)k;
        RAILS_REQUIRE(i >= 0 && i < n && sub[i] < 0, "rails_lu_create: rows[%lld] = %d is out of range or repeated", (long long)k, i);
        sub[i] = (int32_t)k;
    }
    // A^-1: L z = Pr b, (Pr b)[perm_r[i]] = b[i];  x[i] = y[perm_c[i]].   A^-T: U' z = Pc' b, (Pc' b)[perm_c[i]] = b[i];  x[i] = y[perm_r[i]]
    std::vector<int32_t> in_map[2] = {std::vector<int32_t>(n), std::vector<int32_t>(n)}, out_pos[2] = {std::vector<int32_t>(n, -1), std::vector<int32_t>(n, -1)};
    for (int64_t j = 0; j < n; ++j) {
        in_map[0][j] = sub[iperm_r[j]];
        in_map[1][j] = sub[iperm_c[j]];
    }
    for (int64_t i = 0; i < n; ++i)
        if (sub[i] >= 0) {
            out_pos[0][perm_c[i]] = sub[i];
            out_pos[1][perm_r[i]] = sub[i];
        }
    std::vector<int64_t> lp, up, ltp, utp;
    std::vector<int32_t> lc, uc, ltc, utc;
    std::vector<double> lv, uv, ltv, utv, ud;
    RAILS_TRY(split_tri("L", n, L_rowptr, L_col, L_val, true, true, lp, lc, lv, nullptr));
    RAILS_TRY(split_tri("U", n, U_rowptr, U_col, U_val, false, false, up, uc, uv, &ud));
    transpose_csr(n, lp, lc, lv, ltp, ltc, ltv);
    transpose_csr(n, up, uc, uv, utp, utc, utv);
    rails_lu *lu = new rails_lu;
    lu->ctx = c;
    lu->n = n;
    lu->m_sub = m_sub;
    int rc = tri_create(c, lu->tri[0], n, true, lp, lc, lv, nullptr);
    if (rc == RAILS_OK) rc = tri_create(c, lu->tri[1], n, false, up, uc, uv, &ud);
    if (rc == RAILS_OK) rc = tri_create(c, lu->tri[2], n, true, utp, utc, utv, &ud);
    if (rc == RAILS_OK) rc = tri_create(c, lu->tri[3], n, false, ltp, ltc, ltv, nullptr);
    for (int t = 0; t < 2 && rc == RAILS_OK; ++t) {
        for (int32_t **dst : {&lu->in_map[t], &lu->out_pos[t]}) {
            const std::vector<int32_t> &src = dst == &lu->in_map[t] ? in_map[t] : out_pos[t];
            if (hipMalloc((void **)dst, (size_t)n * sizeof(int32_t)) != hipSuccess || hipMemcpy(*dst, src.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) {
                rails_set_error("rails_lu_create: device allocation or upload failed");
                rc = RAILS_EHIP;
                break;
            }
        }
    }
    if (rc != RAILS_OK) {
        rails_lu_destroy(lu);
        return rc;
    }
    *out = lu;
    return RAILS_OK;
}

extern "C" int rails_lu_solve(rails_ctx *c, rails_lu *lu, int trans, const rails_panel *X, int xc0, int nc, rails_panel *Y, int yc0)
{
    if (c) hipSetDevice(c->device);
    rails_slow_guard slow__(c, "rails_lu_solve", nc, lu ? lu->n : 0);
    RAILS_REQUIRE(c && lu && X && Y, "rails_lu_solve: null argument");
    RAILS_REQUIRE(c == lu->ctx, "rails_lu_solve: the object belongs to another context");
    RAILS_REQUIRE(X->m == lu->m_sub && Y->m == lu->m_sub, "rails_lu_solve: the operator has %lld rows, X %lld, Y %lld", (long long)lu->m_sub, (long long)X->m,
                  (long long)Y->m);
    RAILS_REQUIRE(xc0 >= 0 && nc >= 0 && xc0 + nc <= X->cap && yc0 >= 0 && yc0 + nc <= Y->cap, "rails_lu_solve: column windows outside the panels");
    if (X->d == Y->d) RAILS_REQUIRE(xc0 + nc <= yc0 || yc0 + nc <= xc0, "rails_lu_solve: X and Y windows alias");
    lu->last_launches = 0;
    if (nc == 0) return RAILS_OK;
    if (nc > lu->work_ld) { // the workspace grows to the widest solve asked for and stays
        const int ld = rails_pad_ld(nc);
        RAILS_HIP_CHECK(hipStreamSynchronize(c->stream));
        if (lu->work) RAILS_HIP_CHECK(hipFree(lu->work));
        lu->work = nullptr;
        lu->work_ld = 0;
        RAILS_HIP_CHECK(hipMalloc((void **)&lu->work, (size_t)lu->n * ld * sizeof(double)));
        lu->work_ld = ld;
        c->n_dev_alloc++;
    }
    const int t = trans ? 1 : 0;
    const LuTri &first = lu->tri[trans ? 2 : 0], &second = lu->tri[trans ? 3 : 1];
    const double *Xp = X->d + xc0;
    double *Yp = Y->d + yc0;
    RAILS_TRY(sweep(c, lu, first, true, lu->in_map[t], lu->out_pos[t], Xp, X->ld, Yp, Y->ld, nc));
    RAILS_TRY(sweep(c, lu, second, false, lu->in_map[t], lu->out_pos[t], Xp, X->ld, Yp, Y->ld, nc));
    RAILS_HIP_CHECK(hipGetLastError());
    return RAILS_OK;
}

// info[0..3] levels of L, U, U', L'; [4] nnz of L below its diagonal, [5] nnz of U (diagonal included); [6] launches of the last solve;
// [7] n, [8] rows of the restriction, [9] workspace columns.  Returns the number of entries written (at most cap).
extern "C" int rails_lu_stats(const rails_lu *lu, int64_t *info, int cap)
{
    RAILS_REQUIRE(lu && info && cap >= 0, "rails_lu_stats: bad argument");
    const int64_t v[10] = {(int64_t)lu->tri[0].level_ptr.size() - 1, (int64_t)lu->tri[1].level_ptr.size() - 1, (int64_t)lu->tri[2].level_ptr.size() - 1,
                           (int64_t)lu->tri[3].level_ptr.size() - 1, lu->tri[0].nnz, lu->tri[1].nnz + lu->n, lu->last_launches, lu->n, lu->m_sub,
                           lu->work_ld};
    const int k = std::min(cap, 10);
    for (int i = 0; i < k; ++i) info[i] = v[i];
    return k;
}

extern "C" int rails_csr_create_lu(rails_ctx *c, rails_lu *lu, rails_csr **out)
{
    RAILS_REQUIRE(c && lu && out, "rails_csr_create_lu: null argument");
    RAILS_REQUIRE(c == lu->ctx, "rails_csr_create_lu: the object belongs to another context");
    RAILS_REQUIRE(c->nranks == 1 && !c->rccl, "rails_csr_create_lu: single GPU only (the context has a partition or a communicator)");
    rails_csr *A = new rails_csr();
    A->ctx = c;
    A->m = lu->m_sub;
    A->ncols_ext = lu->m_sub;
    A->kind = rails_csr::LU;
    A->delegate = lu;
    A->last_kernel = "lu";
    *out = A;
    return RAILS_OK;
}
