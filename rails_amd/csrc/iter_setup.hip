// iter_setup.hip -- the iterative A^-1 operator (itsolve.hip has the map of its files): the object's lifetime (rails_iter_create, on a
// context that reduces a collective call; rails_iter_destroy), its settings (rails_iter_set), the facts the preconditioner rule decides on
// (rails_iter_facts for iter_precond.h), the work panels and the columns' scalars, the statistics, and the operator handle whose products
// are the solves.  Nothing in here launches a kernel.
#include "iter_object.h"

#include <algorithm>
#include <cmath>

#include "cheb_coef.h"
#include "iter_agree.h"

namespace {

void release_work(rails_iter *it)
{
    for (rails_panel *&p : it->w) {
        rails_panel_destroy(p);
        p = nullptr;
    }
    it->work_cols = 0;
}

} // namespace

bool rails_iter_host_csr(const rails_csr *A, int64_t m)
{
    return A->kind == rails_csr::STORED && (int64_t)A->h_rowptr.size() == m + 1 && (int64_t)A->h_val.size() == A->h_rowptr[m] && A->h_col.size() == A->h_val.size();
}

rails_precond_facts rails_iter_facts(const rails_iter *it)
{
    const rails_csr *A = it->A;
    rails_precond_facts f;
    f.cg = it->method == RAILS_ITER_CG;
    switch (A->kind) {
    case rails_csr::BSR: f.op = RAILS_PC_OP_BSR; break;
    case rails_csr::CALLBACK: f.op = RAILS_PC_OP_CALLBACK; break;
    case rails_csr::LU: f.op = RAILS_PC_OP_LU; break;
    case rails_csr::ITER: f.op = RAILS_PC_OP_ITER; break;
    default: f.op = RAILS_PC_OP_STORED; break; // (a sparse right-hand side never becomes an object: rails_iter_create)
    }
    f.host_csr = rails_iter_host_csr(A, it->m);
    int64_t mb = 0;
    const int64_t *browptr = nullptr;
    const int32_t *bcol = nullptr;
    const double *bval = nullptr;
    if (A->kind != rails_csr::BSR || !rails_bsr_host_arrays(A, &f.host_b, &mb, &browptr, &bcol, &bval)) f.host_b = 0;
    f.reduces = it->reduces;
    f.exchanges = A->n_ghost > 0 || A->n_send > 0;
    f.m = it->m;
    f.diag = it->dinv != nullptr;
    f.blocks_b = it->bj_dev ? it->bj_b : 0;
    f.defsign = it->defsign < 0.0 ? -1 : 1;
    f.jacobi = it->jacobi != 0;
    f.poly_degree = it->poly_degree;
    f.amg = it->amg != 0;
    f.block_amg = it->block_amg != 0;
    f.block_jacobi = it->block_jacobi != 0;
    return f;
}

int rails_iter_grant(const rails_iter *it, int request, int v, const char *who)
{
    char err[256];
    if (rails_precond_grant(rails_iter_facts(it), request, v, who, err, sizeof err)) return RAILS_OK;
    rails_set_error("%s", err);
    return RAILS_EINVAL;
}

double rails_iter_poly_hi(const rails_iter *it, int pass)
{
    if (it->eig_max > 0.0) return it->eig_max;
    return pass == RAILS_PC_PASS_DIAG ? it->hi_jacobi : it->hi_plain;
}

int rails_iter_grow_work(rails_ctx *c, rails_iter *it, int cols, unsigned want)
{
    bool missing = false; // a setting made after the last solve may ask for a panel that is not there yet
    for (int k = 0; k < W_COUNT; ++k) missing = missing || ((want >> k & 1) && !it->w[k]);
    if (cols <= it->work_cols && !missing) return RAILS_OK;
    cols = std::max(cols, it->work_cols);
    for (int k = 0; k < W_COUNT; ++k) want |= it->w[k] ? 1u << k : 0u;
    release_work(it);
    for (int k = 0; k < W_COUNT; ++k)
        if (want >> k & 1) {
            RAILS_TRY(rails_panel_create(c, it->m, cols, &it->w[k]));
            RAILS_HIP_CHECK(hipMemsetAsync(it->w[k]->d, 0, (size_t)it->m * it->w[k]->ld * sizeof(double), c->stream));
        }
    it->work_cols = cols;
    return RAILS_OK;
}

int rails_iter_grow_cols(rails_ctx *c, rails_iter *it, int nc)
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

extern "C" void rails_iter_destroy(rails_iter *it)
{
    if (!it) return;
    if (it->ctx) {
        hipSetDevice(it->ctx->device);
        hipStreamSynchronize(it->ctx->stream);
    }
    rails_iter_amg_release(it);
    release_work(it);
    hipFree(it->dinv);
    hipFree(it->bj_dev);
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
        RAILS_TRY(rails_iter_grant(it, RAILS_PC_POLY, (int)value, "rails_iter_set"));
        it->poly_degree = (int)value;
    } else if (n == "poly_ratio") {
        RAILS_REQUIRE(value > 1.0, "rails_iter_set: poly_ratio %g is not above 1", value);
        it->poly_ratio = value;
    } else if (n == "eig_max") {
        RAILS_REQUIRE(value >= 0.0, "rails_iter_set: eig_max %g", value);
        it->eig_max = value;
    } else if (n == "poly_fused")
        it->poly_fused = value != 0.0;
    else if (n == "block_jacobi") {
        if (value != 0.0) RAILS_TRY(rails_iter_grant(it, RAILS_PC_BLOCK_JACOBI, 1, "rails_iter_set"));
        it->block_jacobi = value != 0.0;
    } else if (n == "amg") {
        if (value != 0.0) RAILS_TRY(rails_iter_grant(it, RAILS_PC_AMG, 1, "rails_iter_set"));
        it->amg = value != 0.0;
    } else if (n == "block_amg") {
        if (value != 0.0) RAILS_TRY(rails_iter_grant(it, RAILS_PC_BLOCK_AMG, 1, "rails_iter_set"));
        it->block_amg = value != 0.0;
    } else if (n == "amg_degree") {
        RAILS_REQUIRE(value >= 0.0 && value <= 8.0 && value == std::floor(value), "rails_iter_set: amg_degree %g is not a whole number in 0 .. 8", value);
        it->amg_degree = (int)value;
    } else if (n == "amg_ratio") {
        RAILS_REQUIRE(value > 1.0, "rails_iter_set: amg_ratio %g is not above 1", value);
        it->amg_ratio = value;
    } else if (n == "amg_theta") {
        RAILS_REQUIRE(value >= 0.0 && value < 1.0, "rails_iter_set: amg_theta %g is not in [0, 1)", value);
        if (value != it->amg_theta) rails_iter_amg_release(it);
        it->amg_theta = value;
    } else if (n == "amg_coarse") {
        RAILS_REQUIRE(value >= 1.0 && value <= RAILS_AMG_MAX_COARSE && value == std::floor(value), "rails_iter_set: amg_coarse %g is not a whole number in 1 .. %d", value,
                      RAILS_AMG_MAX_COARSE);
        if ((int)value != it->amg_coarse) rails_iter_amg_release(it);
        it->amg_coarse = (int)value;
    } else {
        rails_set_error("rails_iter_set: no setting named '%s' (tolerance, max_iterations, jacobi, check_every, strict, poly_degree, poly_ratio, eig_max, poly_fused, amg, amg_degree, "
                        "amg_ratio, amg_theta, amg_coarse, block_jacobi, block_amg)", name);
        return RAILS_EINVAL;
    }
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
    const double hi = it->poly_degree > 0 ? rails_iter_poly_hi(it, rails_precond_effect_of(rails_iter_facts(it)).pass) : 0.0;
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
