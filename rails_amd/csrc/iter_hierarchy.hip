// iter_hierarchy.hip -- the iterative A^-1 operator (itsolve.hip has the map of its files): what a preconditioner keeps on the device
// beside the work panels.  The multigrid hierarchies of "amg" and "block_amg" -- release, the level panels, the one upload of what
// amg_host.h or block_amg_host.h built on the host, the two set-ups and their infos -- and the diagonal blocks of "block_jacobi"
// (block_jacobi_host.h) with theirs.  Nothing in here launches a kernel.
#include "iter_object.h"

#include <algorithm>
#include <chrono>

#include "block_amg_host.h"
#include "block_jacobi_host.h"

namespace {

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

} // namespace

void rails_iter_amg_release(rails_iter *it)
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
        hipFree(L.ginv);
    }
    hipFree(H->Ainv);
    delete H;
    it->hier = nullptr;
}

// Installs (or clears) the block-Jacobi preconditioner: where the diagonal blocks come from and what is refused of the operator and the
// block size is rails_bj_plan (block_jacobi_host.h), what of the other preconditioners iter_precond.h; the extraction and the long-double inverses are host code there too; nothing touches the device before the
// inverses stand.  Installing sets "block_jacobi" to 1.
extern "C" int rails_iter_block_jacobi(rails_ctx *c, rails_iter *it, int b, const double *blocks_host)
{
    if (c) hipSetDevice(c->device);
    RAILS_REQUIRE(c && it, "rails_iter_block_jacobi: null argument");
    RAILS_REQUIRE(c == it->ctx, "rails_iter_block_jacobi: the object belongs to another context");
    const rails_csr *A = it->A;
    const int64_t m = it->m;
    int hb = 0;
    int64_t hmb = 0;
    const int64_t *browptr = nullptr;
    const int32_t *bcol = nullptr;
    const double *bval = nullptr;
    int op = RAILS_BJ_OP_CALLBACK;
    switch (A->kind) {
    case rails_csr::STORED: op = rails_iter_host_csr(A, m) ? RAILS_BJ_OP_CSR : RAILS_BJ_OP_CSR_NO_HOST; break;
    case rails_csr::BSR:
        RAILS_REQUIRE(rails_bsr_host_arrays(A, &hb, &hmb, &browptr, &bcol, &bval), "rails_iter_block_jacobi: the block-CSR operator keeps no host copy");
        op = RAILS_BJ_OP_BSR;
        break;
    case rails_csr::LU: op = RAILS_BJ_OP_LU; break;
    case rails_csr::ITER: op = RAILS_BJ_OP_ITER; break;
    default: op = RAILS_BJ_OP_CALLBACK; break;
    }
    const bool reduces = it->reduces || A->n_ghost > 0 || A->n_send > 0;
    int source = RAILS_BJ_CLEAR, be = 0;
    char err[256] = "";
    if (rails_bj_plan(op, hb, reduces, m, b, blocks_host != nullptr, &source, &be, err, sizeof err)) {
        rails_set_error("%s", err);
        return RAILS_EINVAL;
    }
    if (source == RAILS_BJ_CLEAR) {
        RAILS_HIP_CHECK(hipStreamSynchronize(c->stream));
        hipFree(it->bj_dev);
        it->bj_dev = nullptr;
        it->bj_host.clear();
        it->bj_b = it->block_jacobi = 0;
        return RAILS_OK;
    }
    RAILS_TRY(rails_iter_grant(it, RAILS_PC_INSTALL_BLOCKS, be, "rails_iter_block_jacobi"));
    const int64_t nb = m / be;
    const size_t n = (size_t)nb * be * be;
    std::vector<double> blocks, inv(n);
    if (source != RAILS_BJ_FROM_ARGUMENT) {
        blocks.resize(n);
        if (source == RAILS_BJ_FROM_BSR)
            rails_bj_from_bsr(nb, be, browptr, bcol, bval, blocks.data());
        else
            rails_bj_from_csr(nb, be, A->h_rowptr.data(), A->h_col.data(), A->h_val.data(), blocks.data());
        blocks_host = blocks.data();
    }
    if (rails_bj_invert(nb, be, blocks_host, inv.data(), err, sizeof err)) {
        rails_set_error("%s", err);
        return RAILS_EINVAL;
    }
    double *dev = nullptr;
    RAILS_HIP_CHECK(hipStreamSynchronize(c->stream)); // (a solve still queued reads the old blocks)
    RAILS_HIP_CHECK(hipMalloc((void **)&dev, n * sizeof(double)));
    const hipError_t e = hipMemcpy(dev, inv.data(), n * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        hipFree(dev);
        RAILS_HIP_CHECK(e);
    }
    hipFree(it->bj_dev);
    it->bj_dev = dev;
    it->bj_host.swap(inv);
    it->bj_b = be;
    it->block_jacobi = 1;
    c->n_dev_alloc++;
    return RAILS_OK;
}

// the number of blocks (0: none installed) and their size; the first cap_blocks inverses exactly as uploaded
extern "C" int64_t rails_iter_block_jacobi_info(const rails_iter *it, int *b, double *inv_blocks_host, int64_t cap_blocks)
{
    RAILS_REQUIRE(it, "rails_iter_block_jacobi_info: null argument");
    const int64_t nb = it->bj_b ? it->m / it->bj_b : 0;
    if (b) *b = it->bj_b;
    if (inv_blocks_host && cap_blocks > 0 && nb > 0)
        std::copy(it->bj_host.begin(), it->bj_host.begin() + (size_t)std::min(nb, cap_blocks) * it->bj_b * it->bj_b, inv_blocks_host);
    return nb;
}

namespace {

// a level matrix of either hierarchy: its rows and scalar entries, and its operator on the device
int64_t rows_of(const rails_amg_csr &A, int) { return A.n_rows; }
int64_t nnz_of(const rails_amg_csr &A, int) { return A.nnz(); }
int make_level(rails_ctx *c, const rails_amg_csr &A, int, rails_csr **out) { return rails_csr_create(c, A.n_rows, A.n_rows, A.rowptr.data(), A.col.data(), A.val.data(), out); }
int64_t rows_of(const rails_bamg_bsr &A, int b) { return A.mb * b; }
int64_t nnz_of(const rails_bamg_bsr &A, int b) { return A.nnzb() * b * b; }
int make_level(rails_ctx *c, const rails_bamg_bsr &A, int b, rails_csr **out) { return rails_csr_create_bsr(c, A.mb, A.mb, b, A.browptr.data(), A.bcol.data(), A.bval.data(), out); }

// The upload of a hierarchy built on the host (h: rails_amg_hierarchy, b = 0, or rails_bamg_hierarchy of block size b) into a new Amg of
// the object, which has none: the level operators (make_level), P and R = P' as rectangular operators, the smoother's G of every level --
// the host vector g_host of a level into the device array g_dev of its AmgLevel -- and the dense inverse.  `t0`, `t1`: when the host build
// began and ended.  The two set-ups differ in two ways that are kept as they were, deliberate leftovers of their separate histories and
// not requirements: the scalar one drops the old hierarchy before it builds and the block one only after a build that succeeded (its
// callers do that), and the block one alone ends on a synchronisation of the stream (`sync`).
template <class Hier, class Level>
int upload(rails_ctx *c, rails_iter *it, const char *who, const Hier &h, int b, std::vector<double> Level::*g_host, double *AmgLevel::*g_dev, bool sync,
           std::chrono::steady_clock::time_point t0, std::chrono::steady_clock::time_point t1)
{
    Amg *H = new Amg;
    it->hier = H; // (released by rails_iter_amg_release, also when an upload below fails)
    H->b = b;
    H->n_coarse = rows_of(h.coarse, b);
    H->coarse_nnz = nnz_of(h.coarse, b);
    H->lv.resize(h.levels.size());
    int rc = RAILS_OK;
    hipError_t e = hipSuccess;
    for (size_t l = 0; l < h.levels.size() && rc == RAILS_OK && e == hipSuccess; ++l) {
        const Level &S = h.levels[l];
        const std::vector<double> &G = S.*g_host;
        AmgLevel &L = H->lv[l];
        L.n = rows_of(S.A, b);
        L.nnz = nnz_of(S.A, b);
        L.hi = S.hi;
        if (l == 0)
            L.A = it->A;
        else
            rc = make_level(c, S.A, b, &L.A);
        if (rc == RAILS_OK) rc = rails_csr_create_rect(c, S.P.n_rows, S.P.n_cols, S.P.rowptr.data(), S.P.col.data(), S.P.val.data(), &L.P);
        if (rc == RAILS_OK) rc = rails_csr_create_rect(c, S.R.n_rows, S.R.n_cols, S.R.rowptr.data(), S.R.col.data(), S.R.val.data(), &L.R);
        if (rc == RAILS_OK) e = hipMalloc((void **)&(L.*g_dev), G.size() * sizeof(double));
        if (rc == RAILS_OK && e == hipSuccess) e = hipMemcpy(L.*g_dev, G.data(), G.size() * sizeof(double), hipMemcpyHostToDevice);
    }
    if (rc == RAILS_OK && e == hipSuccess) e = hipMalloc((void **)&H->Ainv, h.coarse_inv.size() * sizeof(double));
    if (rc == RAILS_OK && e == hipSuccess) e = hipMemcpy(H->Ainv, h.coarse_inv.data(), h.coarse_inv.size() * sizeof(double), hipMemcpyHostToDevice);
    if (rc == RAILS_OK && e == hipSuccess && sync) e = hipStreamSynchronize(c->stream);
    if (rc != RAILS_OK || e != hipSuccess) {
        if (rc == RAILS_OK) rails_set_error("%s: device allocation or upload failed: %s", who, hipGetErrorString(e));
        rails_iter_amg_release(it);
        return rc != RAILS_OK ? rc : RAILS_EHIP;
    }
    H->host_seconds = std::chrono::duration<double>(t1 - t0).count();
    H->upload_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
    return RAILS_OK;
}

} // namespace

// Builds (or rebuilds) the multigrid hierarchy from the CSR arrays the operator's handle keeps on the host (amg_host.h) and uploads it.
// What it refuses before it looks at the entries is iter_precond.h's; it may be called with "amg" off.
extern "C" int rails_iter_amg_setup(rails_ctx *c, rails_iter *it)
{
    if (c) hipSetDevice(c->device);
    RAILS_REQUIRE(c && it, "rails_iter_amg_setup: null argument");
    RAILS_REQUIRE(c == it->ctx, "rails_iter_amg_setup: the object belongs to another context");
    RAILS_TRY(rails_iter_grant(it, RAILS_PC_SETUP_AMG, 1, "rails_iter_amg_setup"));
    rails_iter_amg_release(it);
    const rails_csr *A = it->A;
    const auto t0 = std::chrono::steady_clock::now();
    rails_amg_hierarchy h;
    RAILS_TRY(rails_amg_build_host(it->m, A->h_rowptr.data(), A->h_col.data(), A->h_val.data(), it->amg_theta, it->amg_coarse, &h));
    return upload(c, it, "rails_iter_amg_setup", h, 0, &rails_amg_level::dinv, &AmgLevel::dinv, false, t0, std::chrono::steady_clock::now());
}

// Builds (or rebuilds) the block hierarchy from the block-CSR arrays the operator's handle keeps on the host (block_amg_host.h) and
// uploads it, the level operators as block-CSR handles.  Every refusal comes before any device work.
extern "C" int rails_iter_block_amg_setup(rails_ctx *c, rails_iter *it)
{
    if (c) hipSetDevice(c->device);
    RAILS_REQUIRE(c && it, "rails_iter_block_amg_setup: null argument");
    RAILS_REQUIRE(c == it->ctx, "rails_iter_block_amg_setup: the object belongs to another context");
    RAILS_TRY(rails_iter_grant(it, RAILS_PC_SETUP_BLOCK_AMG, 1, "rails_iter_block_amg_setup"));
    int b = 0;
    int64_t mb = 0;
    const int64_t *browptr = nullptr;
    const int32_t *bcol = nullptr;
    const double *bval = nullptr;
    RAILS_REQUIRE(rails_bsr_host_arrays(it->A, &b, &mb, &browptr, &bcol, &bval), "rails_iter_block_amg_setup: the block-CSR operator keeps no host copy");
    const auto t0 = std::chrono::steady_clock::now();
    rails_bamg_hierarchy h;
    RAILS_TRY(rails_bamg_build_host(mb, b, browptr, bcol, bval, it->amg_theta, it->amg_coarse, &h));
    const auto t1 = std::chrono::steady_clock::now();
    rails_iter_amg_release(it); // (a refused rebuild leaves the hierarchy there was)
    return upload(c, it, "rails_iter_block_amg_setup", h, b, &rails_bamg_level::ginv, &AmgLevel::ginv, true, t0, t1);
}

namespace {

// rails_iter_amg_info (block 0) and rails_iter_block_amg_info (block 1) on the hierarchy of their kind
int hierarchy_info(const rails_iter *it, int block, int64_t *rows, int64_t *nnz, double *hi, int cap)
{
    const Amg *H = it->hier;
    if (!H || (H->b != 0) != (block != 0)) return 0;
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

} // namespace

// rails_iter_amg_info's conventions on the block hierarchy: rows, scalar entries (blocks times b^2) and the smoother's bound per matrix,
// then the two trailing entries.  0 when no block hierarchy has been built.
extern "C" int rails_iter_block_amg_info(const rails_iter *it, int64_t *rows, int64_t *nnz, double *hi, int cap)
{
    RAILS_REQUIRE(it && cap >= 0, "rails_iter_block_amg_info: bad argument");
    return hierarchy_info(it, 1, rows, nnz, hi, cap);
}

// The hierarchy by its matrices, the last (dense) one included: rows, entries and the Gershgorin bound hi of the smoother's interval (0 for
// the last) of matrix l in rows[l], nnz[l], hi[l], l < n.  Two more entries where cap allows: [n] the last call's cycles, the products
// inside them (with A_l, P and R) and the launches of the object's own kernels inside them; [n + 1] the set-up's host time and its upload
// time in microseconds, and in hi[n + 1] the operator complexity (the entries of all matrices over those of the first).  Returns n, 0
// when no hierarchy has been built; at most cap entries are written.
extern "C" int rails_iter_amg_info(const rails_iter *it, int64_t *rows, int64_t *nnz, double *hi, int cap)
{
    RAILS_REQUIRE(it && cap >= 0, "rails_iter_amg_info: bad argument");
    return hierarchy_info(it, 0, rows, nnz, hi, cap);
}

int rails_iter_amg_prepare(rails_ctx *c, rails_iter *it, bool block)
{
    if (!it->hier || (it->hier->b != 0) != block) RAILS_TRY(block ? rails_iter_block_amg_setup(c, it) : rails_iter_amg_setup(c, it));
    return amg_grow(c, it);
}
