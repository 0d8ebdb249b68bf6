// sprhs.hip -- the sparse right-hand side as a library object (include/rails_hip.h: rails_sprhs): B (m x p) and its transpose as
// rectangular CSR operators, products with either through the rectangular SpMM, and the plan of the fused Lanczos' transposed
// product (rails_internal.h: rails_sprhs, lanczos.hip: k_sprhs_bt).  The host part is sprhs_host.cpp.
#include "rails_internal.h"

#include <algorithm>

namespace {

template <typename T>
int upload(rails_ctx *c, const std::vector<T> &h, T **d)
{
    *d = nullptr;
    RAILS_HIP_CHECK(hipMalloc((void **)d, std::max<size_t>(h.size(), 1) * sizeof(T)));
    if (!h.empty()) RAILS_HIP_CHECK(hipMemcpyAsync(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, c->stream));
    return RAILS_OK;
}

// long transposed rows cut into items of RAILS_SPRHS_CHUNK entries
int build_plan(rails_ctx *c, rails_sprhs *S, const std::vector<int64_t> &t_rowptr)
{
    std::vector<int64_t> item_beg, long_item0;
    std::vector<int32_t> item_len, long_row;
    for (int j = 0; j < S->p; ++j) {
        const int64_t b = t_rowptr[j], e = t_rowptr[j + 1];
        if (e - b <= RAILS_SPRHS_SHORT) continue;
        long_row.push_back(j);
        long_item0.push_back((int64_t)item_beg.size());
        for (int64_t q = b; q < e; q += RAILS_SPRHS_CHUNK) {
            item_beg.push_back(q);
            item_len.push_back((int32_t)std::min<int64_t>(RAILS_SPRHS_CHUNK, e - q));
        }
    }
    long_item0.push_back((int64_t)item_beg.size());
    S->n_items = (int64_t)item_beg.size();
    S->n_long = (int64_t)long_row.size();
    RAILS_TRY(upload(c, item_beg, &S->item_beg));
    RAILS_TRY(upload(c, item_len, &S->item_len));
    RAILS_TRY(upload(c, long_row, &S->long_row));
    RAILS_TRY(upload(c, long_item0, &S->long_item0));
    RAILS_HIP_CHECK(hipMalloc((void **)&S->item_partial, std::max<size_t>((size_t)S->n_items, 1) * sizeof(double)));
    RAILS_HIP_CHECK(rails_stream_sync(c)); // the host vectors go away
    return RAILS_OK;
}

} // namespace

extern "C" int rails_sprhs_create(rails_ctx *c, int64_t m_local, int p, const int64_t *rowptr, const int32_t *col, const double *val,
                                  rails_sprhs **out)
{
    if (c) hipSetDevice(c->device); // allocations and launches go to the context's device whatever the caller's current device is
    RAILS_REQUIRE(c && out && rowptr, "rails_sprhs_create: null argument");
    RAILS_REQUIRE(c->nranks == 1 && !c->rccl,
                  "rails_sprhs_create: single GPU only (B'W of a row-partitioned B needs an all-reduce; the context has a partition or a communicator)");
    RAILS_REQUIRE(m_local >= 0 && m_local <= 0x7fffffffLL && p >= 0, "rails_sprhs_create: bad shape %lld x %d", (long long)m_local, p);
    RAILS_REQUIRE(rowptr[0] == 0, "rails_sprhs_create: rowptr[0] != 0");
    for (int64_t i = 0; i < m_local; ++i)
        RAILS_REQUIRE(rowptr[i + 1] >= rowptr[i], "rails_sprhs_create: rowptr not monotone at row %lld", (long long)i);
    const int64_t nnz = rowptr[m_local];
    // the transposed form (p + 1 row pointers; one more for the 1 x m operator that stands in for p = 0); validates the columns
    std::vector<int64_t> t_rowptr((size_t)p + 2, 0);
    std::vector<int32_t> t_col((size_t)nnz);
    std::vector<double> t_val((size_t)nnz);
    RAILS_TRY(rails_csr_transpose_host(m_local, p, rowptr, col, val, t_rowptr.data(), t_col.data(), t_val.data()));
    t_rowptr[(size_t)p + 1] = nnz;
    rails_sprhs *S = new rails_sprhs();
    S->ctx = c;
    S->m = m_local;
    S->p = p;
    S->nnz = nnz;
    const int64_t pc = std::max(p, 1);
    int rc = rails_csr_gram_norm2_host(m_local, p, rowptr, col, val, t_rowptr.data(), t_col.data(), t_val.data(), &S->gram_norm2);
    if (rc == RAILS_OK) rc = rails_csr_create_rect(c, m_local, pc, rowptr, col, val, &S->B);
    if (rc == RAILS_OK) rc = rails_csr_create_rect(c, pc, std::max<int64_t>(m_local, 1), t_rowptr.data(), t_col.data(), t_val.data(), &S->Bt);
    if (rc == RAILS_OK) rc = build_plan(c, S, t_rowptr);
    if (rc != RAILS_OK) {
        rails_sprhs_destroy(S);
        return rc;
    }
    *out = S;
    return RAILS_OK;
}

extern "C" void rails_sprhs_destroy(rails_sprhs *S)
{
    if (!S) return;
    hipStreamSynchronize(S->ctx->stream);
    if (S->B) rails_csr_destroy(S->B);
    if (S->Bt) rails_csr_destroy(S->Bt);
    if (S->item_beg) hipFree(S->item_beg);
    if (S->item_len) hipFree(S->item_len);
    if (S->long_row) hipFree(S->long_row);
    if (S->long_item0) hipFree(S->long_item0);
    if (S->item_partial) hipFree(S->item_partial);
    delete S;
}

extern "C" int64_t rails_sprhs_rows(const rails_sprhs *S) { return S ? S->m : -1; }
extern "C" int64_t rails_sprhs_cols(const rails_sprhs *S) { return S ? S->p : -1; }
extern "C" int64_t rails_sprhs_nnz(const rails_sprhs *S) { return S ? S->nnz : -1; }
extern "C" double rails_sprhs_gram_norm2(const rails_sprhs *S) { return S ? S->gram_norm2 : -1.0; }

extern "C" int rails_sprhs_apply(rails_ctx *c, rails_sprhs *S, int trans, const rails_panel *X, int xc0, int nc, rails_panel *Y, int yc0)
{
    RAILS_REQUIRE(c && S && X && Y, "rails_sprhs_apply: null argument");
    RAILS_REQUIRE(c == S->ctx, "rails_sprhs_apply: the object belongs to another context");
    RAILS_REQUIRE(xc0 >= 0 && nc >= 0 && xc0 + nc <= X->cap, "rails_sprhs_apply: X columns [%d,%d) outside capacity %d", xc0, xc0 + nc, X->cap);
    RAILS_REQUIRE(yc0 >= 0 && yc0 + nc <= Y->cap, "rails_sprhs_apply: Y columns [%d,%d) outside capacity %d", yc0, yc0 + nc, Y->cap);
    const int64_t xr = trans ? S->m : S->p, yr = trans ? S->p : S->m;
    RAILS_REQUIRE(X->m == xr && Y->m == yr, "rails_sprhs_apply: B%s is %lld x %lld, X has %lld rows, Y %lld", trans ? "'" : "", (long long)yr,
                  (long long)xr, (long long)X->m, (long long)Y->m);
    if (nc == 0 || yr == 0) return RAILS_OK;
    if (xr == 0) return rails_panel_fill(c, Y, yc0, nc, 0.0); // an empty sum
    return rails_spmm(c, trans ? S->Bt : S->B, 0, X, xc0, nc, Y, yc0);
}

extern "C" int rails_csr_create_sprhs(rails_ctx *c, rails_sprhs *S, rails_csr **out)
{
    RAILS_REQUIRE(c && S && out, "rails_csr_create_sprhs: null argument");
    RAILS_REQUIRE(c == S->ctx, "rails_csr_create_sprhs: the object belongs to another context");
    rails_csr *A = new rails_csr();
    A->ctx = c;
    A->m = S->m;
    A->ncols_ext = S->p;
    A->nnz = S->nnz;
    A->kind = rails_csr::SPRHS;
    A->delegate = S;
    A->last_kernel = "sprhs";
    *out = A;
    return RAILS_OK;
}

extern "C" int64_t rails_csr_cols(const rails_csr *A)
{
    if (!A) return -1;
    return (A->rect || A->kind == rails_csr::SPRHS) ? A->ncols_ext : A->m;
}

extern "C" rails_sprhs *rails_csr_sprhs(const rails_csr *A) { return A ? A->sprhs() : nullptr; }
