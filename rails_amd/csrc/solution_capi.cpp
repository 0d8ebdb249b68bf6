// solution_capi.cpp -- the solution object of include/rails_solution.h, X = U S U', in terms of the library's own entry points: every
// reduction over rows is a rails_gram (so it holds under a row partition), the small algebra is on the host, the m x k work is the
// kernels of dense_*.hip, orth.hip and solution.hip.  rails_solution_from_solver lives in solver_capi.cpp (it reads the solver object).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <numeric>
#include <vector>

#include "rails_solution.h"

void rails_set_error(const char *fmt, ...);

struct rails_solution {
    rails_ctx *ctx = nullptr;
    rails_panel *own = nullptr; // the device copy, when the object keeps one
    const rails_panel *U = nullptr;
    int c0 = 0, k = 0;
    int64_t m = 0;
    std::vector<double> S; // k x k column-major, symmetric
};

#define SOL_REQUIRE(cond, ...)                                                                                                              \
    do {                                                                                                                                   \
        if (!(cond)) {                                                                                                                     \
            rails_set_error(__VA_ARGS__);                                                                                                  \
            return RAILS_EINVAL;                                                                                                           \
        }                                                                                                                                  \
    } while (0)
#define SOL_TRY(expr)                                                                                                                      \
    do {                                                                                                                                   \
        int rc__ = (expr);                                                                                                                 \
        if (rc__ != RAILS_OK) return rc__;                                                                                                 \
    } while (0)

namespace
{
// releases a temporary panel on every way out
struct PanelGuard {
    rails_panel *p = nullptr;
    ~PanelGuard()
    {
        if (p) rails_panel_destroy(p);
    }
};
} // namespace

extern "C" int rails_solution_create(rails_ctx *ctx, const rails_panel *U, int c0, int k, const double *S_host, int lds, int copy, rails_solution **out)
try {
    SOL_REQUIRE(ctx && U && out, "rails_solution_create: null argument");
    SOL_REQUIRE(k >= 1 && c0 >= 0 && c0 + k <= rails_panel_capacity(U), "rails_solution_create: columns [%d,%d) outside capacity %d", c0, c0 + k, rails_panel_capacity(U));
    SOL_REQUIRE(S_host && lds >= k, "rails_solution_create: bad small matrix (leading dimension %d < %d)", lds, k);
    rails_solution *s = new rails_solution();
    s->ctx = ctx;
    s->k = k;
    s->m = rails_panel_rows(U);
    s->S.resize((size_t)k * k);
    for (int j = 0; j < k; ++j)
        for (int i = 0; i < k; ++i) s->S[i + (size_t)j * k] = 0.5 * (S_host[i + (size_t)j * lds] + S_host[j + (size_t)i * lds]);
    if (copy) {
        int rc = rails_panel_create(ctx, s->m, k, &s->own);
        if (rc == RAILS_OK) rc = rails_panel_copy(ctx, U, c0, k, s->own, 0);
        if (rc != RAILS_OK) {
            if (s->own) rails_panel_destroy(s->own);
            delete s;
            return rc;
        }
        s->U = s->own;
        s->c0 = 0;
    } else {
        s->U = U;
        s->c0 = c0;
    }
    *out = s;
    return RAILS_OK;
} catch (std::bad_alloc const &) {
    rails_set_error("rails_solution_create: out of host memory");
    return RAILS_ENOMEM;
}

extern "C" int rails_solution_destroy(rails_solution *s)
{
    if (!s) return RAILS_OK;
    if (s->own) rails_panel_destroy(s->own);
    delete s;
    return RAILS_OK;
}

extern "C" int rails_solution_rank(const rails_solution *s) { return s ? s->k : -1; }
extern "C" int64_t rails_solution_rows(const rails_solution *s) { return s ? s->m : -1; }
extern "C" const rails_panel *rails_solution_panel(const rails_solution *s, int *c0)
{
    if (!s) return nullptr;
    if (c0) *c0 = s->c0;
    return s->U;
}
extern "C" const double *rails_solution_small(const rails_solution *s) { return s ? s->S.data() : nullptr; }

extern "C" int rails_solution_variance(rails_solution *s, rails_panel *out, int c0)
{
    SOL_REQUIRE(s && out, "rails_solution_variance: null argument");
    return rails_panel_rowquad(s->ctx, s->U, s->c0, s->k, s->S.data(), s->k, out, c0);
}

extern "C" int rails_solution_trace(rails_solution *s, double *tr)
try {
    SOL_REQUIRE(s && tr, "rails_solution_trace: null argument");
    const int k = s->k;
    std::vector<double> G((size_t)k * k);
    SOL_TRY(rails_gram(s->ctx, s->U, s->c0, k, s->U, s->c0, k, G.data(), k));
    double t = 0.0;
    for (int j = 0; j < k; ++j)
        for (int i = 0; i < k; ++i) t += s->S[i + (size_t)j * k] * G[j + (size_t)i * k];
    *tr = t;
    return RAILS_OK;
} catch (std::bad_alloc const &) {
    rails_set_error("rails_solution_trace: out of host memory");
    return RAILS_ENOMEM;
}

extern "C" int rails_solution_apply(rails_solution *s, const rails_panel *W, int c0, int nc, rails_panel *Y, int yc0)
try {
    SOL_REQUIRE(s && W && Y, "rails_solution_apply: null argument");
    SOL_REQUIRE(nc >= 0 && c0 >= 0 && yc0 >= 0 && c0 + nc <= rails_panel_capacity(W) && yc0 + nc <= rails_panel_capacity(Y), "rails_solution_apply: bad windows");
    SOL_REQUIRE(rails_panel_rows(W) == s->m && rails_panel_rows(Y) == s->m, "rails_solution_apply: the solution has %lld rows, W %lld, Y %lld", (long long)s->m,
                (long long)rails_panel_rows(W), (long long)rails_panel_rows(Y));
    SOL_REQUIRE(Y != s->U && rails_panel_device_ptr(Y) != rails_panel_device_ptr(s->U), "rails_solution_apply: Y is the solution's own panel");
    if (nc == 0 || s->m == 0) return RAILS_OK;
    const int k = s->k;
    std::vector<double> C((size_t)k * nc), D((size_t)k * nc);
    SOL_TRY(rails_gram(s->ctx, s->U, s->c0, k, W, c0, nc, C.data(), k));
    rails_dgemm('N', 'N', k, nc, k, 1.0, s->S.data(), k, C.data(), k, 0.0, D.data(), k);
    return (nc > 256 ? rails_panel_gemm_wide : rails_panel_gemm)(s->ctx, 1.0, s->U, s->c0, k, D.data(), k, nc, 0.0, Y, yc0);
} catch (std::bad_alloc const &) {
    rails_set_error("rails_solution_apply: out of host memory");
    return RAILS_ENOMEM;
}

extern "C" int rails_solution_eigs(rails_solution *s, int want, double tol, double *values, rails_panel *vectors, int *found)
try {
    SOL_REQUIRE(s && values && found, "rails_solution_eigs: null argument");
    const int k = s->k;
    const int cap = (want <= 0 || want > k) ? k : want;
    SOL_REQUIRE(!vectors || (rails_panel_rows(vectors) == s->m && rails_panel_capacity(vectors) >= cap), "rails_solution_eigs: the vectors panel needs %lld rows and %d columns",
                (long long)s->m, cap);
    SOL_REQUIRE(!vectors || rails_panel_device_ptr(vectors) != rails_panel_device_ptr(s->U), "rails_solution_eigs: the vectors panel is the solution's own");
    *found = 0;
    // Q: an orthonormal basis of U (a dependent column of U leaves a column of Q that U has no part along: a zero row of R)
    PanelGuard Q;
    SOL_TRY(rails_panel_create(s->ctx, s->m, k, &Q.p));
    SOL_TRY(rails_panel_copy(s->ctx, s->U, s->c0, k, Q.p, 0));
    SOL_TRY(rails_orthogonalize(s->ctx, Q.p, 0, k, 0, nullptr));
    std::vector<double> R((size_t)k * k), RS((size_t)k * k), M((size_t)k * k), w(k);
    SOL_TRY(rails_gram(s->ctx, Q.p, 0, k, s->U, s->c0, k, R.data(), k));
    rails_dgemm('N', 'N', k, k, k, 1.0, R.data(), k, s->S.data(), k, 0.0, RS.data(), k);
    rails_dgemm('N', 'T', k, k, k, 1.0, RS.data(), k, R.data(), k, 0.0, M.data(), k);
    for (int j = 0; j < k; ++j)
        for (int i = 0; i < j; ++i) M[i + (size_t)j * k] = M[j + (size_t)i * k] = 0.5 * (M[i + (size_t)j * k] + M[j + (size_t)i * k]);
    int info = 0;
    rails_dsyev('V', 'U', k, M.data(), k, w.data(), &info);
    if (info != 0) {
        rails_set_error("rails_solution_eigs: the symmetric eigensolver returned info = %d", info);
        return RAILS_ELAPACK;
    }
    std::vector<int> order(k);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return std::abs(w[a]) > std::abs(w[b]); });
    const double wmax = std::abs(w[order[0]]);
    int nf = 0;
    std::vector<double> Z((size_t)k * cap);
    for (int q = 0; q < cap; ++q) {
        const int idx = order[q];
        if (!(std::abs(w[idx]) > tol * wmax)) break;
        values[nf] = w[idx];
        memcpy(&Z[(size_t)nf * k], &M[(size_t)idx * k], sizeof(double) * k);
        ++nf;
    }
    *found = nf;
    if (vectors && nf > 0) SOL_TRY((nf > 256 ? rails_panel_gemm_wide : rails_panel_gemm)(s->ctx, 1.0, Q.p, 0, k, Z.data(), k, nf, 0.0, vectors, 0));
    return rails_ctx_sync(s->ctx); // Q goes away here
} catch (std::bad_alloc const &) {
    rails_set_error("rails_solution_eigs: out of host memory");
    return RAILS_ENOMEM;
}

extern "C" int rails_solution_block(rails_solution *s, const int32_t *rows, int nr, const int32_t *cols, int nc, double *out, int ld)
try {
    SOL_REQUIRE(s && rows && cols && out, "rails_solution_block: null argument");
    SOL_REQUIRE(nr >= 1 && nc >= 1 && ld >= nr, "rails_solution_block: bad shape %d x %d, leading dimension %d", nr, nc, ld);
    const int k = s->k, n = nr + nc;
    std::vector<int32_t> idx(rows, rows + nr);
    idx.insert(idx.end(), cols, cols + nc);
    PanelGuard G;
    SOL_TRY(rails_panel_create(s->ctx, n, k, &G.p));
    SOL_TRY(rails_panel_move_rows(s->ctx, s->U, s->c0, k, idx.data(), n, 0, G.p, 0)); // checks the indices
    std::vector<double> Uh((size_t)n * k), US((size_t)nr * k);
    SOL_TRY(rails_panel_download(s->ctx, G.p, 0, k, Uh.data(), n)); // synchronises
    rails_dgemm('N', 'N', nr, k, k, 1.0, Uh.data(), n, s->S.data(), k, 0.0, US.data(), nr);
    rails_dgemm('N', 'T', nr, nc, k, 1.0, US.data(), nr, Uh.data() + nr, n, 0.0, out, ld);
    return RAILS_OK;
} catch (std::bad_alloc const &) {
    rails_set_error("rails_solution_block: out of host memory");
    return RAILS_ENOMEM;
}

extern "C" int rails_solution_pairs(rails_solution *s, const int32_t *ia, const int32_t *ib, int64_t n, rails_panel *out, int c0)
{
    SOL_REQUIRE(s && out, "rails_solution_pairs: null argument");
    return rails_panel_rowpair(s->ctx, s->U, s->c0, s->k, s->S.data(), s->k, ia, ib, n, out, c0);
}

// One-point maps.  Whatever only this rank can see to be wrong (an index outside its rows) is not refused before the collective -- the other
// ranks would wait in it -- but poisons the owner count of that reference unknown, so that every rank refuses after it.
extern "C" int rails_solution_maps(rails_solution *s, const int32_t *rows, int q, int correlation, rails_panel *Out, int oc0, int var_col)
try {
    SOL_REQUIRE(s && Out && (q == 0 || rows), "rails_solution_maps: null argument");
    SOL_REQUIRE(q >= 0 && q <= 64, "rails_solution_maps: q = %d outside [0, 64]", q);
    SOL_REQUIRE(oc0 >= 0 && oc0 + q <= rails_panel_capacity(Out), "rails_solution_maps: columns [%d,%d) outside capacity %d", oc0, oc0 + q, rails_panel_capacity(Out));
    SOL_REQUIRE(var_col < 0 || (var_col < rails_panel_capacity(Out) && (var_col < oc0 || var_col >= oc0 + q)),
                "rails_solution_maps: the variance column %d lies inside the maps [%d,%d) or outside capacity %d", var_col, oc0, oc0 + q, rails_panel_capacity(Out));
    SOL_REQUIRE(rails_panel_rows(Out) == s->m, "rails_solution_maps: the solution has %lld rows, Out %lld", (long long)s->m, (long long)rails_panel_rows(Out));
    SOL_REQUIRE(Out != s->U && (s->m == 0 || rails_panel_device_ptr(Out) != rails_panel_device_ptr(s->U)), "rails_solution_maps: Out is the solution's own panel");
    const int k = s->k;
    // 1. the rows this rank owns, gathered and brought to the host
    std::vector<int32_t> idx, slot;
    std::vector<double> buf((size_t)k * q + q, 0.0); // G (k x q), then the owner counts
    double *G = buf.data(), *count = buf.data() + (size_t)k * q;
    for (int j = 0; j < q; ++j) {
        if (rows[j] >= 0 && rows[j] < s->m) {
            idx.push_back(rows[j]);
            slot.push_back(j);
            count[j] = 1.0;
        } else if (rows[j] != -1)
            count[j] = 2.0; // refused by every rank below
    }
    const int nown = (int)idx.size();
    PanelGuard R;
    if (nown > 0) {
        SOL_TRY(rails_panel_create(s->ctx, nown, k, &R.p));
        SOL_TRY(rails_panel_move_rows(s->ctx, s->U, s->c0, k, idx.data(), nown, 0, R.p, 0));
        std::vector<double> Uh((size_t)nown * k), SU((size_t)k * nown);
        SOL_TRY(rails_panel_download(s->ctx, R.p, 0, k, Uh.data(), nown)); // synchronises
        // 2. G = S U[r,:]'
        rails_dgemm('N', 'T', k, nown, k, 1.0, s->S.data(), k, Uh.data(), nown, 0.0, SU.data(), k);
        for (int t = 0; t < nown; ++t) memcpy(G + (size_t)slot[t] * k, &SU[(size_t)t * k], sizeof(double) * k);
    }
    // 3. summed over the ranks; the counts say whether every reference unknown has exactly one owner
    SOL_TRY(rails_allreduce_host(s->ctx, buf.data(), (int64_t)buf.size()));
    for (int j = 0; j < q; ++j)
        SOL_REQUIRE(count[j] == 1.0, "rails_solution_maps: reference unknown %d has %s", j, count[j] == 0.0 ? "no owner (row -1 on every rank)" : "several owners or an index outside the local rows");
    // 4. Out = U G
    if (q > 0 && s->m > 0) SOL_TRY(rails_panel_gemm(s->ctx, 1.0, s->U, s->c0, k, G, k, q, 0.0, Out, oc0));
    if (!correlation && var_col < 0) return rails_ctx_sync(s->ctx); // the gathered rows go away here
    // 5. diag(X), in the caller's column or a temporary one
    PanelGuard V;
    const rails_panel *var = Out;
    int vc = var_col;
    if (var_col >= 0)
        SOL_TRY(rails_solution_variance(s, Out, var_col));
    else if (s->m > 0) {
        SOL_TRY(rails_panel_create(s->ctx, s->m, 1, &V.p));
        SOL_TRY(rails_solution_variance(s, V.p, 0));
        var = V.p;
        vc = 0;
    }
    if (correlation && q > 0) {
        // 6. the reference variances from their owners' variance column, summed like G
        std::vector<double> rv(q, 0.0);
        if (nown > 0) {
            PanelGuard Rv;
            std::vector<double> got(nown);
            SOL_TRY(rails_panel_create(s->ctx, nown, 1, &Rv.p));
            SOL_TRY(rails_panel_move_rows(s->ctx, var, vc, 1, idx.data(), nown, 0, Rv.p, 0));
            SOL_TRY(rails_panel_download(s->ctx, Rv.p, 0, 1, got.data(), nown));
            for (int t = 0; t < nown; ++t) rv[slot[t]] = got[t];
        }
        SOL_TRY(rails_allreduce_host(s->ctx, rv.data(), q));
        if (s->m > 0) SOL_TRY(rails_panel_corr_scale(s->ctx, Out, oc0, q, var, vc, rv.data(), rows));
    }
    return rails_ctx_sync(s->ctx); // the temporaries go away here
} catch (std::bad_alloc const &) {
    rails_set_error("rails_solution_maps: out of host memory");
    return RAILS_ENOMEM;
}
