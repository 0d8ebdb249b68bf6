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
