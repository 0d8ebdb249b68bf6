// C++ test of the solution object through the C ABI alone (include/rails_solution.h): a 2D Dirichlet Laplacian is solved, the solution
// object is made from the solver (rails_solution_from_solver), and its variance, trace and eigenpairs are checked against the dense
// X = V T V' formed on the host from the downloaded V and T.  Built by rails_amd/csrc/Makefile into rails_amd/lib/solution_capi, run by
// tests/test_gpu_solution_cpp.py.  Prints OK at the end.
#include <cmath>
#include <cstdio>
#include <vector>

#include "rails_solution.h"

int main()
{
    const int g = 16, m = g * g, p = 2;
    std::vector<int64_t> rp(1, 0);
    std::vector<int32_t> ci;
    std::vector<double> va;
    for (int y = 0; y < g; ++y)
        for (int x = 0; x < g; ++x) {
            const int r = x + g * y;
            auto add = [&](int c, double v) {
                ci.push_back(c);
                va.push_back(v);
            };
            if (y > 0) add(r - g, 1.0);
            if (x > 0) add(r - 1, 1.0);
            add(r, -4.0);
            if (x < g - 1) add(r + 1, 1.0);
            if (y < g - 1) add(r + g, 1.0);
            rp.push_back((int64_t)ci.size());
        }
    std::vector<double> B((size_t)m * p);
    for (int j = 0; j < p; ++j)
        for (int i = 0; i < m; ++i) B[i + (size_t)j * m] = std::sin(0.37 * (i + 1) * (j + 1)) + 0.1 * (i % 7);
    rails_ctx *ctx = nullptr;
    if (rails_ctx_create(0, nullptr, &ctx) != RAILS_OK) {
        std::printf("no gfx950 device: %s\n", rails_last_error());
        return 2;
    }
    int failures = 0;
    rails_csr *A = nullptr;
    rails_solver *s = nullptr;
    int code = 0, k = 0, pc = 0;
    if (rails_csr_create(ctx, m, m, rp.data(), ci.data(), va.data(), &A) != RAILS_OK || rails_solver_create(ctx, A, nullptr, B.data(), m, p, m, &s) != RAILS_OK) {
        std::printf("set-up: %s\nFAILED\n", rails_last_error());
        return 1;
    }
    rails_solution *none = nullptr;
    if (rails_solution_from_solver(s, &none) == RAILS_OK) { // nothing solved yet: refused
        std::printf("a solution object before the first solve was not refused\n");
        failures++;
    }
    rails_solver_set_parameter(s, "Expand size", 3.0);
    rails_solver_set_parameter(s, "Lanczos iterations", 10.0);
    rails_solver_set_parameter(s, "Tolerance", 1e-6);
    rails_solver_apply_parameters(s, &pc);
    rails_solver_set_option(s, "verbose", 0.0);
    if (rails_solver_solve(s, &code, &k) != RAILS_OK || code != 0) {
        std::printf("solve: code %d, %s\nFAILED\n", code, rails_last_error());
        return 1;
    }
    std::vector<double> V((size_t)m * k), T((size_t)k * k), X((size_t)m * m, 0.0), VT((size_t)m * k, 0.0);
    rails_solver_get_V(s, V.data(), m);
    rails_solver_get_T(s, T.data(), k);
    for (int j = 0; j < k; ++j)
        for (int l = 0; l < k; ++l)
            for (int i = 0; i < m; ++i) VT[i + (size_t)j * m] += V[i + (size_t)l * m] * T[l + (size_t)j * k];
    for (int l = 0; l < k; ++l)
        for (int j = 0; j < m; ++j)
            for (int i = 0; i < m; ++i) X[i + (size_t)j * m] += VT[i + (size_t)l * m] * V[j + (size_t)l * m];
    double xmax = 0.0, trX = 0.0;
    for (int i = 0; i < m; ++i) trX += X[i + (size_t)i * m];
    for (double x : X) xmax = std::fmax(xmax, std::fabs(x));

    rails_solution *sol = nullptr;
    if (rails_solution_from_solver(s, &sol) != RAILS_OK) {
        std::printf("rails_solution_from_solver: %s\nFAILED\n", rails_last_error());
        return 1;
    }
    rails_solver_destroy(s); // the object holds its own copy of V
    if (rails_solution_rank(sol) != k || rails_solution_rows(sol) != m) failures++;
    // variance
    rails_panel *out = nullptr, *vec = nullptr;
    rails_panel_create(ctx, m, 1, &out);
    std::vector<double> var(m);
    if (rails_solution_variance(sol, out, 0) != RAILS_OK || rails_panel_download(ctx, out, 0, 1, var.data(), m) != RAILS_OK) {
        std::printf("variance: %s\n", rails_last_error());
        failures++;
    }
    double verr = 0.0;
    for (int i = 0; i < m; ++i) verr = std::fmax(verr, std::fabs(var[i] - X[i + (size_t)i * m]));
    // trace
    double tr = 0.0;
    if (rails_solution_trace(sol, &tr) != RAILS_OK) failures++;
    // five leading eigenpairs: residual |X z - lambda z| and orthonormality
    const int want = 5;
    int found = 0;
    std::vector<double> lam(want), Z((size_t)m * want);
    rails_panel_create(ctx, m, want, &vec);
    if (rails_solution_eigs(sol, want, 0.0, lam.data(), vec, &found) != RAILS_OK || found != want || rails_panel_download(ctx, vec, 0, want, Z.data(), m) != RAILS_OK) {
        std::printf("eigs: found %d, %s\n", found, rails_last_error());
        failures++;
    }
    double resid = 0.0, orth = 0.0, share = 0.0;
    for (int q = 0; q < found; ++q) {
        for (int i = 0; i < m; ++i) {
            double r = -lam[q] * Z[i + (size_t)q * m];
            for (int j = 0; j < m; ++j) r += X[i + (size_t)j * m] * Z[j + (size_t)q * m];
            resid = std::fmax(resid, std::fabs(r));
        }
        for (int q2 = 0; q2 <= q; ++q2) {
            double d = 0.0;
            for (int i = 0; i < m; ++i) d += Z[i + (size_t)q * m] * Z[i + (size_t)q2 * m];
            orth = std::fmax(orth, std::fabs(d - (q == q2 ? 1.0 : 0.0)));
        }
        if (q > 0 && std::fabs(lam[q]) > std::fabs(lam[q - 1])) failures++;
        share += lam[q] / tr;
    }
    std::printf("k = %d: variance error %.2e (max |X| %.2e), trace %.12e against %.12e, %d eigenpairs: residual %.2e, |Z'Z - I| %.2e, share of the trace %.4f\n", k, verr, xmax,
                tr, trX, found, resid, orth, share);
    if (!(verr <= 1e-12 * xmax) || !(std::fabs(tr - trX) <= 1e-12 * std::fabs(trX)) || !(resid <= 1e-11 * xmax * m) || !(orth <= 1e-11) || !(share <= 1.0 + 1e-12)) failures++;
    rails_panel_destroy(out);
    rails_panel_destroy(vec);
    rails_solution_destroy(sol);
    rails_csr_destroy(A);
    rails_ctx_destroy(ctx);
    std::printf(failures ? "FAILED\n" : "OK\n");
    return failures ? 1 : 0;
}
