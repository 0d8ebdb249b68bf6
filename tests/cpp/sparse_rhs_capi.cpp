// C++ test of the sparse right-hand side through the C ABI alone (include/rails_hip.h, include/rails_solver.h): the reference's known
// answer (test/LyapunovSolverEpetra_test.cpp:109-177) -- A = [0 1; -5 -5], B = -I given as a 2 x 2 CSR operator, X = [0.62 -0.5; -0.5 0.6]
// to 1e-12 -- with rails_sprhs_create and rails_solver_create_sparse; also what the object reports, a product in each direction, and the
// refusals of a projection method that starts from B and of a context with two ranks.  Built by rails_amd/csrc/Makefile into
// rails_amd/lib/sparse_rhs_capi, run by tests/test_gpu_sparse_rhs_cpp.py.  Prints OK at the end.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rails_solver.h"

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("line %d: %s is false (%s)\n", __LINE__, #cond, rails_last_error()); \
            failures++;                                                 \
        }                                                               \
    } while (0)

int main()
{
    rails_ctx *ctx = nullptr;
    if (rails_ctx_create(0, nullptr, &ctx) != RAILS_OK) {
        std::printf("no gfx950 device: %s\n", rails_last_error());
        return 2;
    }
    const int n = 2;
    const int64_t a_rp[] = {0, 2, 4}, b_rp[] = {0, 1, 2};
    const int32_t a_ci[] = {0, 1, 0, 1}, b_ci[] = {0, 1};
    const double a_va[] = {0.0, 1.0, -5.0, -5.0}, b_va[] = {-1.0, -1.0};
    rails_csr *A = nullptr;
    rails_sprhs *S = nullptr;
    CHECK(rails_csr_create(ctx, n, n, a_rp, a_ci, a_va, &A) == RAILS_OK);
    CHECK(rails_sprhs_create(ctx, n, n, b_rp, b_ci, b_va, &S) == RAILS_OK);
    if (failures) {
        std::printf("FAILED\n");
        return 1;
    }
    CHECK(rails_sprhs_rows(S) == 2 && rails_sprhs_cols(S) == 2 && rails_sprhs_nnz(S) == 2 && rails_sprhs_gram_norm2(S) == 2.0);
    { // the operator handle: B X and B'X of a 2 x 1 panel
        rails_csr *op = nullptr;
        rails_panel *X = nullptr, *Y = nullptr;
        const double x[] = {3.0, -4.0};
        double y[2] = {0.0, 0.0};
        CHECK(rails_csr_create_sprhs(ctx, S, &op) == RAILS_OK && rails_csr_sprhs(op) == S && rails_csr_rows(op) == 2 && rails_csr_cols(op) == 2);
        CHECK(rails_panel_create(ctx, n, 1, &X) == RAILS_OK && rails_panel_create(ctx, n, 1, &Y) == RAILS_OK);
        CHECK(rails_panel_upload(ctx, X, 0, 1, x, n) == RAILS_OK);
        for (int trans = 0; trans < 2; ++trans) {
            CHECK(rails_spmm(ctx, op, trans, X, 0, 1, Y, 0) == RAILS_OK && rails_panel_download(ctx, Y, 0, 1, y, n) == RAILS_OK);
            CHECK(y[0] == -3.0 && y[1] == 4.0);
        }
        rails_panel_destroy(X);
        rails_panel_destroy(Y);
        rails_csr_destroy(op);
    }
    rails_solver *s = nullptr;
    CHECK(rails_solver_create_sparse(ctx, A, nullptr, S, n, &s) == RAILS_OK);
    if (s) {
        int pc = -1, code = -99, k = 0;
        rails_solver_set_parameter(s, "Minimize solution space", 0.0);
        rails_solver_set_parameter(s, "Lanczos iterations", 10.0);
        rails_solver_set_parameter(s, "Expand size", 3.0);
        CHECK(rails_solver_apply_parameters(s, &pc) == RAILS_OK && pc == 0);
        rails_solver_set_option(s, "verbose", 0.0);
        CHECK(rails_solver_set_option(s, "subspace", 1.0) == RAILS_OK); // accepted and ignored: the direct back end runs
        CHECK(rails_solver_solve(s, &code, &k) == RAILS_OK && code == 0 && k >= 1 && k <= 2);
        CHECK(std::strcmp(rails_solver_backend_stats(s), "{}") == 0);
        std::vector<double> V((size_t)n * k), T((size_t)k * k);
        CHECK(rails_solver_get_V(s, V.data(), n) == RAILS_OK && rails_solver_get_T(s, T.data(), k) == RAILS_OK);
        double X[2][2] = {{0, 0}, {0, 0}};
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j)
                for (int a = 0; a < k; ++a)
                    for (int b = 0; b < k; ++b) X[i][j] += V[i + (size_t)a * n] * T[a + (size_t)b * k] * V[j + (size_t)b * n];
        const double want[2][2] = {{0.62, -0.5}, {-0.5, 0.6}};
        double worst = 0.0, rel = -1.0, scale = -1.0;
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) worst = std::fmax(worst, std::fabs(X[i][j] - want[i][j]));
        CHECK(rails_solver_relative_residual(s, &rel) == RAILS_OK && rails_solver_scale(s, &scale) == RAILS_OK);
        std::printf("known answer: return %d, %d trips, %d vectors, max |X - X_ref| %.2e, relative residual %.2e, scale %.15g\n", code,
                    rails_solver_trips(s), k, worst, rel, scale);
        CHECK(worst <= 1e-12);
        CHECK(rel >= 0.0 && rel <= 1e-7); // the Gram form of the residual bottoms out near 1e-8 (include/rails_solver.h)
        CHECK(std::fabs(scale - 1.0) <= 1e-12);
        // a projection method that starts from B needs B as a multivector: refused before the first trip
        rails_solver_set_parameter(s, "Projection method", 1.2);
        CHECK(rails_solver_apply_parameters(s, &pc) == RAILS_OK && pc == 0);
        CHECK(rails_solver_set_inverse(s, A) == RAILS_OK); // any operator of A's rows stands for the inverse here: the solve is refused before it is used
        code = -99;
        CHECK(rails_solver_solve(s, &code, &k) == RAILS_OK && code == -2);
        rails_solver_destroy(s);
    }
    { // more than one rank: refused with a message that says so
        rails_ctx *two = nullptr;
        rails_sprhs *S2 = nullptr;
        CHECK(rails_ctx_create(0, nullptr, &two) == RAILS_OK && rails_ctx_set_partition(two, 0, 2, 0, 4) == RAILS_OK);
        CHECK(rails_sprhs_create(two, n, n, b_rp, b_ci, b_va, &S2) == RAILS_EINVAL && S2 == nullptr && std::strstr(rails_last_error(), "single GPU only"));
        rails_ctx_destroy(two);
    }
    rails_sprhs_destroy(S);
    rails_csr_destroy(A);
    rails_ctx_destroy(ctx);
    std::printf(failures ? "FAILED\n" : "OK\n");
    return failures ? 1 : 0;
}
