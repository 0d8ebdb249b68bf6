// C++ test of the sparse right-hand side through the drop-in classes (rails_amd/include/rails/): HipOperatorWrapper over a rails_sprhs
// is m x p, sizes its products by the operator and not by X, has a norm; BOperand exposes it; and rails::HipSolver with such a B gives the
// reference's known answer (test/LyapunovSolverEpetra_test.cpp:109-177; A = [0 1; -5 -5], B = -I, X = [0.62 -0.5; -0.5 0.6] to 1e-12)
// through the fused sparse Lanczos.  Built by rails_amd/csrc/Makefile into rails_amd/lib/sparse_rhs_classes, run by
// tests/test_gpu_sparse_rhs_cpp.py.  Prints OK at the end.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "rails/HipSolverOps.hpp"

using rails::HipMultiVectorWrapper;
using rails::HipOperatorWrapper;
using rails::HostDenseMatrix;

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("line %d: %s is false\n", __LINE__, #cond);     \
            failures++;                                                 \
        }                                                               \
    } while (0)

struct Parameters {
    std::map<std::string, double> p;
    template <typename T>
    T get(std::string const &name, T def)
    {
        auto it = p.find(name);
        return it == p.end() ? def : (T)it->second;
    }
};

static std::vector<double> host_of(HipMultiVectorWrapper const &X)
{
    std::vector<double> h((size_t)X.M() * std::max(X.N(), 1));
    X.to_host(h.data(), X.M());
    return h;
}

int main()
{
    rails_ctx *ctx = nullptr;
    if (rails_ctx_create(0, nullptr, &ctx) != RAILS_OK) {
        std::printf("no gfx950 device: %s\n", rails_last_error());
        return 2;
    }
    rails_ctx_set_seed(ctx, 1, 0);
    { // a 5 x 3 operator: shapes of both products, the norm
        const int m = 5, p = 3;
        const int64_t rp[] = {0, 1, 1, 3, 4, 5};
        const int32_t ci[] = {0, 0, 2, 1, 2};
        const double va[] = {2.0, -1.0, 0.5, 3.0, 1.5};
        rails_sprhs *S = nullptr;
        CHECK(rails_sprhs_create(ctx, m, p, rp, ci, va, &S) == RAILS_OK);
        HipOperatorWrapper B(ctx, S);
        CHECK(B.M() == m && B.N() == p && B.sprhs() == S);
        HipMultiVectorWrapper X(p, 2, ctx), W(m, 2, ctx);
        const double xh[] = {1.0, 2.0, 3.0, -1.0, 0.0, 4.0}, wh[] = {1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0, 2.0, 3.0, 4.0};
        X.from_host(xh, p);
        W.from_host(wh, m);
        HipMultiVectorWrapper Y = B * X, Z = B.transpose() * W;
        CHECK(Y.M() == m && Y.N() == 2 && Z.M() == p && Z.N() == 2);
        const double ywant[] = {2.0, 0.0, 0.5, 6.0, 4.5, -2.0, 0.0, 3.0, 0.0, 6.0}, zwant[] = {1.0, 3.0, 2.0, -2.0, 9.0, 7.0};
        std::vector<double> yh = host_of(Y), zh = host_of(Z);
        for (int i = 0; i < 10; ++i) CHECK(yh[i] == ywant[i]);
        for (int i = 0; i < 6; ++i) CHECK(zh[i] == zwant[i]);
        // ||B||_2 = sqrt of the largest eigenvalue of B'B = [[5 0 -0.5], [0 9 0], [-0.5 0 2.5]]: 3
        const double nb = B.norm();
        std::printf("norm of the 5 x 3 operator: %.15g\n", nb);
        CHECK(std::fabs(nb - 3.0) <= 1e-6 && nb <= 3.0 + 1e-12);
        rails_sprhs_destroy(S);
    }
    { // the known answer through the solver template
        const int n = 2;
        const int64_t a_rp[] = {0, 2, 4}, b_rp[] = {0, 1, 2};
        const int32_t a_ci[] = {0, 1, 0, 1}, b_ci[] = {0, 1};
        const double a_va[] = {0.0, 1.0, -5.0, -5.0}, b_va[] = {-1.0, -1.0};
        rails_sprhs *S = nullptr;
        CHECK(rails_sprhs_create(ctx, n, n, b_rp, b_ci, b_va, &S) == RAILS_OK);
        HipOperatorWrapper A(ctx, n, n, a_rp, a_ci, a_va), B(ctx, S);
        rails::clear_sticky_error();
        rails::HipSolver solver(A, B, A);
        CHECK(solver.B().given_as_operator() && solver.B().op().sprhs() == S);
        Parameters params;
        params.p = {{"Minimize solution space", 0.0}, {"Lanczos iterations", 10.0}, {"Expand size", 3.0}};
        CHECK(solver.set_parameters(params) == 0);
        solver.set_verbose(false);
        HipMultiVectorWrapper V(n, 1, ctx);
        HostDenseMatrix T;
        long before = 0, after = 0;
        char buf[1024];
        rails_ctx_stats(ctx, buf, sizeof(buf));
        if (const char *q = std::strstr(buf, "\"lanczos\":")) before = std::atol(q + 10);
        const int code = solver.solve(V, T);
        rails_ctx_stats(ctx, buf, sizeof(buf));
        if (const char *q = std::strstr(buf, "\"lanczos\":")) after = std::atol(q + 10);
        CHECK(code == 0 && rails::sticky_error() == RAILS_OK);
        CHECK(after - before == solver.trips() && solver.trips() >= 1); // every trip's estimate came from the fused kernel
        std::vector<double> h = host_of(V);
        const int k = V.N();
        const double want[2][2] = {{0.62, -0.5}, {-0.5, 0.6}};
        double worst = 0.0;
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) {
                double x = 0.0;
                for (int a = 0; a < k; ++a)
                    for (int b = 0; b < k; ++b) x += h[i + (size_t)a * n] * T(a, b) * h[j + (size_t)b * n];
                worst = std::fmax(worst, std::fabs(x - want[i][j]));
            }
        std::printf("known answer through the classes: return %d, %d trips, %d vectors, max |X - X_ref| %.2e, scale %.15g\n", code, solver.trips(), k,
                    worst, solver.scale());
        CHECK(worst <= 1e-12);
        rails_sprhs_destroy(S);
    }
    rails_ctx_destroy(ctx);
    std::printf(failures ? "FAILED\n" : "OK\n");
    return failures ? 1 : 0;
}
