// C++ test of the nullspace option through the C ABI alone (include/rails_solver.h): a pure Neumann 2D Laplacian, whose kernel is the
// constants, solved with rails_solver_set_nullspace on both back ends; V must come out orthogonal to the constants and the solve must
// converge.  Also the refusal of a nullspace without an independent column.  Built by rails_amd/csrc/Makefile into
// rails_amd/lib/nullspace_capi, run by tests/test_gpu_nullspace_cpp.py.  Prints OK at the end.
#include <cmath>
#include <cstdio>
#include <vector>

#include "rails_solver.h"

int main()
{
    const int k = 16, m = k * k, p = 2;
    // A = Neumann 5-point Laplacian (negative semidefinite): the diagonal is minus the number of neighbours
    std::vector<int64_t> rp(1, 0);
    std::vector<int32_t> ci;
    std::vector<double> va;
    for (int y = 0; y < k; ++y)
        for (int x = 0; x < k; ++x) {
            const int r = x + k * y;
            const int nb = (y > 0) + (x > 0) + (x < k - 1) + (y < k - 1);
            auto add = [&](int c, double v) {
                ci.push_back(c);
                va.push_back(v);
            };
            if (y > 0) add(r - k, 1.0);
            if (x > 0) add(r - 1, 1.0);
            add(r, -(double)nb);
            if (x < k - 1) add(r + 1, 1.0);
            if (y < k - 1) add(r + k, 1.0);
            rp.push_back((int64_t)ci.size());
        }
    // B: smooth columns with their means removed (B in the complement of the kernel)
    std::vector<double> B((size_t)m * p), N(m, 1.0), Z((size_t)m * 2, 0.0);
    for (int j = 0; j < p; ++j) {
        double mean = 0.0;
        for (int i = 0; i < m; ++i) mean += (B[i + (size_t)j * m] = std::sin(0.37 * (i + 1) * (j + 1)) + 0.1 * (i % 7));
        mean /= m;
        for (int i = 0; i < m; ++i) B[i + (size_t)j * m] -= mean;
    }
    rails_ctx *ctx = nullptr;
    if (rails_ctx_create(0, nullptr, &ctx) != RAILS_OK) {
        std::printf("no gfx950 device: %s\n", rails_last_error());
        return 2;
    }
    int failures = 0;
    rails_csr *A = nullptr;
    if (rails_csr_create(ctx, m, m, rp.data(), ci.data(), va.data(), &A) != RAILS_OK) {
        std::printf("rails_csr_create: %s\nFAILED\n", rails_last_error());
        return 1;
    }
    const char *names[] = {"Expand size", "Lanczos iterations", "Tolerance"};
    const double values[] = {3.0, 10.0, 1e-8};
    for (int backend = 0; backend < 2; ++backend) {
        rails_solver *s = nullptr;
        int code = 0, kk = 0, pc = 0;
        if (rails_solver_create(ctx, A, nullptr, B.data(), m, p, m, &s) != RAILS_OK) {
            std::printf("rails_solver_create: %s\n", rails_last_error());
            failures++;
            continue;
        }
        for (int i = 0; i < 3; ++i) rails_solver_set_parameter(s, names[i], values[i]);
        rails_solver_apply_parameters(s, &pc);
        rails_solver_set_option(s, "verbose", 0.0);
        rails_solver_set_option(s, "subspace", backend ? 1.0 : 0.0);
        // a nullspace without an independent column is refused, V and T untouched
        if (rails_solver_set_nullspace(s, Z.data(), m, 2) != RAILS_OK || rails_solver_solve(s, &code, &kk) != RAILS_OK || code != -2 ||
            rails_solver_nullspace_rank(s) != 0) {
            std::printf("zero nullspace: code %d (expected -2)\n", code);
            failures++;
        }
        if (rails_solver_set_nullspace(s, N.data(), m, 1) != RAILS_OK || rails_solver_solve(s, &code, &kk) != RAILS_OK) {
            std::printf("solve: %s\n", rails_last_error());
            failures++;
            rails_solver_destroy(s);
            continue;
        }
        std::vector<double> V((size_t)m * kk);
        rails_solver_get_V(s, V.data(), m);
        double worst = 0.0; // |1'v| / sqrt(m) over the columns of V
        for (int j = 0; j < kk; ++j) {
            double d = 0.0;
            for (int i = 0; i < m; ++i) d += V[i + (size_t)j * m];
            worst = std::fmax(worst, std::fabs(d) / std::sqrt((double)m));
        }
        double rel = 0.0;
        rails_solver_relative_residual(s, &rel);
        std::printf("%s back end, nullspace rank %d: return %d, %d trips, %d vectors, max |N'V| %.2e, relative residual %.2e\n",
                    backend ? "coordinate-space" : "direct", rails_solver_nullspace_rank(s), code, rails_solver_trips(s), kk, worst, rel);
        if (code != 0 || rails_solver_nullspace_rank(s) != 1 || !(worst < 1e-10) || !(rel < 1e-6)) failures++;
        rails_solver_destroy(s);
    }
    rails_csr_destroy(A);
    rails_ctx_destroy(ctx);
    std::printf(failures ? "FAILED\n" : "OK\n");
    return failures ? 1 : 0;
}
