// C++ test of continuation through the C ABI alone (include/rails_solver.h, include/rails_solution.h): a banded stable problem is
// solved, its solution object's device panel becomes the start space (rails_solver_set_start_space) of a second solver whose A is
// perturbed by 1 %, with "Restart upon start"; a third solver solves the perturbed problem cold.  Prints the start rank and the trips of
// the warm and the cold solve; ends with OK only if the warm solve converged in no more trips than the cold one.  Both back ends.  Built by
// rails_amd/csrc/Makefile into rails_amd/lib/start_space_capi, run by tests/test_gpu_start_space_cpp.py.
#include <cmath>
#include <cstdio>
#include <vector>

#include "rails_solution.h"
#include "rails_solver.h"

namespace
{

// five diagonals, diagonally dominant; `scale` multiplies the diagonal
void banded(int m, double scale, std::vector<int64_t> &rp, std::vector<int32_t> &ci, std::vector<double> &va)
{
    rp.assign(1, 0);
    ci.clear();
    va.clear();
    for (int r = 0; r < m; ++r) {
        for (int d = -2; d <= 2; ++d) {
            const int c = r + d;
            if (c < 0 || c >= m) continue;
            ci.push_back(c);
            va.push_back(d == 0 ? -scale * (3.0 + 2.0 * std::sin(0.7 * r) * std::sin(0.7 * r)) : 0.9 * std::sin(1.3 * r + 0.4 * d));
        }
        rp.push_back((int64_t)ci.size());
    }
}

rails_solver *make_solver(rails_ctx *ctx, rails_csr *A, std::vector<double> const &B, int m, int p, int backend, bool restart_upon_start)
{
    rails_solver *s = nullptr;
    if (rails_solver_create(ctx, A, nullptr, B.data(), m, p, m, &s) != RAILS_OK) return nullptr;
    const char *names[] = {"Expand size", "Lanczos iterations", "Tolerance"};
    const double values[] = {2.0, 8.0, 1e-6};
    for (int i = 0; i < 3; ++i) rails_solver_set_parameter(s, names[i], values[i]);
    if (restart_upon_start) rails_solver_set_parameter(s, "Restart upon start", 1.0);
    int pc = 0;
    rails_solver_apply_parameters(s, &pc);
    rails_solver_set_option(s, "verbose", 0.0);
    rails_solver_set_option(s, "subspace", backend ? 1.0 : 0.0);
    return pc == 0 ? s : nullptr;
}

} // namespace

int main()
{
    const int m = 300, p = 2;
    std::vector<int64_t> rp, rp2;
    std::vector<int32_t> ci, ci2;
    std::vector<double> va, va2, B((size_t)m * p);
    banded(m, 1.0, rp, ci, va);
    banded(m, 1.01, rp2, ci2, va2);
    for (int j = 0; j < p; ++j)
        for (int i = 0; i < m; ++i) B[i + (size_t)j * m] = std::sin(0.37 * (i + 1) * (j + 1)) + 0.1 * (i % 7) - 0.3;
    rails_ctx *ctx = nullptr;
    if (rails_ctx_create(0, nullptr, &ctx) != RAILS_OK) {
        std::printf("no gfx950 device: %s\n", rails_last_error());
        return 2;
    }
    rails_csr *A = nullptr, *A2 = nullptr;
    if (rails_csr_create(ctx, m, m, rp.data(), ci.data(), va.data(), &A) != RAILS_OK ||
        rails_csr_create(ctx, m, m, rp2.data(), ci2.data(), va2.data(), &A2) != RAILS_OK) {
        std::printf("rails_csr_create: %s\nFAILED\n", rails_last_error());
        return 1;
    }
    int failures = 0;
    for (int backend = 0; backend < 2; ++backend) {
        const char *name = backend ? "coordinate-space" : "direct";
        rails_solver *first = make_solver(ctx, A, B, m, p, backend, false), *warm = make_solver(ctx, A2, B, m, p, backend, true),
                     *cold = make_solver(ctx, A2, B, m, p, backend, false);
        rails_solution *sol = nullptr;
        int code = 0, k1 = 0, kw = 0, kc = 0, code_w = 0, code_c = 0, c0 = 0;
        if (!first || !warm || !cold || rails_solver_solve(first, &code, &k1) != RAILS_OK || code != 0 ||
            rails_solution_from_solver(first, &sol) != RAILS_OK) {
            std::printf("%s back end: set-up or first solve failed (code %d): %s\n", name, code, rails_last_error());
            failures++;
        } else {
            const rails_panel *P = rails_solution_panel(sol, &c0);
            const int k = rails_solution_rank(sol);
            // refusals: no column, a window past the panel
            if (rails_solver_set_start_space(warm, P, c0, 0) != RAILS_EINVAL || rails_solver_set_start_space(warm, P, c0, rails_panel_capacity(P) + 1) != RAILS_EINVAL) {
                std::printf("%s back end: a bad window was not refused\n", name);
                failures++;
            }
            if (rails_solver_set_start_space(warm, P, c0, k) != RAILS_OK || rails_solver_solve(warm, &code_w, &kw) != RAILS_OK ||
                rails_solver_solve(cold, &code_c, &kc) != RAILS_OK) {
                std::printf("%s back end: %s\n", name, rails_last_error());
                failures++;
            } else {
                double rel = 0.0;
                rails_solver_relative_residual(warm, &rel);
                std::printf("%s back end: start rank %d of %d, warm return %d in %d trips (%d vectors, relative residual %.2e), cold return %d in %d trips\n",
                            name, rails_solver_start_rank(warm), k, code_w, rails_solver_trips(warm), kw, rel, code_c, rails_solver_trips(cold));
                if (code_w != 0 || code_c != 0 || rails_solver_start_rank(warm) != k || rails_solver_trips(warm) > rails_solver_trips(cold) || !(rel < 1e-3) ||
                    rails_solver_start_rank(cold) != 1)
                    failures++;
            }
        }
        if (sol) rails_solution_destroy(sol);
        for (rails_solver *s : {first, warm, cold})
            if (s) rails_solver_destroy(s);
    }
    rails_csr_destroy(A);
    rails_csr_destroy(A2);
    rails_ctx_destroy(ctx);
    std::printf(failures ? "FAILED\n" : "OK\n");
    return failures ? 1 : 0;
}
