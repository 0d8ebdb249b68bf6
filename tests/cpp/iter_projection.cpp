// C++ test of the iterative A^-1 object and the extended Krylov projection through the header-only classes and the C ABI alone: the
// program of projection_lu.cpp with a rails_iter (conjugate gradients, Jacobi) in place of the sparse LU.  It builds a 2D Laplacian, checks
// A (A^-1 x) = x to 10 tol, and solves A X + X A' + B B' = 0 with "Projection method" 2.2 and set_inverse on both back ends of the solver
// template.  Built by rails_amd/csrc/Makefile into rails_amd/lib/iter_projection, run by tests/test_gpu_iter_cpp.py.  Prints OK at the end.
#include <cmath>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "rails/HipSolverOps.hpp"
#include "rails/SubspaceSolverOps.hpp"

struct ParameterList {
    std::map<std::string, double> p;
    template <typename T>
    T get(std::string const &name, T def)
    {
        auto it = p.find(name);
        return it == p.end() ? def : (T)it->second;
    }
};

int main()
{
    const int k = 20, m = k * k, p = 2;
    const double tol = 1e-10;
    // A = 5-point Laplacian (negative definite)
    std::vector<int64_t> rp(1, 0);
    std::vector<int32_t> ci;
    std::vector<double> va;
    for (int y = 0; y < k; ++y)
        for (int x = 0; x < k; ++x) {
            const int r = x + k * y;
            auto add = [&](int c, double v) {
                ci.push_back(c);
                va.push_back(v);
            };
            if (y > 0) add(r - k, 1.0);
            if (x > 0) add(r - 1, 1.0);
            add(r, -4.0);
            if (x < k - 1) add(r + 1, 1.0);
            if (y < k - 1) add(r + k, 1.0);
            rp.push_back((int64_t)ci.size());
        }
    rails_ctx *ctx = nullptr;
    if (rails_ctx_create(0, nullptr, &ctx) != RAILS_OK) {
        std::printf("no gfx950 device: %s\n", rails_last_error());
        return 2;
    }
    rails::set_default_context(ctx);
    int failures = 0;
    {
        rails::HipOperatorWrapper A(ctx, m, m, rp.data(), ci.data(), va.data());
        rails_csr *A_handle = nullptr;
        if (rails_csr_create(ctx, m, m, rp.data(), ci.data(), va.data(), &A_handle) != RAILS_OK) {
            std::printf("rails_csr_create: %s\nFAILED\n", rails_last_error());
            return 1;
        }
        rails_iter *it = nullptr;
        if (rails_iter_create(ctx, A_handle, RAILS_ITER_CG, nullptr, &it) != RAILS_OK || rails_iter_set(it, "tolerance", tol) != RAILS_OK) {
            std::printf("rails_iter_create: %s\nFAILED\n", rails_last_error());
            return 1;
        }
        {
            rails::HipOperatorWrapper Ainv(ctx, it);
            // A (A^-1 x) = x, column by column
            rails::HipMultiVectorWrapper x(m, 3, ctx);
            rails_ctx_set_seed(ctx, 3, 0);
            x.random();
            rails::HipMultiVectorWrapper y = Ainv * x;
            rails::HipMultiVectorWrapper z = A * y;
            z -= x;
            std::vector<double> zh((size_t)m * 3), xh((size_t)m * 3);
            z.to_host(zh.data(), m);
            x.to_host(xh.data(), m);
            for (int j = 0; j < 3; ++j) {
                double zz = 0.0, xx = 0.0;
                for (int i = 0; i < m; ++i) {
                    zz += zh[i + (size_t)j * m] * zh[i + (size_t)j * m];
                    xx += xh[i + (size_t)j * m] * xh[i + (size_t)j * m];
                }
                const double err = std::sqrt(zz / xx);
                std::printf("column %d: A (A^-1 x) - x: %.2e relative\n", j, err);
                if (!(err <= 10 * tol)) failures++;
            }
            double info[13] = {};
            rails_iter_stats(it, info, 13);
            std::printf("most iterations %g, inner products %g, launches %g, unconverged columns %g, products %g\n", info[0], info[1], info[2], info[3], info[7]);
            if (info[3] != 0.0) failures++;

            rails::HipMultiVectorWrapper B(m, p, ctx);
            rails_ctx_set_seed(ctx, 7, 0);
            B.random();
            ParameterList params;
            params.p = {{"Expand size", 2.0}, {"Lanczos iterations", 10.0}, {"Tolerance", 1e-8}, {"Projection method", 2.2}};
            for (int backend = 0; backend < 2; ++backend) {
                rails_ctx_set_seed(ctx, 11, 0);
                rails::HostDenseMatrix T;
                int ret, trips;
                rails::HipMultiVectorWrapper Vd;
                if (backend == 0) {
                    rails::HipSolver solver(A, B, A);
                    solver.set_verbose(false);
                    if (solver.set_parameters(params) != 0) failures++;
                    solver.set_inverse(Ainv);
                    rails::HipMultiVectorWrapper V(m, 1, ctx);
                    ret = solver.solve(V, T);
                    trips = solver.trips();
                    Vd = V;
                } else {
                    auto basis = std::make_shared<rails::SubspaceBasis>(ctx, m, m, 2 * (100 + 4 + 100) + p + 128);
                    rails::SubspaceMultiVector Bc = rails::SubspaceMultiVector::Absorb(basis, B);
                    rails::SubspaceOperator Ac(A, basis);
                    rails::SubspaceSolver solver(Ac, Bc, Ac);
                    solver.set_verbose(false);
                    if (solver.set_parameters(params) != 0) failures++;
                    solver.set_inverse(rails::SubspaceOperator(Ainv, basis));
                    rails::SubspaceMultiVector V(basis, 1);
                    ret = solver.solve(V, T);
                    trips = solver.trips();
                    Vd = V.materialise();
                }
                // true residual ||A X + X A' + B B'||_F / ||B B'||_F, densely on the host (small m)
                rails::HipMultiVectorWrapper AV = A * Vd;
                const int kk = Vd.N();
                double tr = 0.0;
                std::vector<double> Vh((size_t)m * kk), Bh((size_t)m * p), AVh((size_t)m * kk);
                Vd.to_host(Vh.data(), m);
                B.to_host(Bh.data(), m);
                AV.to_host(AVh.data(), m);
                std::vector<double> L1((size_t)m * kk, 0.0), L2((size_t)m * kk, 0.0); // AV T, V T
                for (int j = 0; j < kk; ++j)
                    for (int l = 0; l < kk; ++l)
                        for (int i = 0; i < m; ++i) {
                            L1[i + (size_t)j * m] += AVh[i + (size_t)l * m] * T(l, j);
                            L2[i + (size_t)j * m] += Vh[i + (size_t)l * m] * T(l, j);
                        }
                double bb = 0.0;
                for (int j = 0; j < m; ++j)
                    for (int i = 0; i < m; ++i) {
                        double r = 0.0, b = 0.0;
                        for (int l = 0; l < kk; ++l) r += L1[i + (size_t)l * m] * Vh[j + (size_t)l * m] + L2[i + (size_t)l * m] * AVh[j + (size_t)l * m];
                        for (int l = 0; l < p; ++l) b += Bh[i + (size_t)l * m] * Bh[j + (size_t)l * m];
                        tr += (r + b) * (r + b);
                        bb += b * b;
                    }
                const double rel = std::sqrt(tr / bb);
                std::printf("%s back end, projection 2.2: return %d, %d trips, %d vectors, true residual %.2e\n", backend ? "coordinate-space" : "direct", ret,
                            trips, kk, rel);
                if (ret != 0 || !(rel < 1e-6)) failures++;
            }
            rails_iter_stats(it, info, 13);
            std::printf("since creation: %g solves, %g columns, %g inner iterations, %g flagged columns\n", info[8], info[9], info[10], info[11]);
            if (info[11] != 0.0) failures++;
        }
        rails_iter_destroy(it);
        rails_csr_destroy(A_handle);
    }
    rails_ctx_destroy(ctx);
    std::printf(failures ? "FAILED\n" : "OK\n");
    return failures ? 1 : 0;
}
