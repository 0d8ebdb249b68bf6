// C++ test of the sparse LU object and the extended Krylov projection through the header-only classes and the C ABI alone: the program
// factors a 2D Laplacian itself (no pivoting: the matrix is definite), builds a rails_lu from its own L and U, checks A (A^-1 x) = x,
// and solves A X + X A' + B B' = 0 with "Projection method" 2.2 and set_inverse on both back ends of the solver template.
// Built by rails_amd/csrc/Makefile into rails_amd/lib/projection_lu, run by tests/test_gpu_projection_cpp.py.  Prints OK at the end.
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
    // A = 5-point Laplacian (negative definite), CSR and dense
    std::vector<int64_t> rp(1, 0);
    std::vector<int32_t> ci;
    std::vector<double> va, D((size_t)m * m, 0.0);
    for (int y = 0; y < k; ++y)
        for (int x = 0; x < k; ++x) {
            const int r = x + k * y;
            auto add = [&](int c, double v) {
                ci.push_back(c);
                va.push_back(v);
                D[r + (size_t)c * m] = v;
            };
            if (y > 0) add(r - k, 1.0);
            if (x > 0) add(r - 1, 1.0);
            add(r, -4.0);
            if (x < k - 1) add(r + 1, 1.0);
            if (y < k - 1) add(r + k, 1.0);
            rp.push_back((int64_t)ci.size());
        }
    // LU without pivoting (Doolittle, in place): L unit lower below the diagonal, U on and above
    for (int j = 0; j < m; ++j)
        for (int i = j + 1; i < m; ++i) {
            const double f = D[i + (size_t)j * m] / D[j + (size_t)j * m];
            if (f == 0.0) continue;
            D[i + (size_t)j * m] = f;
            for (int c = j + 1; c < m; ++c) D[i + (size_t)c * m] -= f * D[j + (size_t)c * m];
        }
    std::vector<int64_t> Lp(1, 0), Up(1, 0);
    std::vector<int32_t> Lc, Uc, perm(m);
    std::vector<double> Lv, Uv;
    for (int i = 0; i < m; ++i) {
        perm[i] = i;
        for (int c = 0; c < m; ++c) {
            const double v = D[i + (size_t)c * m];
            if (v == 0.0) continue;
            if (c < i) {
                Lc.push_back(c);
                Lv.push_back(v);
            } else {
                Uc.push_back(c);
                Uv.push_back(v);
            }
        }
        Lp.push_back((int64_t)Lc.size());
        Up.push_back((int64_t)Uc.size());
    }
    rails_ctx *ctx = nullptr;
    if (rails_ctx_create(0, nullptr, &ctx) != RAILS_OK) {
        std::printf("no gfx950 device: %s\n", rails_last_error());
        return 2;
    }
    rails::set_default_context(ctx);
    int failures = 0;
    rails_lu *lu = nullptr;
    rails_csr *lu_op = nullptr;
    if (rails_lu_create(ctx, m, Lp.data(), Lc.data(), Lv.data(), Up.data(), Uc.data(), Uv.data(), perm.data(), perm.data(), nullptr, m, &lu) != RAILS_OK ||
        rails_csr_create_lu(ctx, lu, &lu_op) != RAILS_OK) {
        std::printf("rails_lu_create: %s\nFAILED\n", rails_last_error());
        return 1;
    }
    {
        rails::HipOperatorWrapper A(ctx, m, m, rp.data(), ci.data(), va.data());
        rails::HipOperatorWrapper Ainv(ctx, lu_op);
        // A (A^-1 x) = x and A' (A^-T x) = x
        rails::HipMultiVectorWrapper x(m, 3, ctx);
        rails_ctx_set_seed(ctx, 3, 0);
        x.random();
        for (int t = 0; t < 2; ++t) {
            rails::HipMultiVectorWrapper y = t ? Ainv.transpose() * x : Ainv * x;
            rails::HipMultiVectorWrapper z = t ? A.transpose() * y : A * y;
            z -= x;
            const double err = z.norm() / x.norm();
            std::printf("A%s (A%s x) - x: %.2e relative\n", t ? "'" : "", t ? "^-T" : "^-1", err);
            if (!(err < 1e-12)) failures++;
        }
        int64_t info[10] = {};
        rails_lu_stats(lu, info, 10);
        std::printf("levels L %lld U %lld, nnz L %lld U %lld, launches of the last solve %lld\n", (long long)info[0], (long long)info[1], (long long)info[4],
                    (long long)info[5], (long long)info[6]);

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
    }
    rails_csr_destroy(lu_op);
    rails_lu_destroy(lu);
    rails_ctx_destroy(ctx);
    std::printf(failures ? "FAILED\n" : "OK\n");
    return failures ? 1 : 0;
}
