// C++ test of the block-CSR operator through the header-only classes and the C ABI alone: nothing new is needed above the C ABI, a
// handle made by rails_csr_create_bsr goes where a rails_csr goes.  The program builds a 7-point grid stencil of dense 3 x 3 blocks itself,
// as block-CSR arrays and entry by entry as CSR, and solves A X + X A' + B B' = 0 on both back ends of the solver template with the
// block-CSR handle and with the CSR handle forced to the row-gather kernel (rails_csr_set_variant 3): return code, trips, T and V have to
// agree bit for bit, since the block-CSR product is the row-gather product of the expanded matrix.
// Built by rails_amd/csrc/Makefile into rails_amd/lib/bsr_solve, run by tests/test_gpu_bsr.py.  Prints OK at the end.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
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

struct Outcome {
    int ret = -9, trips = -1, k = 0;
    std::vector<double> V, T;
};

static Outcome solve(rails_ctx *ctx, rails_csr *handle, rails::HipMultiVectorWrapper &B, int m, int p, int backend, ParameterList params)
{
    Outcome o;
    rails::HipOperatorWrapper A(ctx, handle);
    rails_ctx_set_seed(ctx, 11, 0);
    rails::HostDenseMatrix T;
    rails::HipMultiVectorWrapper Vd;
    if (backend == 0) {
        rails::HipSolver solver(A, B, A);
        solver.set_verbose(false);
        if (solver.set_parameters(params) != 0) return o;
        rails::HipMultiVectorWrapper V(m, 1, ctx);
        o.ret = solver.solve(V, T);
        o.trips = solver.trips();
        Vd = V;
    } else {
        auto basis = std::make_shared<rails::SubspaceBasis>(ctx, m, m, 2 * (100 + 4 + 100) + p + 128);
        rails::SubspaceMultiVector Bc = rails::SubspaceMultiVector::Absorb(basis, B);
        rails::SubspaceOperator Ac(A, basis);
        rails::SubspaceSolver solver(Ac, Bc, Ac);
        solver.set_verbose(false);
        if (solver.set_parameters(params) != 0) return o;
        rails::SubspaceMultiVector V(basis, 1);
        o.ret = solver.solve(V, T);
        o.trips = solver.trips();
        Vd = V.materialise();
    }
    o.k = Vd.N();
    o.V.resize((size_t)m * o.k);
    Vd.to_host(o.V.data(), m);
    o.T.resize((size_t)o.k * o.k);
    for (int j = 0; j < o.k; ++j)
        for (int i = 0; i < o.k; ++i) o.T[i + (size_t)j * o.k] = T(i, j);
    return o;
}

int main()
{
    const int nx = 6, ny = 5, nz = 4, b = 3, mb = nx * ny * nz, m = mb * b, p = 2;
    std::mt19937 g(5);
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    std::vector<int64_t> brp(1, 0), rp(1, 0);
    std::vector<int32_t> bci, ci;
    std::vector<double> bva, va;
    for (int z = 0; z < nz; ++z)
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                const int i = x + nx * (y + ny * z);
                const size_t first = bci.size();
                if (z > 0) bci.push_back(i - nx * ny);
                if (y > 0) bci.push_back(i - nx);
                if (x > 0) bci.push_back(i - 1);
                bci.push_back(i);
                if (x < nx - 1) bci.push_back(i + 1);
                if (y < ny - 1) bci.push_back(i + nx);
                if (z < nz - 1) bci.push_back(i + nx * ny);
                brp.push_back((int64_t)bci.size());
                bva.resize(bci.size() * b * b);
                for (size_t k = first * b * b; k < bva.size(); ++k) bva[k] = u(g);
                for (int r = 0; r < b; ++r) { // the diagonal dominates its row: a stable matrix
                    double sum = 0.0;
                    size_t diag = 0;
                    for (size_t q = first; q < bci.size(); ++q)
                        for (int s = 0; s < b; ++s) {
                            if (bci[q] == i && s == r)
                                diag = q * b * b + r * b + s;
                            else
                                sum += std::fabs(bva[q * b * b + r * b + s]);
                        }
                    bva[diag] = -(sum + 1.0);
                }
                for (int r = 0; r < b; ++r) {
                    for (size_t q = first; q < bci.size(); ++q)
                        for (int s = 0; s < b; ++s) {
                            ci.push_back(bci[q] * b + s);
                            va.push_back(bva[q * b * b + r * b + s]);
                        }
                    rp.push_back((int64_t)ci.size());
                }
            }
    rails_ctx *ctx = nullptr;
    if (rails_ctx_create(0, nullptr, &ctx) != RAILS_OK) {
        std::printf("no gfx950 device: %s\n", rails_last_error());
        return 2;
    }
    rails::set_default_context(ctx);
    int failures = 0;
    rails_csr *bsr = nullptr, *csr = nullptr;
    if (rails_csr_create_bsr(ctx, mb, mb, b, brp.data(), bci.data(), bva.data(), &bsr) != RAILS_OK || rails_csr_create(ctx, m, m, rp.data(), ci.data(), va.data(), &csr) != RAILS_OK ||
        rails_csr_set_variant(csr, 3) != RAILS_OK) {
        std::printf("creating the operators: %s\nFAILED\n", rails_last_error());
        return 1;
    }
    if (rails_csr_block_size(bsr) != b || rails_csr_block_size(csr) != 1 || rails_csr_rows(bsr) != m || rails_csr_nnz(bsr) != (int64_t)bva.size()) {
        std::printf("block size %d / %d, rows %lld, nnz %lld\n", rails_csr_block_size(bsr), rails_csr_block_size(csr), (long long)rails_csr_rows(bsr), (long long)rails_csr_nnz(bsr));
        failures++;
    }
    {
        rails::HipMultiVectorWrapper B(m, p, ctx);
        rails_ctx_set_seed(ctx, 7, 0);
        B.random();
        ParameterList params;
        params.p = {{"Expand size", 2.0}, {"Lanczos iterations", 6.0}, {"Tolerance", 1e-8}};
        for (int backend = 0; backend < 2; ++backend) {
            const Outcome ob = solve(ctx, bsr, B, m, p, backend, params), oc = solve(ctx, csr, B, m, p, backend, params);
            const bool same = ob.ret == oc.ret && ob.trips == oc.trips && ob.k == oc.k && ob.V.size() == oc.V.size() &&
                              std::memcmp(ob.V.data(), oc.V.data(), ob.V.size() * sizeof(double)) == 0 && std::memcmp(ob.T.data(), oc.T.data(), ob.T.size() * sizeof(double)) == 0;
            std::printf("%s back end: block-CSR returned %d after %d trips with %d vectors (%s), CSR row-gather %d after %d with %d (%s): %s\n", backend ? "coordinate-space" : "direct",
                        ob.ret, ob.trips, ob.k, rails_csr_last_kernel(bsr), oc.ret, oc.trips, oc.k, rails_csr_last_kernel(csr), same ? "the same bits" : "DIFFERENT");
            if (ob.ret != 0 || !same || std::string(rails_csr_last_kernel(bsr)).find("k_spmm_bsr") != 0) failures++;
        }
        int64_t info[10] = {};
        if (rails_csr_bsr_stats(bsr, info, 10) != RAILS_OK || info[0] != (int64_t)bci.size() || info[1] != b || info[4] != b) failures++;
        std::printf("%lld blocks of %lld x %lld, longest block row %lld, %lld bytes on the device; last launch k_spmm_bsr<%lld, %lld>\n", (long long)info[0], (long long)info[1],
                    (long long)info[1], (long long)info[2], (long long)info[3], (long long)info[4], (long long)info[5]);
    }
    rails_csr_destroy(bsr);
    rails_csr_destroy(csr);
    rails_ctx_destroy(ctx);
    std::printf(failures ? "FAILED\n" : "OK\n");
    return failures ? 1 : 0;
}
