// TEST SCAFFOLDING: rails::Solution (rails/Solution.hpp) on the plain CPU backend (CpuDense.hpp), which has no rowquad member and so runs
// the template's contract path for the variance.  Reads U (m x k), S (k x k), W (m x nc) as row-major binary files, writes trace,
// variance, X W and the eigenpairs (tests/test_solution_host.py compares them with dense algebra).
//   solution_cpu_driver U.bin S.bin W.bin m k nc want tol out_prefix
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "CpuDense.hpp"
#include "rails/Solution.hpp"

using cpu::CpuDense;

static CpuDense load(const char *path, int m, int n)
{
    std::vector<double> buf((size_t)m * n);
    FILE *f = fopen(path, "rb");
    if (!f || fread(buf.data(), sizeof(double), buf.size(), f) != buf.size()) {
        fprintf(stderr, "cannot read %s\n", path);
        exit(2);
    }
    fclose(f);
    CpuDense out(m, n);
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < n; ++j) out(i, j) = buf[(size_t)i * n + j];
    return out;
}

static void store(std::string const &path, CpuDense const &A)
{
    FILE *f = fopen(path.c_str(), "wb");
    for (int i = 0; i < A.M(); ++i)
        for (int j = 0; j < A.N(); ++j) {
            double v = A(i, j);
            fwrite(&v, sizeof(double), 1, f);
        }
    fclose(f);
}

int main(int argc, char **argv)
{
    if (argc < 10) return 2;
    const int m = atoi(argv[4]), k = atoi(argv[5]), nc = atoi(argv[6]), want = atoi(argv[7]);
    const double tol = atof(argv[8]);
    const std::string out = argv[9];
    static_assert(!rails::has_rowquad<CpuDense, CpuDense>::value, "the CPU backend is meant to take the contract path");
    CpuDense U = load(argv[1], m, k), S = load(argv[2], k, k), W = load(argv[3], m, nc);
    rails::Solution<CpuDense, CpuDense> sol(U, S);
    auto e = sol.eigs(want, tol);
    store(out + ".var", sol.variance());
    store(out + ".apply", sol.apply(W));
    store(out + ".values", e.values);
    store(out + ".vectors", e.vectors);
    FILE *f = fopen((out + ".txt").c_str(), "w");
    fprintf(f, "%d %d %.17g\n", sol.rank(), e.found, sol.trace());
    fclose(f);
    return 0;
}
