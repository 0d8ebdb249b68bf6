// TEST SCAFFOLDING: the solver template's raw start space (Solver::set_raw_start_space, opts.space of the reference) on the plain CPU
// backend, through the generic path of the MultiVector contract (CpuDense has no orthogonalize_range member).
// usage: driver orth  W.bin N.bin m w q out_prefix
//            rails::orthogonalize_range on W (m x w) against N (m x q, orthonormal; q = 0: none).  Writes out.txt: the columns kept; out.V.
//        driver solve A.bin B.bin V0.bin n p k0 seed out_prefix [name=value ...] [max_trips=k]
//            a solve from the raw start space V0 (n x k0).  Writes out.txt: the return code of set_parameters (100 + code: no solve) or
//            of solve, trips, V.N(), start_rank(); then out.V and out.T.
// (dense column-major files)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "CpuDense.hpp"
#include "rails/LyapunovSolver.hpp"

using cpu::CpuDense;

struct ParameterList {
    std::map<std::string, double> p;
    template <typename T>
    T get(std::string const &name, T def)
    {
        auto it = p.find(name);
        return it == p.end() ? def : (T)it->second;
    }
};

static void read(const char *path, double *dst, size_t n)
{
    FILE *f = fopen(path, "rb");
    if (!f || fread(dst, sizeof(double), n, f) != n) {
        fprintf(stderr, "cannot read %s\n", path);
        exit(2);
    }
    fclose(f);
}

static void write_columns(std::string const &path, CpuDense const &X, int rows, int cols)
{
    FILE *f = fopen(path.c_str(), "wb");
    for (int j = 0; j < cols; ++j) fwrite(&X(0, j), sizeof(double), rows, f);
    fclose(f);
}

static int orth(int argc, char **argv)
{
    if (argc < 8) return 2;
    const int m = atoi(argv[4]), w = atoi(argv[5]), q = atoi(argv[6]);
    const std::string prefix = argv[7];
    CpuDense W(m, w), N(m, std::max(q, 1));
    read(argv[2], (double *)W, (size_t)m * w);
    if (q > 0) read(argv[3], (double *)N, (size_t)m * q);
    static_assert(!rails::has_range_orthogonalize<CpuDense>::value, "CpuDense is to take the generic path");
    const int kept = rails::orthogonalize_range(W, q > 0 ? &N : (CpuDense const *)nullptr, 1e-8, rails::has_range_orthogonalize<CpuDense>());
    FILE *f = fopen((prefix + ".txt").c_str(), "w");
    fprintf(f, "%d %d\n", kept, W.N());
    fclose(f);
    write_columns(prefix + ".V", W, m, W.N());
    return 0;
}

static int solve(int argc, char **argv)
{
    if (argc < 10) return 2;
    const int n = atoi(argv[5]), p = atoi(argv[6]), k0 = atoi(argv[7]);
    cpu::rng().seed = strtoull(argv[8], nullptr, 10);
    cpu::rng().stream = 0;
    const std::string prefix = argv[9];
    ParameterList params;
    int max_trips = 0;
    for (int i = 10; i < argc; ++i) {
        std::string s(argv[i]);
        size_t eq = s.find('=');
        std::string key = s.substr(0, eq), val = s.substr(eq + 1);
        if (key == "max_trips")
            max_trips = atoi(val.c_str());
        else
            params.p[key] = atof(val.c_str());
    }
    CpuDense A(n, n), B(n, p), V(n, k0), T;
    read(argv[2], (double *)A, (size_t)n * n);
    read(argv[3], (double *)B, (size_t)n * p);
    read(argv[4], (double *)V, (size_t)n * k0);
    rails::Solver<CpuDense, CpuDense, CpuDense> solver(A, B, A);
    solver.set_verbose(false);
    solver.set_max_trips(max_trips);
    solver.set_raw_start_space(true);
    const int prc = solver.set_parameters(params);
    const int rc = prc ? 100 + prc : solver.solve(V, T);
    FILE *f = fopen((prefix + ".txt").c_str(), "w");
    fprintf(f, "%d %d %d %d\n", rc, solver.trips(), V.N(), solver.start_rank());
    fclose(f);
    write_columns(prefix + ".V", V, n, V.N());
    remove((prefix + ".T").c_str());
    if (T.M() == V.N() && T.M() > 0) write_columns(prefix + ".T", T, T.M(), T.M());
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "orth")) return orth(argc, argv);
    if (!strcmp(argv[1], "solve")) return solve(argc, argv);
    return 2;
}
