// TEST SCAFFOLDING: the solver template's nullspace deflation (Solver::set_nullspace) on the plain CPU backend, through the generic
// path of the MultiVector contract (CpuDense has no orthogonalize(N) member).
// usage: driver A.bin B.bin N.bin n p q seed out_prefix [name=value ...] [max_trips=k] [nrows=r]
// (dense column-major files; q = 0: no nullspace; nrows: rows of N, n by default).  Writes out.txt: the return code of set_parameters
// (nonzero: no solve) or of solve, trips, V.N(), the nullspace rank kept; then out.V and out.T.
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

int main(int argc, char **argv)
{
    if (argc < 9) return 2;
    const int n = atoi(argv[4]), p = atoi(argv[5]), q = atoi(argv[6]);
    cpu::rng().seed = strtoull(argv[7], nullptr, 10);
    cpu::rng().stream = 0;
    std::string prefix = argv[8];
    ParameterList params;
    int max_trips = 0, nrows = n;
    for (int i = 9; i < argc; ++i) {
        std::string s(argv[i]);
        size_t eq = s.find('=');
        std::string key = s.substr(0, eq), val = s.substr(eq + 1);
        if (key == "max_trips")
            max_trips = atoi(val.c_str());
        else if (key == "nrows")
            nrows = atoi(val.c_str());
        else
            params.p[key] = atof(val.c_str());
    }
    CpuDense A(n, n), B(n, p);
    read(argv[1], (double *)A, (size_t)n * n);
    read(argv[2], (double *)B, (size_t)n * p);
    rails::Solver<CpuDense, CpuDense, CpuDense> solver(A, B, A);
    solver.set_verbose(false);
    solver.set_max_trips(max_trips);
    if (q > 0) {
        CpuDense N(nrows, q);
        read(argv[3], (double *)N, (size_t)nrows * q);
        solver.set_nullspace(N);
    }
    int rc = solver.set_parameters(params);
    CpuDense V(n, 1), T;
    if (!rc) rc = solver.solve(V, T);
    FILE *f = fopen((prefix + ".txt").c_str(), "w");
    fprintf(f, "%d %d %d %d\n", rc, solver.trips(), V.N(), solver.nullspace_rank());
    fclose(f);
    const int k = V.N();
    f = fopen((prefix + ".V").c_str(), "wb");
    for (int j = 0; j < k; ++j) fwrite(&V(0, j), sizeof(double), n, f);
    fclose(f);
    remove((prefix + ".T").c_str());
    if (T.M() == k) {
        f = fopen((prefix + ".T").c_str(), "wb");
        for (int j = 0; j < k; ++j) fwrite(&T(0, j), sizeof(double), k, f);
        fclose(f);
    }
    return 0;
}
