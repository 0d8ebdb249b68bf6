// TEST SCAFFOLDING: the solver template's projection methods ("Projection method", Solver::set_inverse) on the plain CPU backend.
// usage: driver A.bin Ainv.bin B.bin n p seed out_prefix [name=value ...] [inverse=0] [V0=file V0cols=k]
// (dense column-major files; Ainv is any n x n matrix the solver applies as A^-1).  Writes out.txt: the return code of
// set_parameters (nonzero: no solve) or of solve, trips, V.N(); then out.V and out.T.
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
    if (argc < 8) return 2;
    int n = atoi(argv[4]), p = atoi(argv[5]);
    cpu::rng().seed = strtoull(argv[6], nullptr, 10);
    cpu::rng().stream = 0;
    std::string prefix = argv[7];
    ParameterList params;
    int v0cols = 0, with_inverse = 1, max_trips = 0;
    std::string v0file;
    for (int i = 8; i < argc; ++i) {
        std::string s(argv[i]);
        size_t eq = s.find('=');
        std::string key = s.substr(0, eq), val = s.substr(eq + 1);
        if (key == "V0")
            v0file = val;
        else if (key == "V0cols")
            v0cols = atoi(val.c_str());
        else if (key == "inverse")
            with_inverse = atoi(val.c_str());
        else if (key == "max_trips")
            max_trips = atoi(val.c_str());
        else
            params.p[key] = atof(val.c_str());
    }
    CpuDense A(n, n), Ainv(n, n), B(n, p);
    read(argv[1], (double *)A, (size_t)n * n);
    read(argv[2], (double *)Ainv, (size_t)n * n);
    read(argv[3], (double *)B, (size_t)n * p);
    rails::Solver<CpuDense, CpuDense, CpuDense> solver(A, B, A);
    solver.set_verbose(false);
    solver.set_max_trips(max_trips);
    if (with_inverse) solver.set_inverse(Ainv);
    int rc = solver.set_parameters(params);
    CpuDense V(n, std::max(1, v0cols)), T;
    if (!rc) {
        if (v0cols > 0) {
            read(v0file.c_str(), (double *)V, (size_t)n * v0cols);
            V.orthogonalize();
        }
        rc = solver.solve(V, T);
    }
    FILE *f = fopen((prefix + ".txt").c_str(), "w");
    fprintf(f, "%d %d %d\n", rc, solver.trips(), V.N());
    fclose(f);
    const int k = V.N();
    f = fopen((prefix + ".V").c_str(), "wb");
    for (int j = 0; j < k; ++j) fwrite(&V(0, j), sizeof(double), n, f);
    fclose(f);
    if (T.M() == k) {
        f = fopen((prefix + ".T").c_str(), "wb");
        for (int j = 0; j < k; ++j) fwrite(&T(0, j), sizeof(double), k, f);
        fclose(f);
    }
    return 0;
}
