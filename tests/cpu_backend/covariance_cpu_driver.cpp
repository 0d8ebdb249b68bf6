// TEST SCAFFOLDING: the pair and map entries of rails::Solution (rails/Solution.hpp) on the plain CPU backend (CpuDense.hpp), which has no
// rowpair member and so runs the template's element-access fallback.  Reads U (m x k) and S (k x k) as row-major binary doubles and three
// int32 index files (ia, ib: n entries each; rows: q entries), writes the pairs, the covariance maps and the correlation maps
// (tests/test_covariance_host.py compares them with the longdouble reference).
//   covariance_cpu_driver U.bin S.bin m k ia.bin ib.bin n rows.bin q out_prefix
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "CpuDense.hpp"
#include "rails/Solution.hpp"

using cpu::CpuDense;

template <class T>
static std::vector<T> slurp(const char *path, size_t n)
{
    std::vector<T> buf(n);
    FILE *f = fopen(path, "rb");
    if (!f || fread(buf.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "cannot read %s\n", path);
        exit(2);
    }
    fclose(f);
    return buf;
}

static CpuDense load(const char *path, int m, int n)
{
    std::vector<double> buf = slurp<double>(path, (size_t)m * n);
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
    if (argc < 11) return 2;
    const int m = atoi(argv[3]), k = atoi(argv[4]), n = atoi(argv[7]), q = atoi(argv[9]);
    const std::string out = argv[10];
    static_assert(!rails::has_rowpair<CpuDense, CpuDense>::value, "the CPU backend is meant to take the element-access path");
    CpuDense U = load(argv[1], m, k), S = load(argv[2], k, k);
    std::vector<int32_t> ia = slurp<int32_t>(argv[5], n), ib = slurp<int32_t>(argv[6], n), rows = slurp<int32_t>(argv[8], q);
    rails::Solution<CpuDense, CpuDense> sol(U, S);
    store(out + ".pairs", sol.covariance(ia, ib));
    store(out + ".pairs_b", sol.covariance(std::vector<int32_t>(), ib)); // an empty vector is the identity
    store(out + ".maps", sol.maps(rows));
    store(out + ".corr", sol.maps(rows, true));
    return 0;
}
