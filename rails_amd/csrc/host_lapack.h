// host_lapack.h -- the host LAPACK/BLAS this library resolves at run time (host_lapack.cpp: dlopen; the GPU box carries no system LAPACK,
// the image ships scipy's OpenBLAS and MKL), as a table of function pointers, and the few helpers more than one caller uses.  The helpers
// are inline so that each exists once and every translation unit compiles the same arithmetic.  Internal: the C ABI is include/rails_hip.h.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <string>
#include <vector>

extern "C" {
typedef int (*lp_select2)(const double *, const double *);
typedef void (*lp_dsyev)(const char *, const char *, const int *, double *, const int *, double *, double *, const int *, int *);
typedef void (*lp_dsyevd)(const char *, const char *, const int *, double *, const int *, double *, double *, const int *, int *, const int *, int *);
typedef void (*lp_dsteqr)(const char *, const int *, double *, double *, double *, const int *, double *, int *);
typedef void (*lp_dgees)(const char *, const char *, lp_select2, const int *, double *, const int *, int *, double *, double *,
                         double *, const int *, double *, const int *, int *, int *);
typedef void (*lp_dtrsyl)(const char *, const char *, const int *, const int *, const int *, const double *, const int *,
                          const double *, const int *, double *, const int *, double *, int *);
typedef void (*lp_dtrsyl3)(const char *, const char *, const int *, const int *, const int *, const double *, const int *,
                           const double *, const int *, double *, const int *, double *, int *, const int *, double *, const int *, int *);
typedef void (*lp_dpotrf)(const char *, const int *, double *, const int *, int *);
typedef void (*lp_dgeqp3)(const int *, const int *, double *, const int *, int *, double *, double *, const int *, int *);
typedef void (*lp_dorgqr)(const int *, const int *, const int *, double *, const int *, const double *, double *, const int *, int *);
typedef void (*lp_dpstrf)(const char *, const int *, double *, const int *, int *, int *, const double *, double *, int *);
typedef void (*lp_dgemm)(const char *, const char *, const int *, const int *, const int *, const double *, const double *,
                         const int *, const double *, const int *, const double *, double *, const int *);
typedef void (*lp_dtrsm)(const char *, const char *, const char *, const char *, const int *, const int *, const double *, const double *,
                         const int *, double *, const int *);
typedef void (*lp_dsyrk)(const char *, const char *, const int *, const int *, const double *, const double *, const int *, const double *,
                         double *, const int *);
typedef void (*lp_dgetrf)(const int *, const int *, double *, const int *, int *, int *);
typedef void (*lp_dgetrs)(const char *, const int *, const int *, const double *, const int *, const int *, double *, const int *, int *);
typedef void (*lp_dlaswp)(const int *, double *, const int *, const int *, const int *, const int *, const int *);
typedef void (*lp_dgetri)(const int *, double *, const int *, const int *, double *, const int *, int *);
}

struct HostLapack {
    void *handle = nullptr;
    std::string path;
    lp_dsyev dsyev = nullptr;
    lp_dsyevd dsyevd = nullptr; // optional
    lp_dsteqr dsteqr = nullptr;
    lp_dgees dgees = nullptr;
    lp_dtrsyl dtrsyl = nullptr;
    lp_dtrsyl3 dtrsyl3 = nullptr; // optional: blocked (level-3) triangular Sylvester solver of LAPACK >= 3.11
    lp_dpotrf dpotrf = nullptr;
    lp_dpstrf dpstrf = nullptr; // optional
    lp_dgeqp3 dgeqp3 = nullptr; // optional (rails_range_basis)
    lp_dorgqr dorgqr = nullptr;
    lp_dgemm dgemm = nullptr;
    lp_dtrsm dtrsm = nullptr; // optional: the generalized projected solve falls back to loops
    lp_dsyrk dsyrk = nullptr;   // optional: X = Z Z' of the factored ADI route
    lp_dgetrf dgetrf = nullptr; // optional: the squared-Smith fast path of rails_sb03md
    lp_dgetrs dgetrs = nullptr;
    lp_dlaswp dlaswp = nullptr; // optional: the bordered LU update of the factored ADI route
    lp_dgetri dgetri = nullptr; // optional: explicit (M - p I)^-1 of the factored ADI route
};

// The table: filled by rails_host_lapack_init, which every caller runs (and checks) before it reads an entry.
const HostLapack &host_lapack();

// C (m x n) = op(A) op(B)
inline void gemm(char ta, char tb, int m, int n, int k, const double *A, int lda, const double *B, int ldb, double *C, int ldc)
{
    const double one = 1.0, zero = 0.0;
    host_lapack().dgemm(&ta, &tb, &m, &n, &k, &one, A, &lda, B, &ldb, &zero, C, &ldc);
}

// LAPACK's eigen-solvers may not return (or may index out of bounds) on NaN / Inf input: refuse it with an error code instead.
inline bool all_finite(int rows, int cols, const double *a, int lda)
{
    for (int j = 0; j < cols; ++j)
        for (int i = 0; i < rows; ++i)
            if (!std::isfinite(a[i + (size_t)j * lda])) return false;
    return true;
}

// Eigenvalues (and, jobz 'V', vectors) of a symmetric matrix: divide and conquer where the library has it, vectors are asked for and
// n >= dc_from (2-3x faster at the restart sizes: eig(T), k = 200), the QR form otherwise; each with its workspace query.
inline void sym_eig(char jobz, char uplo, int n, double *a, int lda, double *w, int dc_from, int *info)
{
    const HostLapack &lp = host_lapack();
    if (lp.dsyevd && n >= dc_from && (jobz == 'V' || jobz == 'v')) {
        int lwork = -1, liwork = -1, iq = 0;
        double wq = 0.0;
        lp.dsyevd(&jobz, &uplo, &n, a, &lda, w, &wq, &lwork, &iq, &liwork, info);
        if (*info == 0) {
            lwork = (int)wq + 1;
            liwork = iq + 1;
            std::vector<double> work((size_t)lwork);
            std::vector<int> iwork((size_t)liwork);
            lp.dsyevd(&jobz, &uplo, &n, a, &lda, w, work.data(), &lwork, iwork.data(), &liwork, info);
            return;
        }
    }
    int lwork = -1;
    double wq = 0.0;
    lp.dsyev(&jobz, &uplo, &n, a, &lda, w, &wq, &lwork, info); // workspace query, as the reference does
    if (*info) return;
    lwork = (int)wq;
    std::vector<double> work((size_t)std::max(1, lwork));
    lp.dsyev(&jobz, &uplo, &n, a, &lda, w, work.data(), &lwork, info);
}

// A switch of the environment (RAILS_SB03MD_*): unset = dflt, set = its integer value is not 0.  The callers keep what they read in a
// static: once per process.
inline bool env_flag(const char *name, bool dflt)
{
    const char *e = getenv(name);
    return e ? atoi(e) != 0 : dflt;
}
