// host_lapack.cpp -- the run-time LAPACK loader (dlopen: the GPU box carries no system LAPACK; this image ships scipy's OpenBLAS and
// MKL) and the dense pass-throughs of the C ABI, with the argument meaning of the reference's shims
//   rails_dsyev   <- LapackWrapper::DSYEV  (src/LapackWrapper.cpp:20-39)
//   rails_dsteqr  <- LapackWrapper::DSTEQR (src/LapackWrapper.cpp:12-18)
// The projected Lyapunov solve (rails_sb03md) is lyap_dense.cpp.
#include <dlfcn.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "host_lapack.h"
#include "rails_hip.h"

void rails_set_error(const char *fmt, ...);

namespace {

HostLapack g_lp;
std::mutex g_lp_mutex;

void *lookup(void *h, const char *base)
{
    static const char *prefixes[] = {"scipy_", "", nullptr};
    for (int i = 0; prefixes[i]; ++i) {
        std::string s = std::string(prefixes[i]) + base;
        if (void *p = dlsym(h, s.c_str())) return p;
    }
    return nullptr;
}

bool try_open(const std::string &path)
{
    if (path.empty()) return false;
    // OpenBLAS starts its worker threads when the library is loaded -- one per visible CPU (up to its build limit), each
    // spinning for a while before it goes to sleep.  On a box whose CPU quota (cgroup) is far below its CPU count those ~60
    // spinning threads use up the quota of a scheduling period in a few milliseconds and the WHOLE process is throttled for the
    // rest of it: one 40-90 ms trip some 100 ms after the first host LAPACK call of a solve (BENCH_r01: "slowest 42 ms").
    // openblas_set_num_threads() after the fact does not stop them, so the count is given through the environment for the
    // duration of the dlopen (and restored: other BLAS users of the process keep their own setting).
    // setenv is not safe against getenv in other threads of the process, so the window is kept as small as it can be: nothing is touched
    // when the library is in the process already (its threads exist: RTLD_NOLOAD probe), a variable the application has set itself is
    // left alone (its choice stands -- `OPENBLAS_NUM_THREADS=1 python bench.py` never gets here), and what is set is set once, under
    // g_lp_mutex, before the dlopen, and taken back right after.  An application with threads of its own that cannot tolerate even
    // that calls rails_host_lapack_init (or creates its first context) before it starts them, or exports the variable.
    int want_threads = 1;
    if (const char *e = getenv("RAILS_LAPACK_THREADS")) want_threads = atoi(e) > 0 ? atoi(e) : 1;
    void *h = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL | RTLD_NOLOAD);
    if (!h) {
        static const char *thread_vars[] = {"OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS", nullptr};
        bool mine[2] = {false, false};
        for (int i = 0; thread_vars[i]; ++i)
            if (!getenv(thread_vars[i])) {
                mine[i] = true;
                setenv(thread_vars[i], std::to_string(want_threads).c_str(), 1);
            }
        h = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
        for (int i = 0; thread_vars[i]; ++i)
            if (mine[i]) unsetenv(thread_vars[i]);
    }
    if (!h) return false;
    HostLapack L;
    L.handle = h;
    L.path = path;
    L.dsyev = (lp_dsyev)lookup(h, "dsyev_");
    L.dsyevd = (lp_dsyevd)lookup(h, "dsyevd_");
    L.dsteqr = (lp_dsteqr)lookup(h, "dsteqr_");
    L.dgees = (lp_dgees)lookup(h, "dgees_");
    L.dtrsyl = (lp_dtrsyl)lookup(h, "dtrsyl_");
    L.dtrsyl3 = (lp_dtrsyl3)lookup(h, "dtrsyl3_");
    L.dpotrf = (lp_dpotrf)lookup(h, "dpotrf_");
    L.dgemm = (lp_dgemm)lookup(h, "dgemm_");
    L.dtrsm = (lp_dtrsm)lookup(h, "dtrsm_");
    L.dsyrk = (lp_dsyrk)lookup(h, "dsyrk_");
    L.dgetrf = (lp_dgetrf)lookup(h, "dgetrf_");
    L.dgetrs = (lp_dgetrs)lookup(h, "dgetrs_");
    L.dlaswp = (lp_dlaswp)lookup(h, "dlaswp_");
    L.dgetri = (lp_dgetri)lookup(h, "dgetri_");
    L.dpstrf = (lp_dpstrf)lookup(h, "dpstrf_");
    L.dgeqp3 = (lp_dgeqp3)lookup(h, "dgeqp3_");
    L.dorgqr = (lp_dorgqr)lookup(h, "dorgqr_");
    if (!L.dsyev || !L.dsteqr || !L.dgees || !L.dtrsyl || !L.dpotrf || !L.dgemm) {
        dlclose(h);
        return false;
    }
    // The projected matrices are a few hundred rows: threaded BLAS only adds fork/join latency to the thousands of
    // small calls inside dgees/dtrsyl.  RAILS_LAPACK_THREADS overrides (default 1).
    typedef void (*setthreads_t)(int);
    setthreads_t st = (setthreads_t)dlsym(h, "scipy_openblas_set_num_threads");
    if (!st) st = (setthreads_t)dlsym(h, "openblas_set_num_threads");
    if (!st) st = (setthreads_t)dlsym(h, "MKL_Set_Num_Threads");
    int nt = 1;
    if (const char *e = getenv("RAILS_LAPACK_THREADS")) nt = atoi(e) > 0 ? atoi(e) : 1;
    if (st) st(nt);
    g_lp = L;
    return true;
}

} // namespace

const HostLapack &host_lapack() { return g_lp; }

extern "C" int rails_host_lapack_init(const char *path)
{
    std::lock_guard<std::mutex> lock(g_lp_mutex);
    if (g_lp.handle) return RAILS_OK;
    if (path && *path && try_open(path)) return RAILS_OK;
    if (const char *env = getenv("RAILS_LAPACK_LIB"))
        if (try_open(env)) return RAILS_OK;
    // scipy's bundled OpenBLAS (hashed file name): scan the usual site-packages locations
    static const char *dirs[] = {"/usr/local/lib/python3.10/dist-packages/scipy.libs", "/usr/lib/python3/dist-packages/scipy.libs",
                                 nullptr};
    for (int i = 0; dirs[i]; ++i) {
        std::string cmd = std::string("ls ") + dirs[i] + "/libscipy_openblas*.so 2>/dev/null";
        if (FILE *f = popen(cmd.c_str(), "r")) {
            char buf[1024];
            std::vector<std::string> found;
            while (fgets(buf, sizeof(buf), f)) {
                std::string s(buf);
                while (!s.empty() && (s.back() == '\n' || s.back() == ' ')) s.pop_back();
                found.push_back(s);
            }
            pclose(f);
            for (auto &s : found)
                if (try_open(s)) return RAILS_OK;
        }
    }
    static const char *cands[] = {"libopenblas.so.0", "libopenblas.so", "liblapack.so.3", "liblapack.so", "/opt/conda/lib/libmkl_rt.so",
                                  "libmkl_rt.so", nullptr};
    for (int i = 0; cands[i]; ++i)
        if (try_open(cands[i])) return RAILS_OK;
    rails_set_error("no host LAPACK found: set RAILS_LAPACK_LIB to a library exporting dsyev_/dgees_/dtrsyl_/dpotrf_/dgemm_");
    return RAILS_ELAPACK;
}

extern "C" const char *rails_host_lapack_path(void) { return g_lp.path.c_str(); }

extern "C" void rails_dsyev(char jobz, char uplo, int n, double *a, int lda, double *w, int *info)
{
    if (rails_host_lapack_init(nullptr) != RAILS_OK) {
        *info = -100;
        return;
    }
    if (n <= 0) {
        *info = 0;
        return;
    }
    if (!all_finite(n, n, a, lda)) {
        fprintf(stderr, "rails_dsyev: the matrix holds NaN or Inf entries\n");
        *info = n + 1;
        return;
    }
    sym_eig(jobz, uplo, n, a, lda, w, 64, info);
}

extern "C" void rails_dsteqr(char compz, int n, double *d, double *e, double *z, int ldz, double *work, int *info)
{
    if (rails_host_lapack_init(nullptr) != RAILS_OK) {
        *info = -100;
        return;
    }
    g_lp.dsteqr(&compz, &n, d, e, z, &ldz, work, info);
}

// B <- alpha * op(A)^-1 B (side 'L') or alpha * B op(A)^-1 (side 'R'), A triangular: BLAS DTRSM, or plain loops when the library has none
extern "C" void rails_dtrsm(char side, char uplo, char transa, char diag, int m, int n, double alpha, const double *A, int lda, double *B, int ldb)
{
    if (m <= 0 || n <= 0) return;
    const char *force_loops = getenv("RAILS_DTRSM_LOOPS"); // tests: exercise the fallback
    if (!(force_loops && atoi(force_loops) != 0) && rails_host_lapack_init(nullptr) == RAILS_OK && g_lp.dtrsm) {
        g_lp.dtrsm(&side, &uplo, &transa, &diag, &m, &n, &alpha, A, &lda, B, &ldb);
        return;
    }
    const bool left = side == 'L' || side == 'l', upper = uplo == 'U' || uplo == 'u', trans = !(transa == 'N' || transa == 'n'),
               unit = diag == 'U' || diag == 'u';
    const int na = left ? m : n;
    auto a = [&](int i, int j) { return trans ? A[j + (size_t)i * lda] : A[i + (size_t)j * lda]; }; // op(A)(i, j)
    const bool op_upper = upper != trans;
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < m; ++i) B[i + (size_t)j * ldb] *= alpha;
    if (left) { // solve op(A) X = B column by column
        for (int j = 0; j < n; ++j) {
            double *b = B + (size_t)j * ldb;
            if (op_upper)
                for (int i = na - 1; i >= 0; --i) {
                    double s = b[i];
                    for (int l = i + 1; l < na; ++l) s -= a(i, l) * b[l];
                    b[i] = unit ? s : s / a(i, i);
                }
            else
                for (int i = 0; i < na; ++i) {
                    double s = b[i];
                    for (int l = 0; l < i; ++l) s -= a(i, l) * b[l];
                    b[i] = unit ? s : s / a(i, i);
                }
        }
    } else { // solve X op(A) = B row by row
        for (int i = 0; i < m; ++i) {
            if (op_upper)
                for (int j = 0; j < na; ++j) {
                    double s = B[i + (size_t)j * ldb];
                    for (int l = 0; l < j; ++l) s -= B[i + (size_t)l * ldb] * a(l, j);
                    B[i + (size_t)j * ldb] = unit ? s : s / a(j, j);
                }
            else
                for (int j = na - 1; j >= 0; --j) {
                    double s = B[i + (size_t)j * ldb];
                    for (int l = j + 1; l < na; ++l) s -= B[i + (size_t)l * ldb] * a(l, j);
                    B[i + (size_t)j * ldb] = unit ? s : s / a(j, j);
                }
        }
    }
}

extern "C" void rails_dgemm(char ta, char tb, int m, int n, int k, double alpha, const double *A, int lda, const double *B, int ldb,
                            double beta, double *C, int ldc)
{
    if (rails_host_lapack_init(nullptr) != RAILS_OK) return;
    g_lp.dgemm(&ta, &tb, &m, &n, &k, &alpha, A, &lda, B, &ldb, &beta, C, &ldc);
}

extern "C" void rails_dpotrf(char uplo, int n, double *a, int lda, int *info)
{
    if (rails_host_lapack_init(nullptr) != RAILS_OK) {
        *info = -100;
        return;
    }
    g_lp.dpotrf(&uplo, &n, a, &lda, info);
}

// Cholesky with complete pivoting of a positive semi-definite matrix (LAPACK dpstrf): P' A P = R' R, stops at the first
// pivot <= tol and returns the rank found.  piv is 0-based here.  Falls back to an unblocked outer-product form when the
// host LAPACK does not export dpstrf.
extern "C" void rails_dpstrf(char uplo, int n, double *a, int lda, int *piv, int *rank, double tol, int *info)
{
    if (rails_host_lapack_init(nullptr) != RAILS_OK) {
        *info = -100;
        return;
    }
    if (g_lp.dpstrf) {
        std::vector<double> work((size_t)2 * (n > 0 ? n : 1));
        g_lp.dpstrf(&uplo, &n, a, &lda, piv, rank, &tol, work.data(), info);
        for (int i = 0; i < n; ++i) piv[i] -= 1;
        return;
    }
    // upper form: a(i, j), i <= j
    *info = 0;
    if (uplo != 'U' && uplo != 'u') {
        *info = -1;
        return;
    }
    for (int i = 0; i < n; ++i) piv[i] = i;
    int r = 0;
    for (; r < n; ++r) {
        int q = r;
        for (int j = r + 1; j < n; ++j)
            if (a[j + (size_t)j * lda] > a[q + (size_t)q * lda]) q = j;
        if (!(a[q + (size_t)q * lda] > tol)) break;
        if (q != r) { // symmetric swap of r and q in the upper triangle
            std::swap(piv[r], piv[q]);
            std::swap(a[r + (size_t)r * lda], a[q + (size_t)q * lda]);
            for (int i = 0; i < r; ++i) std::swap(a[i + (size_t)r * lda], a[i + (size_t)q * lda]);
            for (int j = q + 1; j < n; ++j) std::swap(a[r + (size_t)j * lda], a[q + (size_t)j * lda]);
            for (int i = r + 1; i < q; ++i) std::swap(a[r + (size_t)i * lda], a[i + (size_t)q * lda]);
        }
        double d = std::sqrt(a[r + (size_t)r * lda]);
        a[r + (size_t)r * lda] = d;
        for (int j = r + 1; j < n; ++j) a[r + (size_t)j * lda] /= d;
        for (int j = r + 1; j < n; ++j) {
            double f = a[r + (size_t)j * lda];
            for (int i = r + 1; i <= j; ++i) a[i + (size_t)j * lda] -= a[r + (size_t)i * lda] * f;
        }
    }
    *rank = r;
    *info = r < n ? 1 : 0;
}

// Orthonormal basis of the column space of A (m x n, column-major, overwritten): Householder QR with column pivoting (dgeqp3),
// numerical rank = pivots with |r_ii| > tol * |r_11|, Q (m x rank) formed with dorgqr into q (ldq >= m).  Used by the
// coordinate-space backend (rails/SubspaceWrappers.hpp) to compress its basis after a restart.
extern "C" void rails_range_basis(int m, int n, double *a, int lda, double tol, double *q, int ldq, int *rank, int *info)
{
    *rank = 0;
    if (rails_host_lapack_init(nullptr) != RAILS_OK || !g_lp.dgeqp3 || !g_lp.dorgqr) {
        *info = -100;
        return;
    }
    if (m <= 0 || n <= 0) {
        *info = 0;
        return;
    }
    const int kmin = m < n ? m : n;
    std::vector<int> jpvt((size_t)n, 0);
    std::vector<double> tau((size_t)kmin);
    double wq = 0.0;
    int lwork = -1;
    g_lp.dgeqp3(&m, &n, a, &lda, jpvt.data(), tau.data(), &wq, &lwork, info);
    if (*info != 0) return;
    lwork = (int)wq + 1;
    std::vector<double> work((size_t)lwork);
    g_lp.dgeqp3(&m, &n, a, &lda, jpvt.data(), tau.data(), work.data(), &lwork, info);
    if (*info != 0) return;
    const double r11 = std::fabs(a[0]);
    int r = 0;
    while (r < kmin && std::fabs(a[r + (size_t)r * lda]) > tol * r11 && r11 > 0.0) ++r;
    *rank = r;
    if (r == 0) return;
    // the reflectors live below the diagonal of a's first r columns: copy them to q and expand
    for (int j = 0; j < r; ++j)
        for (int i = 0; i < m; ++i) q[i + (size_t)j * ldq] = a[i + (size_t)j * lda];
    lwork = -1;
    g_lp.dorgqr(&m, &r, &r, q, &ldq, tau.data(), &wq, &lwork, info);
    if (*info != 0) return;
    lwork = (int)wq + 1;
    work.resize((size_t)lwork);
    g_lp.dorgqr(&m, &r, &r, q, &ldq, tau.data(), work.data(), &lwork, info);
}
