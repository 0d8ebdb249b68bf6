"""A numpy restatement of the Chebyshev polynomial preconditioner of the iterative A^-1 operator (rails_amd/csrc/cheb_coef.h, itsolve.hip:
k_cheb_init, k_cheb_step_csr, k_cheb_pass) and of conjugate gradients preconditioned with it: the coefficients, the Gershgorin bound, the
application z = p_K(G A) G r in float64 and in longdouble, the solve with per-column scalars (the rules of tests/iter_reference.py), the
problems the GPU tests share and the table the default of "poly_ratio" was chosen from.  Not a test module:
tests/test_cheb_reference_host.py checks it against scipy's splu and pins the iteration counts; tests/test_gpu_iter_poly.py compares the
device against it."""
import numpy as np
import scipy.sparse as sp

import iter_reference as R


def laplace2d(nx, ny):
    """5-point Laplacian on an nx x ny grid (x fastest), -4 on the diagonal: negative definite"""
    ex, ey = np.ones(nx), np.ones(ny)
    Tx = sp.diags([ex[:-1], -2 * ex, ex[:-1]], [-1, 0, 1])
    Ty = sp.diags([ey[:-1], -2 * ey, ey[:-1]], [-1, 0, 1])
    A = (sp.kron(sp.eye(ny), Tx) + sp.kron(Ty, sp.eye(nx))).tocsr()
    A.sort_indices()
    return A


def banded41(n=130, half=20):
    """symmetric, positive definite, exactly 2 half + 1 = 41 entries in every row (the band wraps around): a block of 64 rows has 2624
    nonzeros, more than the 2048 the fused kernel stages in LDS"""
    i = np.repeat(np.arange(n), 2 * half + 1)
    k = np.tile(np.arange(-half, half + 1), n)
    j = (i + k) % n
    v = (1.0 + 0.5 * np.cos(i + j + 0.25 * (i * j % 7))) / (1.0 + np.abs(k))  # symmetric in (i, j)
    v[k == 0] = 0.0
    A = sp.csr_matrix((v, (i, j)), shape=(n, n))
    A = A + sp.diags(np.asarray(abs(A).sum(1)).ravel() + 1.0)
    A = sp.csr_matrix(A)
    A.sort_indices()
    assert (A != A.T).nnz == 0 and np.all(np.diff(A.indptr) == 2 * half + 1)
    return A


def problem(tag):
    if tag == "lap9x8":
        return laplace2d(9, 8)
    if tag == "lap64":
        return laplace2d(64, 64)
    if tag == "lap128":
        return laplace2d(128, 128)
    if tag == "one":
        return sp.csr_matrix(np.array([[-3.0]]))
    if tag == "stencil27":
        from rails_amd import problems as P

        rowptr, col, val = P.stencil27(5, 4, 3)
        n = rowptr.size - 1
        return sp.csr_matrix((val, col, rowptr), shape=(n, n))
    if tag == "banded41":
        return banded41()
    if tag == "neg_banded41":
        return sp.csr_matrix(-banded41())
    raise KeyError(tag)


def g_of(A, jacobi):
    """G as a vector: the Jacobi diagonal's inverse, or the sign of the diagonal (the library's defsign: -1 when every diagonal entry is
    negative) times ones"""
    d = np.asarray(A.diagonal(), dtype=float)
    if jacobi:
        return 1.0 / d
    return np.full(d.size, -1.0 if np.all(d < 0) else 1.0)


def gershgorin(A, g=None):
    """max_i |g_i| sum_j |a_ij| (rails_cheb_gershgorin)"""
    s = np.asarray(abs(sp.csr_matrix(A)).sum(1)).ravel()
    return float((s * (np.abs(g) if g is not None else 1.0)).max())


def coefficients(lo, hi, K, dtype=np.float64):
    """theta, a[0 .. K), b[0 .. K) (rails_cheb_coef)"""
    lo, hi, two = dtype(lo), dtype(hi), dtype(2)
    theta, delta = (hi + lo) / two, (hi - lo) / two
    sigma = theta / delta
    rho = dtype(1) / sigma
    a, b = [], []
    for _ in range(K):
        nxt = dtype(1) / (two * sigma - rho)
        a.append(nxt * rho)
        b.append(two * nxt / delta)
        rho = nxt
    return theta, a, b


def _matmul(A, Z):
    """A Z in the precision of Z (scipy multiplies in float64 only): row sums of a_ij z_j in the order of the stored entries"""
    if Z.dtype == np.float64:
        return A @ Z
    assert np.all(np.diff(A.indptr) > 0)
    return np.add.reduceat(A.data.astype(Z.dtype)[:, None] * Z[A.indices], A.indptr[:-1], axis=0)


def polynomial(A, Rm, K, hi, ratio, g, dtype=np.float64):
    """z = p_K(G A) G r: d = z = (g r) / theta, then K times d = a d + b g (r - A z), z = z + d.  K = 0: G r."""
    A = sp.csr_matrix(A)
    Rm = np.asarray(Rm).astype(dtype).reshape(A.shape[0], -1)
    gv = np.asarray(g).astype(dtype)[:, None]
    if K == 0:
        return gv * Rm
    theta, a, b = coefficients(np.float64(hi) / np.float64(ratio), hi, K, dtype)
    D = (gv * Rm) / theta
    Z = D.copy()
    for k in range(K):
        D = a[k] * D + b[k] * (gv * (Rm - _matmul(A, Z)))
        Z = Z + D
    return Z


def pcg(A, Bm, K, ratio=30.0, hi=None, tol=1e-10, maxit=1000, jacobi=True):
    """conjugate gradients with z = p_K(G A) G r, per-column scalars and the freeze as in iter_reference.cg; K = 0 is iter_reference.cg.
    Returns X, Columns."""
    if K == 0:
        return R.cg(A, Bm, tol=tol, maxit=maxit, jacobi=jacobi)
    A = sp.csr_matrix(A)
    Bm = np.asarray(Bm, dtype=float).reshape(A.shape[0], -1)
    g = g_of(A, jacobi)
    if hi is None:
        hi = gershgorin(A, g)
    prec = lambda Rm: polynomial(A, Rm, K, hi, ratio, g)
    tol2 = tol * tol
    Rm = Bm.copy()
    Z = prec(Rm)
    P = Z.copy()
    X = np.zeros_like(Rm)
    with np.errstate(all="ignore"):
        c = R.Columns((Rm * Rm).sum(0), (Rm * Z).sum(0), maxit)
    n = Rm.shape[1]
    done = 0
    while c.any_active() and done < maxit:
        with np.errstate(all="ignore"):
            Q = A @ P
            pq = (P * Q).sum(0)
        for j in range(n):
            if not c.active(j):
                continue
            if not np.isfinite(pq[j]):
                c.iter[j] += 1
                c.freeze(j, R.NONFINITE)
            elif pq[j] == 0.0 or ((pq[j] > 0.0) != (c.rho[j] > 0.0)):  # r.z carries the operator's sign, as with Jacobi
                c.iter[j] += 1
                c.freeze(j, R.BREAKDOWN)
            else:
                c.alpha[j] = c.rho[j] / pq[j]
        X = R._sel(c.alpha, P, X)
        Rm = R._sel(-c.alpha, Q, Rm)
        with np.errstate(all="ignore"):
            Z = prec(Rm)
            rz, rr = (Rm * Z).sum(0), (Rm * Rm).sum(0)
        for j in range(n):
            if not c.active(j):
                continue
            c.iter[j] += 1
            c.rr[j] = rr[j]
            if not (np.isfinite(rr[j]) and np.isfinite(rz[j])):
                c.freeze(j, R.NONFINITE)
            elif rr[j] <= tol2 * c.bb[j]:
                c.freeze(j, R.CONVERGED)
            elif c.iter[j] >= maxit:
                c.freeze(j, R.MAXIT)
            elif rz[j] == 0.0:
                c.freeze(j, R.BREAKDOWN)
            else:
                c.beta[j] = rz[j] / c.rho[j]
                c.rho[j] = rz[j]
        P = R._sel(c.beta, P, Z)
        done += 1
    return X, c


def products(c, K):
    """products with A of a solve in the restatement's count: K + 1 per outer iteration of its slowest column"""
    return int(c.iter.max()) * (K + 1)


_cache = {}


def reference(tag, nc, K, ratio=30.0, jacobi=True, tol=1e-10, seed=5):
    """the restatement's solve of problem `tag` with iter_reference's shared right-hand side of nc columns, computed once: (A, B, X, Columns)"""
    key = (tag, nc, K, ratio, jacobi, tol, seed)
    if key not in _cache:
        A = problem(tag)
        Bm = R.rhs(A.shape[0], nc, seed)
        X, c = pcg(A, Bm, K, ratio=ratio, tol=tol, maxit=5000, jacobi=jacobi)
        X.setflags(write=False)
        _cache[key] = (A, Bm, X, c)
    return _cache[key]


def ratio_table(tags=("lap9x8", "lap64", "lap128"), degrees=(1, 2, 4, 8), ratios=(4, 10, 30, 100)):
    """products relative to plain CG (Jacobi, Gershgorin hi, two random columns, 1e-10): {(tag, K, ratio): (outer iterations, products,
    products / plain CG's)}, and per ratio the worst of the last -- what the default of "poly_ratio" was chosen by"""
    table, worst = {}, {r: 0.0 for r in ratios}
    for tag in tags:
        plain = products(reference(tag, 2, 0)[3], 0)
        table[(tag, 0, None)] = (plain, plain, 1.0)
        for K in degrees:
            for r in ratios:
                c = reference(tag, 2, K, ratio=float(r))[3]
                assert np.all(c.flags == R.CONVERGED)
                table[(tag, K, r)] = (int(c.iter.max()), products(c, K), products(c, K) / plain)
                worst[r] = max(worst[r], products(c, K) / plain)
    return table, worst
