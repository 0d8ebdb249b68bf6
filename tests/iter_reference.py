"""A numpy restatement of the iterative A^-1 operator (rails_amd/csrc/itsolve.hip, iter_scalars.h): conjugate gradients and
right-preconditioned BiCGStab with per-column scalars, the freeze, the Jacobi preconditioner and the breakdown rules, and the test problems
the GPU tests share.  Not a test module: tests/test_iter_reference_host.py checks it against scipy's splu and pins the iteration counts
the GPU tests depend on; tests/test_gpu_iter.py compares the device against it."""
import numpy as np
import scipy.sparse as sp

ACTIVE, CONVERGED, MAXIT, BREAKDOWN, NONFINITE, PENDING = 1, 2, 4, 8, 16, 32


class Columns:
    """the scalar block: one entry per column (rails_iter_col)"""

    def __init__(self, bb, rho0, maxit):
        n = bb.size
        self.rho = rho0.astype(float).copy()
        self.alpha, self.beta, self.omega = np.zeros(n), np.zeros(n), np.zeros(n)
        self.bb, self.rr = bb.astype(float).copy(), bb.astype(float).copy()
        self.iter = np.zeros(n, dtype=np.int64)
        self.flags = np.full(n, ACTIVE, dtype=np.int64)
        for j in range(n):
            if not (np.isfinite(bb[j]) and np.isfinite(rho0[j])):
                self.freeze(j, NONFINITE)
            elif bb[j] == 0.0:
                self.freeze(j, CONVERGED)
            elif maxit <= 0:
                self.freeze(j, MAXIT)
            elif rho0[j] == 0.0:
                self.freeze(j, BREAKDOWN)

    def freeze(self, j, flag):
        self.flags[j] = (self.flags[j] & ~(ACTIVE | PENDING)) | flag
        self.alpha[j] = self.beta[j] = self.omega[j] = 0.0

    def active(self, j):
        if self.flags[j] & ACTIVE:
            return True
        self.alpha[j] = self.beta[j] = self.omega[j] = 0.0
        return False

    def any_active(self):
        return bool(np.any(self.flags & ACTIVE))

    def relres(self):
        with np.errstate(all="ignore"):
            return np.where(self.bb > 0, np.sqrt(self.rr / np.where(self.bb > 0, self.bb, 1.0)), 0.0)


def _sel(a, x, y):
    """y + a x where a != 0, y itself where a == 0 (axpy_sel of itsolve.hip)"""
    with np.errstate(all="ignore"):
        return np.where(a[None, :] != 0.0, y + a[None, :] * x, y)


def _diag_info(A, jacobi):
    d = np.asarray(A.diagonal(), dtype=float)
    have = bool(np.all(d != 0.0))
    dinv = 1.0 / d if (jacobi and have) else None
    sign = 1.0 if dinv is not None else (-1.0 if (have and np.all(d < 0)) else 1.0)
    return dinv, sign


def cg(A, Bm, tol=1e-10, maxit=1000, jacobi=True, stop_after=None):
    """returns X, Columns.  stop_after: iterations queued in all (the host's loop), None: until no column is active"""
    A = sp.csr_matrix(A)
    Bm = np.asarray(Bm, dtype=float).reshape(A.shape[0], -1)
    dinv, sign = _diag_info(A, jacobi)
    prec = (lambda R: R * dinv[:, None]) if dinv is not None else (lambda R: R)
    tol2 = tol * tol
    R = Bm.copy()
    Z = prec(R)
    P = Z.copy()
    X = np.zeros_like(R)
    with np.errstate(all="ignore"):
        c = Columns((R * R).sum(0), (R * Z).sum(0), maxit)
    n = R.shape[1]
    done = 0
    while c.any_active() and done < maxit and (stop_after is None or done < stop_after):
        with np.errstate(all="ignore"):
            Q = A @ P
            pq = (P * Q).sum(0)
        for j in range(n):
            if not c.active(j):
                continue
            if not np.isfinite(pq[j]):
                c.iter[j] += 1
                c.freeze(j, NONFINITE)
            elif pq[j] == 0.0 or ((pq[j] > 0.0) != (sign * c.rho[j] > 0.0)):
                c.iter[j] += 1
                c.freeze(j, BREAKDOWN)
            else:
                c.alpha[j] = c.rho[j] / pq[j]
        X = _sel(c.alpha, P, X)
        R = _sel(-c.alpha, Q, R)
        Z = prec(R)
        with np.errstate(all="ignore"):
            rz, rr = (R * Z).sum(0), (R * R).sum(0)
        for j in range(n):
            if not c.active(j):
                continue
            c.iter[j] += 1
            c.rr[j] = rr[j]
            if not (np.isfinite(rr[j]) and np.isfinite(rz[j])):
                c.freeze(j, NONFINITE)
            elif rr[j] <= tol2 * c.bb[j]:
                c.freeze(j, CONVERGED)
            elif c.iter[j] >= maxit:
                c.freeze(j, MAXIT)
            elif rz[j] == 0.0:
                c.freeze(j, BREAKDOWN)
            else:
                c.beta[j] = rz[j] / c.rho[j]
                c.rho[j] = rz[j]
        P = _sel(c.beta, P, Z)
        done += 1
    return X, c


def bicgstab(A, Bm, tol=1e-10, maxit=1000, jacobi=True, trans=False, stop_after=None):
    A = sp.csr_matrix(A)
    Bm = np.asarray(Bm, dtype=float).reshape(A.shape[0], -1)
    dinv, _ = _diag_info(A, jacobi)
    if trans:
        A = sp.csr_matrix(A.T)
    prec = (lambda R: R * dinv[:, None]) if dinv is not None else (lambda R: R)
    tol2 = tol * tol
    R = Bm.copy()
    RH = R.copy()
    X, P, V = np.zeros_like(R), np.zeros_like(R), np.zeros_like(R)
    with np.errstate(all="ignore"):
        bb = (R * R).sum(0)
    c = Columns(bb, bb, maxit)
    n = R.shape[1]
    done = 0
    while c.any_active() and done < maxit and (stop_after is None or done < stop_after):
        P = _sel(c.beta, _sel(-c.omega, V, P), R)
        PH = prec(P)
        with np.errstate(all="ignore"):
            V = A @ PH
            rhv = (RH * V).sum(0)
        for j in range(n):
            if not c.active(j):
                continue
            if not np.isfinite(rhv[j]):
                c.iter[j] += 1
                c.freeze(j, NONFINITE)
            elif rhv[j] == 0.0:
                c.iter[j] += 1
                c.freeze(j, BREAKDOWN)
            else:
                c.alpha[j] = c.rho[j] / rhv[j]
        S = _sel(-c.alpha, V, R)
        SH = prec(S)
        with np.errstate(all="ignore"):
            T = A @ SH
            ts, tt = (T * S).sum(0), (T * T).sum(0)
        for j in range(n):
            if not c.active(j):
                continue
            if not (np.isfinite(ts[j]) and np.isfinite(tt[j])):
                c.iter[j] += 1
                c.freeze(j, NONFINITE)
            elif tt[j] == 0.0:
                c.omega[j] = 0.0
                c.flags[j] |= PENDING
            else:
                c.omega[j] = ts[j] / tt[j]
        X = _sel(c.omega, SH, _sel(c.alpha, PH, X))
        R = _sel(-c.omega, T, S)
        with np.errstate(all="ignore"):
            rhr, rr = (RH * R).sum(0), (R * R).sum(0)
        for j in range(n):
            if not c.active(j):
                continue
            c.iter[j] += 1
            c.rr[j] = rr[j]
            if not (np.isfinite(rr[j]) and np.isfinite(rhr[j])):
                c.freeze(j, NONFINITE)
            elif rr[j] <= tol2 * c.bb[j]:
                c.freeze(j, CONVERGED)
            elif c.flags[j] & PENDING:
                c.freeze(j, BREAKDOWN)
            elif c.iter[j] >= maxit:
                c.freeze(j, MAXIT)
            elif rhr[j] == 0.0 or c.omega[j] == 0.0:
                c.freeze(j, BREAKDOWN)
            else:
                c.beta[j] = (rhr[j] / c.rho[j]) * (c.alpha[j] / c.omega[j])
                c.rho[j] = rhr[j]
        done += 1
    return X, c


def solve(method, A, Bm, **kw):
    return (cg if method == "cg" else bicgstab)(A, Bm, **kw)


# ---- the problems ---------------------------------------------------------------------------------------------------------------------

def convection_diffusion(nx, ny, cx=0.7, cy=0.4):
    """5-point convection-diffusion on an nx x ny grid, central differences: -4 on the diagonal, 1 -+ cx along x, 1 -+ cy along y.
    Nonsymmetric, diagonally dominant for |cx|, |cy| < 1."""
    ex, ey = np.ones(nx), np.ones(ny)
    Tx = sp.diags([(1 + cx) * ex[:-1], -2 * ex, (1 - cx) * ex[:-1]], [-1, 0, 1])
    Ty = sp.diags([(1 + cy) * ey[:-1], -2 * ey, (1 - cy) * ey[:-1]], [-1, 0, 1])
    return (sp.kron(sp.eye(ny), Tx) + sp.kron(Ty, sp.eye(nx))).tocsr()


def scaled(A, seed):
    """S A S with S^2 = 10^U(-1.5, 1.5): the diagonal spread over three decades"""
    s = np.sqrt(10.0 ** np.random.default_rng(seed).uniform(-1.5, 1.5, A.shape[0]))
    S = sp.diags(s)
    return (S @ A @ S).tocsr()


def problem(tag):
    """(matrix, method) of the issue's problems (a) .. (e)"""
    import generalized_problems as G
    from rails_amd import problems as P

    def from_triple(t):
        rowptr, col, val = t
        n = rowptr.size - 1
        return sp.csr_matrix((val, col, rowptr), shape=(n, n))

    if tag == "a":
        return G.laplacian2(1024), "cg"
    if tag == "b":
        return scaled(G.laplacian2(1024), 21), "cg"
    if tag == "c":
        return convection_diffusion(37, 29), "bicgstab"
    if tag == "c4":
        return convection_diffusion(65, 63), "bicgstab"
    if tag == "c'":
        return scaled(convection_diffusion(37, 29), 22), "bicgstab"
    if tag == "d":
        return from_triple(P.laplace7(13, 11, 10)), "cg"
    if tag == "e":
        return from_triple(P.stencil27(12, 11, 10, random_values=True, seed=3)), "bicgstab"
    raise KeyError(tag)


def rhs(n, nc, seed=5):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (n, nc))


_cache = {}


def reference(tag, nc, jacobi=True, trans=False, tol=1e-10, seed=5):
    """the restatement's solve of problem `tag` with the shared right-hand side of nc columns, computed once: (A, B, X, Columns)"""
    key = (tag, nc, jacobi, trans, tol, seed)
    if key not in _cache:
        A, method = problem(tag)
        Bm = rhs(A.shape[0], nc, seed)
        kw = {"trans": trans} if method == "bicgstab" else {}
        X, c = solve(method, A, Bm, tol=tol, maxit=5000, jacobi=jacobi, **kw)
        X.setflags(write=False)
        _cache[key] = (A, Bm, X, c)
    return _cache[key]


def true_relres(A, X, Bm, trans=False):
    A = sp.csr_matrix(A)
    Aop = A.T if trans else A
    return np.linalg.norm(Aop @ X - Bm, axis=0) / np.linalg.norm(Bm, axis=0)
