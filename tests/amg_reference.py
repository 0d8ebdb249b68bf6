"""A numpy/scipy restatement of the smoothed-aggregation multigrid preconditioner of the iterative A^-1 operator (rails_amd/csrc/amg_host.h
and amg_host.cpp for the set-up; itsolve.hip: Run::vcycle, iter_kernels.inc: k_amg_residual_csr, k_amg_coarse_dense, k_amg_prolong_add for the cycle),
written from the rules and not by calling the library: strength, the three aggregation passes, the smoothed prolongation, the Galerkin
product, the stop rules, the dense coarsest inverse; the V(1,1)-cycle with the Chebyshev smoother of tests/cheb_reference.py in float64
and in longdouble; conjugate gradients preconditioned with the cycle (the rules of tests/iter_reference.py).  Not a test module:
tests/test_amg_host.py compares the library's host set-up against it, tests/test_gpu_iter_amg.py the device."""
import numpy as np
import scipy.sparse as sp

import cheb_reference as C
import iter_reference as R

THETA, COARSE, RATIO, DEGREE = 0.08, 256, 4.0, 1
MAX_LEVELS, MAX_COARSE = 16, 1024
LD = np.longdouble


def laplace7(nx, ny, nz):
    """7-point Laplacian on an nx x ny x nz grid (x fastest), -6 on the diagonal: negative definite"""
    def t(n):
        e = np.ones(n)
        return sp.diags([e[:-1], -2 * e, e[:-1]], [-1, 0, 1])
    A = (sp.kron(sp.eye(nz), sp.kron(sp.eye(ny), t(nx))) + sp.kron(sp.eye(nz), sp.kron(t(ny), sp.eye(nx))) + sp.kron(t(nz), sp.eye(nx * ny))).tocsr()
    A.sort_indices()
    return A


def problem(tag):
    """(matrix, coarse) of the problems the host and GPU tests share.  With coarse 16 the small ones have levels: lap9x8 72 / 14 rows,
    the banded ones 130 / 65 / 2 with rows of P of 23 entries and second-level rows of 63; stencil27 (60 rows) stops at the rule that a
    level may keep at most 0.8 of its rows and is one dense block, as `one` is."""
    if tag == "lap24":
        return C.laplace2d(24, 24), 16
    if tag == "lap7_12":
        return laplace7(12, 12, 12), 64
    if tag in ("lap9x8", "banded41", "neg_banded41", "stencil27", "one"):
        return C.problem(tag), 16
    return C.problem(tag), COARSE


def aggregate(A, d, theta_l):
    """the three passes in row order; returns (aggregate of every row, number of aggregates)"""
    n = A.shape[0]
    Ap, Aj, Ax = A.indptr, A.indices, A.data
    absd = np.abs(d)
    rows = np.repeat(np.arange(n), np.diff(Ap))
    strong = (Aj != rows) & (np.abs(Ax) >= theta_l * np.sqrt(absd[rows] * absd[Aj]))
    agg = np.full(n, -1, dtype=np.int64)
    count = 0
    for i in range(n):  # (1) a free row whose strong neighbours are all free founds an aggregate with them
        if agg[i] >= 0:
            continue
        nb = Aj[Ap[i]:Ap[i + 1]][strong[Ap[i]:Ap[i + 1]]]
        if nb.size == 0 or np.any(agg[nb] >= 0):
            continue
        agg[i] = count
        agg[nb] = count
        count += 1
    after1 = agg.copy()
    for i in range(n):  # (2) join the strongest aggregated strong neighbour, against the state after pass 1; ties: the lower column
        if after1[i] >= 0:
            continue
        sl = slice(Ap[i], Ap[i + 1])
        ok = strong[sl] & (after1[Aj[sl]] >= 0)
        if np.any(ok):
            w = np.where(ok, np.abs(Ax[sl]), -1.0)
            agg[i] = after1[Aj[sl][int(np.argmax(w))]]  # argmax: the first of equals
    for i in range(n):  # (3) what is left founds aggregates with its free strong neighbours
        if agg[i] >= 0:
            continue
        agg[i] = count
        nb = Aj[Ap[i]:Ap[i + 1]][strong[Ap[i]:Ap[i + 1]]]
        agg[nb[agg[nb] < 0]] = count
        count += 1
    return agg, count


def _terms(A, B):
    """every term a_ik b_kj of A B in Gustavson's order: indices into the entries of A and of B, and the structural pattern (sorted by
    row, then column) with, per term, the entry of the pattern it belongs to"""
    Ap, Aj, Bp, Bj = A.indptr.astype(np.int64), A.indices.astype(np.int64), B.indptr.astype(np.int64), B.indices.astype(np.int64)
    lens = (Bp[1:] - Bp[:-1])[Aj]
    ia = np.repeat(np.arange(Aj.size), lens)
    ib = np.repeat(Bp[Aj], lens) + (np.arange(lens.sum()) - np.repeat(np.cumsum(lens) - lens, lens))
    rows = np.repeat(np.arange(A.shape[0]), np.diff(Ap))[ia]
    key = rows * B.shape[1] + Bj[ib]
    uniq, inv = np.unique(key, return_inverse=True)
    return ia, ib, uniq // B.shape[1], uniq % B.shape[1], inv


def product(A, B, Ad=None, Bd=None):
    """A B with every structural entry kept and sorted columns.  float64: scipy's row-wise product (the sums in Gustavson's order, as
    amg_host.cpp's), its entries put into the structural pattern; with longdouble values Ad, Bd on the patterns of A and B: longdouble
    sums.  Returns the csr matrix (float64) and, in longdouble, the values on its pattern."""
    A, B = sp.csr_matrix(A), sp.csr_matrix(B)
    ia, ib, pr, pc, inv = _terms(A, B)
    shape = (A.shape[0], B.shape[1])
    Cs = sp.csr_matrix(A @ B)
    Cs.sort_indices()
    Cs = Cs.tocoo()
    data = np.zeros(pr.size)
    pos = np.searchsorted(pr * shape[1] + pc, Cs.row.astype(np.int64) * shape[1] + Cs.col)
    data[pos] = Cs.data
    Cm = sp.csr_matrix((data, (pr, pc)), shape=shape)  # (coo -> csr keeps explicit zeros)
    Cm.sort_indices()
    assert Cm.nnz == pr.size
    if Ad is None:
        return Cm, None
    vals = np.zeros(pr.size, dtype=LD)
    np.add.at(vals, inv, Ad[ia] * Bd[ib])
    return Cm, vals


def _gershgorin(A, data, dinv):
    s = np.zeros(A.shape[0], dtype=data.dtype)
    np.add.at(s, np.repeat(np.arange(A.shape[0]), np.diff(A.indptr)), np.abs(data))
    return (s * np.abs(dinv)).max()


def _refined_inverse(M, X):
    """the inverse of M in longdouble from a float64 start by Newton's iteration X <- X (2 I - M X)"""
    M, X = M.astype(LD), X.astype(LD)
    for _ in range(3):
        X = X @ (2 * np.eye(M.shape[0], dtype=LD) - M @ X)
    return X


def setup(A, theta=THETA, coarse=COARSE, longdouble=False):
    """the hierarchy: {"levels": [{"A", "P", "R", "dinv", "hi", "agg"}], "coarse": A_L, "Ainv", "Ainv_ld", "defsign"}.  Ainv_ld is the
    longdouble inverse of the float64 A_L (what an exact coarse solve of this hierarchy is).  longdouble=True: the same set-up with the
    same aggregates evaluated in longdouble beside it -- "A_ld", "P_ld" of every level and "coarse_ld", "Ainv_exact" hold the values on
    the same patterns -- the yardstick for the float64 values' own error.  ValueError where the library refuses."""
    A = sp.csr_matrix(A).astype(float)
    A.sort_indices()
    if not (0.0 <= theta < 1.0) or not (1 <= coarse <= MAX_COARSE):
        raise ValueError("theta or coarse out of range")
    cur, cur_ld = A, A.data.astype(LD)
    levels = []
    d0 = A.diagonal()
    if np.any(d0 == 0) or not (np.all(d0 < 0) or np.all(d0 > 0)):
        raise ValueError("not definite")
    defsign = -1.0 if d0[0] < 0 else 1.0
    while True:
        n = cur.shape[0]
        d = cur.diagonal()
        if np.any(d == 0) or not np.all(np.isfinite(d)) or np.any(np.sign(d) != defsign):
            raise ValueError("not definite")
        dinv = 1.0 / d
        if n <= coarse or len(levels) + 1 >= MAX_LEVELS:
            break
        agg, n_agg = aggregate(cur, d, theta * 0.5 ** len(levels))
        if n_agg * 5 > n * 4:
            break
        rows = np.repeat(np.arange(n), np.diff(cur.indptr))
        hi = float(_gershgorin(cur, cur.data, dinv))
        T = sp.csr_matrix((np.ones(n), agg, np.arange(n + 1)), shape=(n, n_agg))
        if longdouble:
            dinv_ld = 1 / cur_ld[np.flatnonzero(cur.indices == rows)]
            hi_ld = _gershgorin(cur, cur_ld, dinv_ld)
        AT, AT_ld = product(cur, T, cur_ld if longdouble else None, T.data.astype(LD))
        prow = np.repeat(np.arange(n), np.diff(AT.indptr))
        own = AT.indices == agg[prow]
        P = AT.copy()
        P.data = np.where(own, 1.0, 0.0) - ((4.0 / (3.0 * hi)) * dinv)[prow] * AT.data
        Rm = sp.csr_matrix(P.T)  # (csr -> csc is the stable counting sort of rails_csr_transpose_host)
        RA, _ = product(Rm, cur)
        nxt, _ = product(RA, P)
        level = {"A": cur, "P": P, "R": Rm, "dinv": dinv, "hi": hi, "agg": agg}
        nxt_ld = None
        if longdouble:
            P_ld = np.where(own, LD(1), LD(0)) - ((LD(4) / (LD(3) * hi_ld)) * dinv_ld)[prow] * AT_ld
            # R's entries in P's: the transpose of the entry numbers
            perm = sp.csr_matrix((np.arange(1, P.nnz + 1), P.indices, P.indptr), shape=P.shape).T.tocsr().data - 1
            RA2, RA_ld = product(Rm, cur, P_ld[perm], cur_ld)
            nxt2, nxt_ld = product(RA2, P, RA_ld, P_ld)
            assert np.array_equal(nxt2.indices, nxt.indices)
            level.update(A_ld=cur_ld, P_ld=P_ld)
        levels.append(level)
        cur, cur_ld = nxt, nxt_ld
    if cur.shape[0] > MAX_COARSE:
        raise ValueError("does not coarsen")
    dense = cur.toarray()
    try:
        np.linalg.cholesky(defsign * dense)
    except np.linalg.LinAlgError:
        raise ValueError("not definite")
    Ainv = np.linalg.inv(dense)
    h = {"levels": levels, "coarse": cur, "Ainv": Ainv, "Ainv_ld": _refined_inverse(dense, Ainv), "defsign": defsign}
    if longdouble:
        dense_ld = np.zeros(dense.shape, dtype=LD)
        dense_ld[np.repeat(np.arange(cur.shape[0]), np.diff(cur.indptr)), cur.indices] = cur_ld
        h.update(coarse_ld=cur_ld, Ainv_exact=_refined_inverse(dense_ld, Ainv))
    return h


def rows_of(h):
    return [lv["A"].shape[0] for lv in h["levels"]] + [h["coarse"].shape[0]]


def operator_complexity(h):
    nnz = [lv["A"].nnz for lv in h["levels"]] + [h["coarse"].nnz]
    return sum(nnz) / nnz[0]


def vcycle(h, Rm, S=DEGREE, ratio=RATIO, dtype=np.float64, level=0):
    """one V-cycle from zero: z ~ A^-1 r.  Per level: Chebyshev smoothing of degree S on [hi / ratio, hi] from zero (d = z = g r /
    theta, S steps), q = r - A z, the level below on P' q (the dense inverse on the last), z += P z_below, then the post-smoother from z:
    one step with (a, b) = (0, 1 / theta), S steps with the recurrence's coefficients."""
    Rm = np.asarray(Rm).astype(dtype)
    Rm = Rm.reshape(Rm.shape[0], -1)
    if level == len(h["levels"]):
        return (h["Ainv"] if dtype == np.float64 else h["Ainv_ld"].astype(dtype)) @ Rm
    lv = h["levels"][level]
    A, P, Rt = lv["A"], lv["P"], lv["R"]
    g = lv["dinv"].astype(dtype)[:, None]
    theta, a, b = C.coefficients(np.float64(lv["hi"]) / np.float64(ratio), lv["hi"], S, dtype)
    D = (g * Rm) / theta
    Z = D.copy()
    for k in range(S):
        D = a[k] * D + b[k] * (g * (Rm - C._matmul(A, Z)))
        Z = Z + D
    Q = Rm - C._matmul(A, Z)
    Z = Z + C._matmul(P, vcycle(h, C._matmul(Rt, Q), S, ratio, dtype, level + 1))
    for a_k, b_k in [(dtype(0), dtype(1) / theta)] + list(zip(a, b)):
        D = a_k * D + b_k * (g * (Rm - C._matmul(A, Z)))
        Z = Z + D
    return Z


def pcg(A, Bm, h, S=DEGREE, ratio=RATIO, tol=1e-10, maxit=1000):
    """conjugate gradients with z = vcycle(r), per-column scalars and the freeze as in cheb_reference.pcg.  Returns X, Columns."""
    A = sp.csr_matrix(A)
    Bm = np.asarray(Bm, dtype=float).reshape(A.shape[0], -1)
    prec = lambda Rm: vcycle(h, Rm, S, ratio)
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
            elif pq[j] == 0.0 or ((pq[j] > 0.0) != (c.rho[j] > 0.0)):  # r.z carries the operator's sign
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


_hier, _solves = {}, {}


def hierarchy(tag, theta=THETA):
    """the hierarchy of problem `tag`, computed once"""
    if (tag, theta) not in _hier:
        A, coarse = problem(tag)
        _hier[(tag, theta)] = (A, setup(A, theta, coarse))
    return _hier[(tag, theta)]


def reference(tag, nc, S=DEGREE, ratio=RATIO, tol=1e-10, seed=5):
    """the restatement's solve with iter_reference's shared right-hand side, computed once: (A, B, X, Columns)"""
    key = (tag, nc, S, ratio, tol, seed)
    if key not in _solves:
        A, h = hierarchy(tag)
        Bm = R.rhs(A.shape[0], nc, seed)
        X, c = pcg(A, Bm, h, S, ratio, tol=tol, maxit=1000)
        X.setflags(write=False)
        _solves[key] = (A, Bm, X, c)
    return _solves[key]
