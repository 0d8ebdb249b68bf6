"""A numpy/scipy restatement of the block multigrid preconditioner of the iterative A^-1 operator (rails_amd/csrc/block_amg_host.h and
block_amg_host.cpp for the set-up; itsolve.hip: Run::vcycle with the block sweeps, iter_kernels.inc: k_cheb_step_bsr, k_amg_residual_bsr,
k_cheb_init_bj, k_cheb_pass_bj for the cycle; block_amg_choice.h for the launch decision), written from the rules and not by calling the
library.  The set-up: the condensed node matrix, the aggregation passes of tests/amg_reference.py on it, T = T_nodes (x) I_b, the inverse
diagonal blocks, the bound hi, the smoothed prolongator, the Galerkin product, the stop rules, the dense inverse -- in float64 and, on the
same patterns, in longdouble.  The cycle in float64 in three orders of summation and in longdouble.  Conjugate gradients with the cycle
and with block Jacobi.  Not a test module: tests/test_block_amg_host.py compares the host set-up against it, tests/test_gpu_block_amg.py
the device.

Bounds, none of them fitted to the device.  A value of the library is held to max(4 e64, 64 eps scale): e64 is the float64 restatement's
own error against its longdouble evaluation (for the cycle: the worst of the three orders of summation), scale the sum of the absolute
values of the terms the value is made of (for the cycle: ||z||_inf of the column) -- the rule of tests/test_gpu_iter_amg.py::expected and
tests/test_amg_host.py::value_bound.  The inverse blocks are held to block_jacobi_reference.inverse_bound."""
import os
import sys

import numpy as np
import scipy.sparse as sp

import amg_reference as M
import block_jacobi_reference as J
import bsr_reference as K
import cheb_reference as C
import iter_reference as R

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rails_amd import problems as P  # noqa: E402

THETA, COARSE, RATIO, DEGREE = 0.08, 256, 4.0, 1
MAX_LEVELS, MAX_COARSE, MAX_ROWS = 16, 1024, 1 << 24
LD = np.longdouble
EPS = np.finfo(float).eps


def value_bound(err64, scale):
    return np.maximum(4 * err64, 64 * EPS * scale)


def bsr_of(triple):
    """scipy's block matrix of (indptr, indices, data[nnzb, b, b])"""
    indptr, indices, data = triple
    b = data.shape[1]
    mb = len(indptr) - 1
    return sp.bsr_matrix((np.asarray(data, dtype=float), np.asarray(indices), np.asarray(indptr)), shape=(mb * b, mb * b))


def expand(indptr, indices, data):
    """the expanded CSR matrix: scalar row I b + r holds row r of each block of block row I in stored order, zeros kept"""
    nnzb, b, _ = data.shape
    mb = len(indptr) - 1
    counts = np.diff(indptr)
    brow = np.repeat(np.arange(mb), counts)
    rowptr = np.zeros(mb * b + 1, dtype=np.int64)
    np.cumsum(np.repeat(counts, b) * b, out=rowptr[1:])
    col = np.empty(nnzb * b * b, dtype=np.int64)
    val = np.empty(nnzb * b * b, dtype=data.dtype)
    within = np.arange(nnzb) - indptr[brow]
    for r in range(b):
        at = rowptr[brow * b + r] + within * b
        for s in range(b):
            col[at + s] = indices * b + s
            val[at + s] = data[:, r, s]
    if data.dtype == LD:
        return rowptr, col, val
    return sp.csr_matrix((val, col, rowptr), shape=(mb * b, mb * b))


def block_up(A, b):
    """the block-CSR arrays of a block-aligned CSR matrix (rails_bsr_fill_host): touched blocks, sorted block columns, zeros kept; and
    the map from the entries of A to (block, r, s), for values in another precision"""
    A = sp.csr_matrix(A)
    mb = A.shape[0] // b
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    key = (rows // b) * (A.shape[1] // b) + A.indices // b
    uniq, inv = np.unique(key, return_inverse=True)
    bi, bj = uniq // (A.shape[1] // b), uniq % (A.shape[1] // b)
    indptr = np.zeros(mb + 1, dtype=np.int64)
    np.cumsum(np.bincount(bi, minlength=mb), out=indptr[1:])
    data = np.zeros((uniq.size, b, b))
    where = (inv, rows % b, A.indices % b)
    np.add.at(data, where, A.data)
    return (indptr, bj.astype(np.int64), data), where


def condensed(indptr, indices, data):
    """N: the block pattern with the Frobenius norms, the squares added in stored order"""
    bb = data.shape[1] ** 2
    flat = data.reshape(-1, bb)
    s = np.zeros(flat.shape[0])
    for e in range(bb):
        s = s + flat[:, e] * flat[:, e]
    mb = len(indptr) - 1
    return sp.csr_matrix((np.sqrt(s), indices, indptr), shape=(mb, mb))


def scaled_blocks(indptr, indices, data, G):
    """G A block by block -- entry (r, s) one sum over k ascending of a product, then an addition -- and hi = max_i sum_j |(G A)_ij|, the
    blocks in stored order, s ascending"""
    nnzb, b, _ = data.shape
    mb = len(indptr) - 1
    brow = np.repeat(np.arange(mb), np.diff(indptr))
    g = G[brow]
    ga = np.zeros_like(data)
    for k in range(b):
        ga = ga + g[:, :, k, None] * data[:, None, k, :]
    rowsum = np.zeros((mb, b), dtype=data.dtype)
    within = np.arange(nnzb) - indptr[brow]
    for k in range(int(np.diff(indptr).max())):
        sel = np.flatnonzero(within == k)
        for s in range(b):
            rowsum[brow[sel]] = rowsum[brow[sel]] + np.abs(ga[sel, :, s])
    return ga, rowsum.max()


def check(indptr, indices, data):
    mb = len(indptr) - 1
    if not np.all(np.isfinite(data)):
        raise ValueError("not finite")
    for i in range(mb):
        c = indices[indptr[i]:indptr[i + 1]]
        if np.any(np.diff(c) <= 0):
            raise ValueError("not strictly increasing")
        if i not in c:
            raise ValueError("no stored diagonal block")


def setup(triple, theta=THETA, coarse=COARSE, longdouble=False, first_level=0, one_level=False):
    """the hierarchy: {"b", "levels": [{"bsr": (indptr, indices, data), "A" (expanded csr), "P", "R", "G", "hi", "agg"}], "coarse" (csr),
    "coarse_bsr", "Ainv", "Ainv_ld", "defsign"}.  longdouble=True: the same set-up on the same aggregates and patterns evaluated in longdouble
    beside it: "A_ld", "P_ld", "hi_ld", "G_ld" (with "G_bound") per level and "coarse_ld", "Ainv_exact".  ValueError where the library refuses.
    one_level=True: one step of the set-up from a matrix that is level `first_level` of a hierarchy (its strength threshold), without the
    dense inverse: what a level of the library's hierarchy is held to, given the library's own matrix of that level."""
    indptr, indices, data = (np.asarray(triple[0], dtype=np.int64), np.asarray(triple[1], dtype=np.int64), np.asarray(triple[2], dtype=float))
    b = data.shape[1]
    check(indptr, indices, data)
    levels = []
    cur = (indptr, indices, data)
    cur_ld = data.astype(LD)
    defsign = None
    while True:
        ip, ix, dt = cur
        mb = len(ip) - 1
        brow = np.repeat(np.arange(mb), np.diff(ip))
        dblocks = dt[ix == brow]
        d = dblocks[:, np.arange(b), np.arange(b)]
        if defsign is None:
            defsign = -1.0 if d.flat[0] < 0 else 1.0
        if np.any(d == 0) or np.any(np.sign(d) != defsign):
            raise ValueError("not definite")
        E = expand(ip, ix, dt)
        if mb * b <= coarse or len(levels) + 1 + first_level >= MAX_LEVELS or (one_level and levels):
            break
        N = condensed(ip, ix, dt)
        agg, n_agg = M.aggregate(N, N.diagonal(), theta * 0.5 ** (len(levels) + first_level))
        if n_agg * 5 > mb * 4:
            break
        with np.errstate(all="ignore"):
            X, W, V = J.inverse_ld(dblocks)
        if not np.all(np.isfinite(X.astype(float))):
            raise ValueError("singular diagonal block")
        G = X.astype(float)
        ga, hi = scaled_blocks(ip, ix, dt, G)
        hi = float(hi)
        GA = expand(ip, ix, ga)
        n = mb * b
        tcol = np.repeat(agg, b) * b + np.tile(np.arange(b), mb)
        T = sp.csr_matrix((np.ones(n), tcol, np.arange(n + 1)), shape=(n, n_agg * b))
        if longdouble:
            ga_ld, hi_ld = scaled_blocks(ip, ix, cur_ld, G.astype(LD))
            ga_ld = expand(ip, ix, ga_ld)[2]
        AT, AT_ld = M.product(GA, T, ga_ld if longdouble else None, T.data.astype(LD))
        prow = np.repeat(np.arange(n), np.diff(AT.indptr))
        own = AT.indices == tcol[prow]
        Pm = AT.copy()
        Pm.data = np.where(own, 1.0, 0.0) - (4.0 / (3.0 * hi)) * AT.data
        Rm = sp.csr_matrix(Pm.T)
        RA, _ = M.product(Rm, E)
        nxt, _ = M.product(RA, Pm)
        nxt_bsr, where = block_up(nxt, b)
        level = {"bsr": cur, "A": E, "P": Pm, "R": Rm, "G": G, "hi": hi, "agg": agg}
        nxt_ld = None
        if longdouble:
            P_ld = np.where(own, LD(1), LD(0)) - (LD(4) / (LD(3) * hi_ld)) * AT_ld
            perm = sp.csr_matrix((np.arange(1, Pm.nnz + 1), Pm.indices, Pm.indptr), shape=Pm.shape).T.tocsr().data - 1
            E_ld = expand(ip, ix, cur_ld)[2]
            RA2, RA_ld = M.product(Rm, E, P_ld[perm], E_ld)
            nxt2, vals_ld = M.product(RA2, Pm, RA_ld, P_ld)
            assert np.array_equal(nxt2.indices, nxt.indices)
            nxt_ld = np.zeros(nxt_bsr[2].shape, dtype=LD)
            np.add.at(nxt_ld, where, vals_ld)
            level.update(A_ld=cur_ld, P_ld=P_ld, hi_ld=hi_ld, G_ld=X, G_bound=J.inverse_bound(X, W, V))
        levels.append(level)
        cur, cur_ld = nxt_bsr, nxt_ld
    if one_level:
        return {"b": b, "levels": levels, "coarse": E, "coarse_bsr": cur, "coarse_ld": cur_ld, "defsign": defsign}
    if E.shape[0] > MAX_COARSE:
        raise ValueError("does not coarsen")
    dense = E.toarray()
    try:
        np.linalg.cholesky(defsign * dense)
    except np.linalg.LinAlgError:
        raise ValueError("not definite")
    Ainv = np.linalg.inv(dense)
    h = {"b": b, "levels": levels, "coarse": E, "coarse_bsr": cur, "Ainv": Ainv, "Ainv_ld": M._refined_inverse(dense, Ainv), "defsign": defsign}
    if longdouble:
        rp, cl, vl = expand(cur[0], cur[1], cur_ld)
        dense_ld = np.zeros(dense.shape, dtype=LD)
        dense_ld[np.repeat(np.arange(E.shape[0]), np.diff(rp)), cl] = vl
        h.update(coarse_ld=cur_ld, Ainv_exact=M._refined_inverse(dense_ld, Ainv))
    return h


def rows_of(h):
    return [lv["A"].shape[0] for lv in h["levels"]] + [h["coarse"].shape[0]]


def nnz_of(h):
    return [lv["A"].nnz for lv in h["levels"]] + [h["coarse"].nnz]


def operator_complexity(h):
    return sum(nnz_of(h)) / nnz_of(h)[0]


ORDERS = ("stored", "reversed", "halves")


def _matmul(A, Z, order="stored"):
    """A Z in the precision of Z; float64 in one of three orders of summation within a row: the stored order, the reverse of it, and
    the even entries of a row and its odd entries summed apart and then added"""
    if Z.dtype != np.float64 or order == "stored":
        return C._matmul(A, Z)
    if order == "reversed":
        n = A.shape[1]
        Ar = sp.csr_matrix(A[:, ::-1])
        Ar.sort_indices()
        return Ar @ Z[::-1]
    pos = np.arange(A.nnz) - np.repeat(A.indptr[:-1], np.diff(A.indptr))
    halves = []
    for parity in (0, 1):
        H = sp.csr_matrix((np.where(pos % 2 == parity, A.data, 0.0), A.indices, A.indptr), shape=A.shape)
        halves.append(H @ Z)
    return halves[0] + halves[1]


def vcycle(h, Rm, S=DEGREE, ratio=RATIO, dtype=np.float64, order="stored", level=0):
    """one V-cycle from zero (tests/amg_reference.py::vcycle) with G the level's inverse diagonal blocks"""
    Rm = np.asarray(Rm).astype(dtype)
    Rm = Rm.reshape(Rm.shape[0], -1)
    if level == len(h["levels"]):
        Ai = h["Ainv"] if dtype == np.float64 else h["Ainv_ld"].astype(dtype)
        if dtype == np.float64 and order == "reversed":
            return Ai[:, ::-1] @ Rm[::-1]
        return Ai @ Rm
    lv = h["levels"][level]
    A, Pm, Rt = lv["A"], lv["P"], lv["R"]
    g = lambda X: J.apply_blocks(lv["G"], X)
    mul = lambda Mx, X: _matmul(Mx, X, order)
    theta, a, b = C.coefficients(np.float64(lv["hi"]) / np.float64(ratio), lv["hi"], S, dtype)
    D = g(Rm) / theta
    Z = D.copy()
    for k in range(S):
        D = a[k] * D + b[k] * g(Rm - mul(A, Z))
        Z = Z + D
    Q = Rm - mul(A, Z)
    Z = Z + mul(Pm, vcycle(h, mul(Rt, Q), S, ratio, dtype, order, level + 1))
    for a_k, b_k in [(dtype(0), dtype(1) / theta)] + list(zip(a, b)):
        D = a_k * D + b_k * g(Rm - mul(A, Z))
        Z = Z + D
    return Z


def cycle_reference(h, Xm, S, ratio=RATIO):
    """(the longdouble cycle, the allowed error per column): 4 times the worst error of the three float64 orders against longdouble, at
    least 64 eps ||z||_inf"""
    Zl = vcycle(h, Xm, S, ratio, dtype=LD)
    worst = np.zeros(Zl.shape[1])
    for order in ORDERS:
        worst = np.maximum(worst, np.abs(vcycle(h, Xm, S, ratio, order=order) - Zl).max(0).astype(float))
    return Zl, np.maximum(4 * worst, 64 * EPS * np.abs(Zl).max(0).astype(float))


def pcg(A, Bm, prec, tol=1e-8, maxit=1000):
    """conjugate gradients with z = prec(r), per-column scalars and the freeze of tests/amg_reference.py::pcg.  Returns X, Columns."""
    h = {"levels": [], "Ainv": None}
    orig = M.vcycle
    try:
        M.vcycle = lambda _h, Rm, S, ratio: prec(Rm)
        return M.pcg(A, Bm, h, tol=tol, maxit=maxit)
    finally:
        M.vcycle = orig


# ---------------------------------------------------------------------------------------------------------------- the launch decision
bsr_choice = K.bsr_choice  # bsr_choice.h, restated once: tests/bsr_reference.py


def rows_ok(m, b):
    return 2 <= b <= 8 and m >= b and m % b == 0 and m < MAX_ROWS


def step_choice(b, nc, mb, max_brow, ld, want_fused, num_cu=256):
    """block_amg_choice.h::rails_bamg_step: (ok, fused, lds_bytes).  Every instantiation of the fused kernels is free of spills in the
    gfx950 build (profiles/block_amg_kernel_resources.txt), so the rule sends no block size to the unfused step on its own."""
    k = bsr_choice(b, nc, mb, max_brow, num_cu)
    if k is None or nc > 32 or ld < nc:
        return False, False, 0
    cap = 4096 // (b * b)
    return True, bool(want_fused), cap * b * b * 8 + cap * 4


# ---------------------------------------------------------------------------------------------------------------- shared problems
_hier = {}


def long_row(nx, ny, nz, b, seed=0):
    """block_diffusion7 with cell 0 coupled symmetrically to all others by 0.01 K-like blocks and the diagonal raised to keep the matrix
    negative definite: a block row of nx ny nz blocks, longer than the LDS buffer at b = 8 from 65 cells on"""
    (ip, ix, dt), _ = P.block_diffusion7(nx, ny, nz, b, 100.0, 0.01, seed)
    A = bsr_of((ip, ix, dt)).tolil()
    mb = nx * ny * nz
    Kc = 0.01 * np.eye(b)
    for j in range(1, mb):
        A[0:b, j * b:(j + 1) * b] = A[0:b, j * b:(j + 1) * b].toarray() + Kc
        A[j * b:(j + 1) * b, 0:b] = A[j * b:(j + 1) * b, 0:b].toarray() + Kc
        A[j * b:(j + 1) * b, j * b:(j + 1) * b] = A[j * b:(j + 1) * b, j * b:(j + 1) * b].toarray() - 0.02 * np.eye(b)
    A[0:b, 0:b] = A[0:b, 0:b].toarray() - 0.02 * mb * np.eye(b)
    Bm = sp.bsr_matrix(A.tocsr(), blocksize=(b, b))
    Bm.sort_indices()
    return Bm.indptr.astype(np.int64), Bm.indices.astype(np.int64), Bm.data.copy()


def problem(tag):
    """(block triple, coarse) of a named problem: "d<nx>x<ny>x<nz>b<b>[c<coarse>][p]" is block_diffusion7 (spread 100, reaction 0.01; p:
    negated, positive definite), "one<b>" one block row, "long8" the long block row at b = 8"""
    if tag.startswith("one"):
        b = int(tag[3:])
        (ip, ix, dt), _ = P.block_diffusion7(1, 1, 1, b, 100.0, 0.01, seed=b)
        return (ip, ix, dt), COARSE
    if tag == "long8":
        return long_row(6, 4, 3, 8), 64
    body = tag[1:]
    sign = 1.0
    if body.endswith("p"):
        body, sign = body[:-1], -1.0
    coarse = COARSE
    if "c" in body:
        body, c = body.split("c")
        coarse = int(c)
    dims, b = body.split("b")
    nx, ny, nz = (int(v) for v in dims.split("x"))
    (ip, ix, dt), _ = P.block_diffusion7(nx, ny, nz, int(b), 100.0, 0.01)
    return (ip, ix, sign * dt), coarse


def hierarchy(tag, theta=THETA):
    """(expanded matrix, hierarchy) of problem `tag`, computed once"""
    if (tag, theta) not in _hier:
        triple, coarse = problem(tag)
        _hier[(tag, theta)] = (expand(*[np.asarray(t) for t in triple]), setup(triple, theta, coarse))
    return _hier[(tag, theta)]


def block_jacobi_of(triple):
    ip, ix, dt = (np.asarray(t) for t in triple)
    brow = np.repeat(np.arange(len(ip) - 1), np.diff(ip))
    return J.inverse_ld(dt[ix == brow])[0].astype(float)
