"""Restatement of the block-Jacobi preconditioner of the iterative A^-1 operator (rails_amd/csrc/block_jacobi_host.h, iter_hierarchy.hip, itsolve.hip,
iter_kernels.inc: iter_pass_block).  Not a test module: tests/test_block_jacobi_host.py checks it on the CPU,
tests/test_gpu_block_jacobi_steps.py and tests/test_gpu_block_jacobi.py compare the device against it.

Contents: the block geometry of the passes (rails_iter_pass_geom_block) in plain Python; the inverse of the diagonal blocks by Gaussian
elimination in np.longdouble with the bound of the library's inverse against it; block-Jacobi conjugate gradients and right-preconditioned
BiCGStab (both `trans` values) step by step, in longdouble or in float64 with the inner products in one of iter_steps_reference.ORDERS;
a float64 restatement run to a tolerance that returns iteration counts; the cases of the step test and their expectation.

The bounds, and where each comes from:

  steps      iter_steps_reference's rule, unchanged: per column and step, max(64 eps (of |x_k^ld|_inf for x), 4 x the float64
             restatement's worst error over the three orders of summation) against the longdouble run, under that module's two
             conditions (no bound above CAP = 4096 eps; rr_k / bb >= 1e-20 at the last step asked for), which
             tests/test_block_jacobi_host.py asserts for every case here.  Nothing is fitted to the device's output.
  inverse    inverse_bound(): the library eliminates in long double (unit roundoff u_ld = eps_ld / 2) by Gauss-Jordan with partial
             pivoting and rounds once to float64; inverse_ld() here eliminates in longdouble too, in another order (LU with partial
             pivoting, then a forward and a back substitution per column of the identity), and is compared unrounded.  With P A = L U
             the factors of inverse_ld()'s own elimination, W = P' |L| |U| and X the inverse (Higham, Accuracy and Stability of
             Numerical Algorithms, 2nd ed.; to first order in u_ld, componentwise):
               LU and two triangular solves (chapter 9):     |x^ - x| <= 3 b u_ld |A^-1| W |x^|
               Gauss-Jordan elimination (chapter 14):        |x^ - x| <= 2 b u_ld (|A^-1| W + 3 |U^-1| |U|) |x^|
             for every column x of the inverse.  The library's own factors differ from the reference's by rounding only (the pivot
             order is the same unless two candidates tie to rounding, which the random blocks here do not), so to first order the same
             W and U stand in both.  The library's one rounding adds eps / 2 |X|:
               |X_lib - X_ld|_ij <= eps / 2 |X|_ij + u_ld (5 b |X| W |X| + 6 b |U^-1| |U| |X|)_ij
             At condition 1e3 this is some tens of eps of the largest entry, at condition 1 about eps / 2: an elimination in float64
             (errors of condition times eps) does not fit under it.
  apply      G X on the device is one accumulator per entry from +0 with one fma per j: |fl(sum) - sum| <= gamma_b (|G| |X|) with
             gamma_b = b u / (1 - b u) < b eps componentwise (Higham, section 3.1, with u = eps / 2), the bound the issue states."""
import numpy as np
import scipy.sparse as sp

import cheb_reference as C
import iter_steps_reference as S

EPS, LD = S.EPS, S.LD
EPS_LD = float(np.finfo(np.longdouble).eps)
BS = (2, 3, 4, 5, 6, 7, 8)


# ------------------------------------------------------------------------------------------------------------------ the geometry
def geometry(nb, w, b):
    """rails_iter_pass_geom_block of iter_geom.h for a group of w <= 32 columns of nb block rows of b rows: (TY, slabs, block rows per slab,
    block rows of the last slab).  Rows per slab are b times the third entry."""
    assert 1 <= w <= S.GROUP and 2 <= b <= 8 and nb >= 1
    pairs = (w + 1) // 2
    tx_bits = 0
    while (1 << tx_bits) < pairs:
        tx_bits += 1
    TY = 256 >> tx_bits
    nslab = max(1, min(1024, nb // (TY * 8)))
    bps = (nb + nslab - 1) // nslab
    nslab = (nb + bps - 1) // bps
    return TY, nslab, bps, nb - (nslab - 1) * bps


# ------------------------------------------------------------------------------------------------------------------ the blocks
def csr_of(triple):
    rowptr, col, val = triple
    n = len(rowptr) - 1
    A = sp.csr_matrix((val, col, rowptr), shape=(n, n))
    A.sort_indices()
    return A


def diagonal_blocks(A, b):
    """the nb diagonal b x b blocks of a scipy matrix, (nb, b, b) float64 (duplicates summed by scipy)"""
    A = sp.csr_matrix(A)
    nb = A.shape[0] // b
    out = np.zeros((nb, b, b))
    coo = A.tocoo()
    keep = coo.row // b == coo.col // b
    np.add.at(out, (coo.row[keep] // b, coo.row[keep] % b, coo.col[keep] % b), coo.data[keep])
    return out


def inverse_ld(blocks):
    """the inverses of (nb, b, b) blocks in longdouble by LU with partial pivoting and two triangular solves per column of the identity,
    and what inverse_bound needs of each elimination: (X, W = P' |L| |U|, V = |U^-1| |U|), each (nb, b, b) longdouble"""
    blocks = np.asarray(blocks, dtype=np.float64)
    nb, b, _ = blocks.shape
    X = np.zeros((nb, b, b), dtype=LD)
    W = np.zeros((nb, b, b), dtype=LD)
    V = np.zeros((nb, b, b), dtype=LD)
    for k in range(nb):
        U = blocks[k].astype(LD)
        L = np.eye(b, dtype=LD)
        perm = np.arange(b)
        for p in range(b):
            q = p + int(np.argmax(np.abs(U[p:, p])))
            if q != p:
                U[[p, q]] = U[[q, p]]
                perm[[p, q]] = perm[[q, p]]
                L[[p, q], :p] = L[[q, p], :p]
            for i in range(p + 1, b):
                L[i, p] = U[i, p] / U[p, p]
                U[i, p:] = U[i, p:] - L[i, p] * U[p, p:]
                U[i, p] = 0
        E = np.eye(b, dtype=LD)[perm]
        Y = np.zeros((b, b), dtype=LD)
        for i in range(b):
            Y[i] = E[i] - L[i, :i] @ Y[:i]
        for i in range(b - 1, -1, -1):
            X[k, i] = (Y[i] - U[i, i + 1:] @ X[k, i + 1:]) / U[i, i]
        W[k, perm] = np.abs(L) @ np.abs(U)  # row i of P A is row perm[i] of A
        Ui = np.zeros((b, b), dtype=LD)
        for i in range(b - 1, -1, -1):
            Ui[i] = (np.eye(b, dtype=LD)[i] - U[i, i + 1:] @ Ui[i + 1:]) / U[i, i]
        V[k] = np.abs(Ui) @ np.abs(U)
    return X, W, V


def inverse_bound(X, W, V):
    """componentwise bound of |library's inverse - X| (module docstring, "inverse"), float64 (nb, b, b)"""
    b = X.shape[1]
    aX = np.abs(X)
    mm = lambda P, Q: np.einsum("kij,kjl->kil", P, Q)
    return (EPS / 2 * aX + (EPS_LD / 2) * (5 * b * mm(mm(aX, W), aX) + 6 * b * mm(V, aX))).astype(np.float64)


def conditioned_blocks(nb, b, cond, seed):
    """nb random b x b blocks of 2-norm condition number `cond`: U diag(s) V' with s spread geometrically over [1, cond]"""
    g = np.random.default_rng(seed)
    U = np.linalg.qr(g.standard_normal((nb, b, b)))[0]
    V = np.linalg.qr(g.standard_normal((nb, b, b)))[0]
    s = cond ** (np.arange(b) / (b - 1.0))
    return (U * s[None, None, :]) @ V.transpose(0, 2, 1)


def apply_blocks(G, R, trans=False):
    """blockdiag(G) @ R (trans: blockdiag(G)') in R's dtype"""
    nb, b, _ = G.shape
    Gd = G.astype(R.dtype)
    R3 = R.reshape(nb, b, -1)
    return np.einsum("kji,kjc->kic" if trans else "kij,kjc->kic", Gd, R3).reshape(R.shape)


def apply_bound(G, X):
    """b eps (|G| |X|): the componentwise bound of the device's G X against the exact product (module docstring, "apply")"""
    b = G.shape[1]
    return b * EPS * apply_blocks(np.abs(G), np.abs(np.asarray(X, dtype=np.float64)))


# ------------------------------------------------------------------------------------------------------------------ the recurrences
def _mul(A, trans, dtype):
    Aop = sp.csr_matrix(A.T) if trans else sp.csr_matrix(A)
    Aop.sort_indices()
    return (lambda Z: Aop @ Z) if dtype == np.float64 else (lambda Z: C._matmul(Aop, Z))


def _cg_group(A, G, B, K, dtype, order):
    mul = _mul(A, False, dtype)
    B = np.asarray(B, dtype=np.float64).astype(dtype)
    dot = lambda a, c: S._dot(a, c, order)
    Rm = B.copy()
    Z = apply_blocks(G, Rm)
    P = Z.copy()
    X = np.zeros_like(Rm)
    out = S.Steps()
    out.bb = dot(Rm, Rm)
    rho = dot(Rm, Z)
    for k in range(K):
        Q = mul(P)
        pq = dot(P, Q)
        assert np.all(pq != 0) and np.all((pq > 0) == (rho > 0)), "the breakdown rule would stop a column"
        alpha = rho / pq
        X = X + alpha[None, :] * P
        Rm = Rm - alpha[None, :] * Q
        Z = apply_blocks(G, Rm)
        rz, rr = dot(Rm, Z), dot(Rm, Rm)
        out.append((X.copy(), rr))
        beta = rz / rho
        rho = rz
        P = Z + beta[None, :] * P
    return out


def _bi_group(A, G, B, K, trans, dtype, order):
    mul = _mul(A, trans, dtype)
    B = np.asarray(B, dtype=np.float64).astype(dtype)
    w = B.shape[1]
    dot = lambda a, c: S._dot(a, c, order)
    prec = lambda M: apply_blocks(G, M, trans)
    Rm = B.copy()
    RH = Rm.copy()
    X, P, V = np.zeros_like(Rm), np.zeros_like(Rm), np.zeros_like(Rm)
    out = S.Steps()
    out.bb = dot(Rm, Rm)
    rho = out.bb.copy()
    zero = np.zeros(w, dtype=dtype)
    alpha, beta, omega = zero, zero, zero
    for k in range(K):
        P = Rm + beta[None, :] * (P - omega[None, :] * V)
        PH = prec(P)
        V = mul(PH)
        rhv = dot(RH, V)
        assert np.all(rhv != 0)
        alpha = rho / rhv
        Sm = Rm - alpha[None, :] * V
        SH = prec(Sm)
        T = mul(SH)
        ts, tt = dot(T, Sm), dot(T, T)
        last = k + 1 == K  # (only a step that follows divides by what a solve that has arrived may round to zero: one block row)
        assert last or np.all(tt != 0)
        omega = np.where(tt != 0, ts / np.where(tt != 0, tt, 1), 0)
        X = (X + alpha[None, :] * PH) + omega[None, :] * SH
        Rm = Sm - omega[None, :] * T
        rhr, rr = dot(RH, Rm), dot(Rm, Rm)
        out.append((X.copy(), rr))
        if last:
            break
        assert np.all(rhr != 0) and np.all(omega != 0)
        beta = (rhr / rho) * (alpha / omega)
        rho = rhr
    return out


def steps(method, A, G, B, K, trans=False, dtype=np.float64, order="numpy"):
    """block-Jacobi CG (trans ignored: a symmetric operator) or right-preconditioned BiCGStab on every column of B from x = 0, K steps:
    iter_steps_reference.Steps.  G: the inverse diagonal blocks the kernels read, (nb, b, b) float64."""
    if method == "cg":
        return S._by_groups(lambda Bg: _cg_group(A, G, Bg, K, dtype, order), B, None)
    return S._by_groups(lambda Bg: _bi_group(A, G, Bg, K, trans, dtype, order), B, None)


def iterations(method, A, B, tol, prec="block", G=None, trans=False, maxit=5000):
    """the float64 restatement run to the relative tolerance `tol` of the recurrence's residual: iterations per column.  prec: "block"
    (G), "point" (the inverse diagonal) or "none"."""
    A = sp.csr_matrix(A)
    Aop = sp.csr_matrix(A.T) if (trans and method != "cg") else A
    B = np.asarray(B, dtype=np.float64).reshape(A.shape[0], -1)
    dinv = 1.0 / A.diagonal()
    if prec == "block":
        M = lambda R: apply_blocks(G, R, trans and method != "cg")
    elif prec == "point":
        M = lambda R: R * dinv[:, None]
    else:
        M = lambda R: R
    out = np.zeros(B.shape[1], dtype=int)
    dot = lambda a, c: float(np.vdot(a, c))
    for j in range(B.shape[1]):
        r = B[:, j:j + 1].copy()
        bb = dot(r, r)
        x = np.zeros_like(r)
        k = 0
        if method == "cg":
            z = M(r)
            p, rho = z.copy(), dot(r, z)
            while k < maxit and dot(r, r) > tol * tol * bb:
                q = Aop @ p
                alpha = rho / dot(p, q)
                x += alpha * p
                r -= alpha * q
                z = M(r)
                rz = dot(r, z)
                p = z + (rz / rho) * p
                rho = rz
                k += 1
        else:
            rh, p, v = r.copy(), np.zeros_like(r), np.zeros_like(r)
            rho, alpha, beta, omega = bb, 0.0, 0.0, 0.0
            while k < maxit and dot(r, r) > tol * tol * bb:
                p = r + beta * (p - omega * v)
                ph = M(p)
                v = Aop @ ph
                alpha = rho / dot(rh, v)
                s = r - alpha * v
                sh = M(s)
                t = Aop @ sh
                omega = dot(t, s) / dot(t, t)
                x += alpha * ph + omega * sh
                r = s - omega * t
                rhr = dot(rh, r)
                beta = (rhr / rho) * (alpha / omega)
                rho = rhr
                k += 1
        out[j] = k
    return out


# ------------------------------------------------------------------------------------------------------------------ the cases
SPREAD = 1e3
SKEW = 0.4
# (nx, ny, nz, b, widths, steps, what the shape reaches); the geometry of every (block rows, width, b) used is in GEOMETRY
# One block row (every b, one step): block Jacobi is the exact inverse there, so x_1 is the solution and the recurrence's residual is
# rounding noise on both sides.  x_1 is held to its bound like every other case; condition 2, which guards the comparison of the
# residuals, cannot hold and is not asked for, and the residuals are not compared (Case.one_block).  A column may even arrive exactly
# (rr = 0): the flag is then "converged", not "stopped at max_iterations".
SHAPES = tuple((1, 1, 1, b, (1, 3), (1,), "one block row, b = %d" % b) for b in BS) + (
    (3, 2, 1, 5, (1, 2, 5), (1, 2, 3), "fewer block rows than row classes"),
    (6, 5, 4, 2, (1, 2, 3, 5, 9, 17, 32, 33), (1, 2, 3), "every tx_bits, odd last columns, one slab; 33: two groups"),
    (6, 5, 4, 4, (3, 17), (1, 2, 3), "b = 4, one slab"),
    (5, 5, 4, 6, (3, 32), (1, 2, 3), "b = 6"),
    (4, 4, 3, 3, (2,), (1, 2, 3), "b = 3 (the large shape of b = 3 runs conjugate gradients only)"),
    (5, 4, 3, 7, (5,), (1, 2, 3), "b = 7"),
    (5, 4, 3, 8, (9,), (1, 2, 3), "b = 8"),
    (13, 13, 13, 3, (3, 32), (1, 2), "2197 block rows: 2 slabs at 3 columns (1099 + 1098), 17 at 32 (130 .. 117)"),
    (17, 8, 32, 2, (32,), (1, 2), "4352 block rows at b = 2: 34 slabs of 128"),
    (17, 8, 16, 2, (17,), (1, 2), "2176 block rows: exactly 17 slabs of 128"),
)
GEOMETRY = {
    **{(1, 1, b): (256, 1, 1, 1) for b in BS}, **{(1, 3, b): (128, 1, 1, 1) for b in BS},
    (6, 1, 5): (256, 1, 6, 6), (6, 2, 5): (256, 1, 6, 6), (6, 5, 5): (64, 1, 6, 6),
    (120, 1, 2): (256, 1, 120, 120), (120, 2, 2): (256, 1, 120, 120), (120, 3, 2): (128, 1, 120, 120), (120, 5, 2): (64, 1, 120, 120),
    (120, 9, 2): (32, 1, 120, 120), (120, 17, 2): (16, 1, 120, 120), (120, 32, 2): (16, 1, 120, 120),
    (120, 3, 4): (128, 1, 120, 120), (120, 17, 4): (16, 1, 120, 120),
    (100, 3, 6): (128, 1, 100, 100), (100, 32, 6): (16, 1, 100, 100),
    (48, 2, 3): (256, 1, 48, 48), (60, 5, 7): (64, 1, 60, 60), (60, 9, 8): (32, 1, 60, 60),
    (2197, 3, 3): (128, 2, 1099, 1098), (2197, 32, 3): (16, 17, 130, 117),
    (4352, 32, 2): (16, 34, 128, 128), (2176, 17, 2): (16, 17, 128, 128),
}
# (name, method, transposed, skew)
VARIANTS = (("cg", "cg", False, 0.0), ("bicgstab", "bicgstab", False, SKEW), ("bicgstab-trans", "bicgstab", True, SKEW))
# the large shapes run conjugate gradients only (every b has run each method at the small ones)
CG_ONLY_ABOVE = 2000


class Case:
    def __init__(self, variant, shape, w):
        self.variant, self.method, self.trans, self.skew = variant
        self.nx, self.ny, self.nz, self.b, _, self.steps, _ = shape
        self.nb = self.nx * self.ny * self.nz
        self.m, self.w = self.nb * self.b, w
        self.one_block = self.nb == 1
        self.id = "%s-%dx%dx%d-b%d-w%d" % (self.variant, self.nx, self.ny, self.nz, self.b, w)

    def problem(self):
        """((indptr, indices, data), scipy CSR matrix) of rails_amd.problems.block_coupled7"""
        from rails_amd import problems as P

        bsr, csr = P.block_coupled7(self.nx, self.ny, self.nz, self.b, SPREAD, skew=self.skew, seed=self.b)
        return bsr, csr_of(csr)

    def rhs(self):
        return S.rhs(self.m, self.w)

    def run(self, G, dtype=np.float64, order="numpy", K=None):
        return steps(self.method, self.problem()[1], G, self.rhs(), K or max(self.steps), self.trans, dtype, order)


def _cases():
    out = []
    for variant in VARIANTS:
        for shape in SHAPES:
            if variant[1] != "cg" and shape[0] * shape[1] * shape[2] > CG_ONLY_ABOVE:
                continue
            out += [Case(variant, shape, w) for w in shape[4]]
    return out


CASES = _cases()


def case(case_id):
    return next(c for c in CASES if c.id == case_id)


def reference_inverse(A, b):
    """the inverse diagonal blocks as float64, from inverse_ld: what the library uploads, up to the bound of inverse_bound"""
    return inverse_ld(diagonal_blocks(A, b))[0].astype(np.float64)


class Expected(S.Expected):
    """iter_steps_reference.Expected for a case here: the longdouble run, the float64 runs in the three orders, the bounds.  G: the
    inverse blocks the runs apply (the library's own, from rails_iter_block_jacobi_info, on the GPU; reference_inverse on the host)."""

    def __init__(self, c, G):
        class _Bound:  # what S.Expected asks of a case
            steps = c.steps

            @staticmethod
            def run(dtype=np.float64, order="numpy"):
                return c.run(G, dtype=dtype, order=order)

        S.Expected.__init__(self, _Bound)
        self.case = c
