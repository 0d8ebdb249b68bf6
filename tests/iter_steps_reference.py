"""Step-by-step restatement of the iterative A^-1 operator's recurrences (rails_amd/csrc/itsolve.hip, iter_scalars.h), the case list, the
bounds and a plain restatement of the pass geometry (iter_geom.h).  Not a test module: tests/test_iter_steps_host.py checks it on the CPU (the
bounds' conditions, the geometry table, seeded mistakes), tests/test_gpu_iter_steps.py compares the device against it.

Why step by step.  A Krylov iteration corrects itself: x and r move with the same alpha, so a wrong inner product costs a converged solve a
few iterations and nothing else.  With tolerance 0 and max_iterations k a solve stops every column after exactly k iterations and delivers
x_k and sqrt(rr_k / bb); x_k depends on every alpha, beta and omega up to k, so on every inner product, reduction and update pass.  The
restatement here is free of frozen columns: the inputs are chosen so that no column stops before the last step asked for (condition 2).

cg_steps and bicgstab_steps run one iteration after another and return (x_k, rr_k) for k = 1 .. K, in np.longdouble (products as
cheb_reference._matmul takes them) or in float64 with the inner products summed in one of ORDERS:

  "numpy"     numpy's own (pairwise) sum
  "reversed"  sequential, from the last row to the first
  "classes"   16 interleaved row classes, each summed sequentially, then added 0 .. 15: the device's shape

Bounds, per column and per step, against the longdouble run (the rule of test_gpu_iter_poly.py::expected: a margin of 4 over a correct
float64 implementation in another order of summation, a floor of 64 eps):

  |x_k - x_k^ld|_inf      <= max(64 eps |x_k^ld|_inf, 4 * worst error of the float64 restatement over ORDERS)
  |relres_k - relres_k^ld| <= max(64 eps,             4 * the restatement's worst)        (already relative to ||b||)

Conditions (host arithmetic, not measurements; test_iter_steps_host.py asserts them for every case):

  1. no bound exceeds CAP = 4096 eps, of |x_k^ld|_inf for x and absolutely for the residual;
  2. in the longdouble run every column still has rr_k / bb >= 1e-20 at the last step asked for.

A case that misses one at some width gets fewer steps; the cap is not raised.

Seeded mistakes (MISTAKES) are variants of the float64 restatement; each must leave the bounds at the smallest case that can show it."""
import numpy as np
import scipy.sparse as sp

import cheb_reference as C
import iter_reference as R

EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble
ORDERS = ("numpy", "reversed", "classes")
FLOOR, MARGIN, CAP, RR_FLOOR = 64 * EPS, 4.0, 4096 * EPS, 1e-20
GROUP = 32          # RAILS_ITER_GROUP
POLY_RATIO = 30.0   # "poly_ratio" of the polynomial cases
POLY_DEGREE = 2


# ------------------------------------------------------------------------------------------------------------------ the problems
def tridiag(m, lower, diag, upper):
    e = np.ones(m)
    return sp.diags([lower * e[:-1], diag * e, upper * e[:-1]], [-1, 0, 1]).tocsr() if m > 1 else sp.csr_matrix(np.array([[float(diag)]]))


def matrix(method, m, negated=False):
    """CG: scaled(tridiag(-1, 2.5, -1), 21), symmetric positive definite; BiCGStab: scaled(tridiag(1.7, -4.0, 0.3), 22).  The scaling
    spreads the diagonal over three decades, so Jacobi on and off are different computations."""
    A = R.scaled(tridiag(m, -1.0, 2.5, -1.0), 21) if method == "cg" else R.scaled(tridiag(m, 1.7, -4.0, 0.3), 22)
    A = sp.csr_matrix(-A if negated else A)
    A.sort_indices()
    return A


def rhs(m, w):
    return R.rhs(m, w, seed=11)


# ------------------------------------------------------------------------------------------------------------------ the geometry
def geometry(m, w):
    """rails_iter_pass_geom of iter_geom.h for a group of w <= 32 columns of m rows: (TY, slabs, rows per slab, rows of the last slab)"""
    assert 1 <= w <= GROUP
    pairs = (w + 1) // 2
    tx_bits = 0
    while (1 << tx_bits) < pairs:
        tx_bits += 1
    TY = 256 >> tx_bits
    nslab = max(1, min(1024, m // (TY * 8)))
    rps = (m + nslab - 1) // nslab
    nslab = (m + rps - 1) // rps
    return TY, nslab, rps, m - (nslab - 1) * rps


def groups(w):
    """the column groups of a solve of w columns: [(first column, width)]"""
    return [(g0, min(GROUP, w - g0)) for g0 in range(0, w, GROUP)]


# ------------------------------------------------------------------------------------------------------------------ the inner products
MISTAKES = ("dot_skips_last_row_of_slab", "reduce_skips_last_slab", "beta_from_neighbour", "alpha_from_neighbour", "p_without_omega_v",
            "x_with_p_not_dinv_p", "rr_before_omega_t", "jacobi_row0_everywhere")


def _dot(a, b, order, keep=None):
    """per-column inner products of two m x w arrays; keep: a row mask (the mistakes that drop rows)"""
    prod = a * b
    if keep is not None:
        prod = prod[keep]
    if prod.dtype != np.float64 or order == "numpy":
        return prod.sum(0)
    if order == "reversed":
        return np.cumsum(prod[::-1], axis=0)[-1] if prod.shape[0] else np.zeros(prod.shape[1])
    assert order == "classes"
    n, w = prod.shape
    pad = np.zeros(((n + 15) // 16 * 16, w))
    pad[:n] = prod
    cls = np.cumsum(pad.reshape(-1, 16, w), axis=0)[-1]  # row class c = rows c, c + 16, ... in increasing order
    s = np.zeros(w)
    for c in range(16):
        s = s + cls[c]
    return s


def _row_mask(m, w, bug):
    TY, nslab, rps, last = geometry(m, w)
    if bug == "dot_skips_last_row_of_slab":
        keep = np.ones(m, dtype=bool)
        keep[np.minimum(np.arange(1, nslab + 1) * rps, m) - 1] = False
        return keep
    if bug == "reduce_skips_last_slab" and nslab > 16:
        keep = np.ones(m, dtype=bool)
        keep[(nslab - 1) * rps:] = False
        return keep
    return None


def _neighbour(v):
    """every column takes the value of the other column of its pair (2 t, 2 t + 1); an odd last column has none and keeps its own"""
    j = np.arange(v.size) ^ 1
    j[j >= v.size] = v.size - 1
    return v[j]


# ------------------------------------------------------------------------------------------------------------------ the recurrences
class Steps(list):
    """[(x_1, rr_1), ..., (x_K, rr_K)] with .bb, the squared norms of the right-hand sides as the start pass sums them"""
    bb = None

    def relres(self, k):
        return np.sqrt(self[k - 1][1] / self.bb)


def _setup(A, B, jacobi, trans, dtype):
    A = sp.csr_matrix(A)
    A.sort_indices()
    d = np.asarray(A.diagonal(), dtype=np.float64)
    dinv = (1.0 / d).astype(dtype) if jacobi else None  # the library inverts in float64: the rounded factors are the kernels' input
    Aop = sp.csr_matrix(A.T) if trans else A
    Aop.sort_indices()
    B = np.asarray(B, dtype=np.float64).reshape(A.shape[0], -1).astype(dtype)
    mul = (lambda Z: Aop @ Z) if dtype == np.float64 else (lambda Z: C._matmul(Aop, Z))
    return A, d, dinv, mul, B


def _cg_group(A, B, K, jacobi, dtype, order, poly, bug):
    A, d, dinv, mul, B = _setup(A, B, jacobi, False, dtype)
    m, w = B.shape
    keep = _row_mask(m, w, bug)
    dot = lambda a, b: _dot(a, b, order, keep)
    sign = 1.0
    if poly:
        g = C.g_of(A, jacobi)
        hi = C.gershgorin(A, g)
        prec = lambda Rm: C.polynomial(A, Rm, poly, hi, POLY_RATIO, g, dtype=dtype)
    elif jacobi:
        dv = np.full(m, dinv[0]) if bug == "jacobi_row0_everywhere" else dinv
        prec = lambda Rm: Rm * dv[:, None]
    else:
        prec = lambda Rm: Rm
        sign = -1.0 if np.all(d < 0) else 1.0  # iter_scalars.h: the sign p.q / rho must have without the preconditioner
    Rm = B.copy()
    Z = prec(Rm)
    P = Z.copy()
    X = np.zeros_like(Rm)
    out = Steps()
    out.bb = dot(Rm, Rm)
    rho = dot(Rm, Z)
    for k in range(K):
        Q = mul(P)
        pq = dot(P, Q)
        assert np.all(pq != 0) and np.all((pq > 0) == (sign * rho > 0)), "the breakdown rule would stop a column"
        alpha = rho / pq
        if bug == "alpha_from_neighbour":
            alpha = _neighbour(alpha)
        X = X + alpha[None, :] * P
        Rm = Rm - alpha[None, :] * Q
        Z = prec(Rm)
        rz, rr = dot(Rm, Z), dot(Rm, Rm)
        out.append((X.copy(), rr))
        beta = rz / rho
        if bug == "beta_from_neighbour":
            beta = _neighbour(beta)
        rho = rz
        P = Z + beta[None, :] * P
    return out


def _bi_group(A, B, K, jacobi, trans, dtype, order, bug):
    A, d, dinv, mul, B = _setup(A, B, jacobi, trans, dtype)
    m, w = B.shape
    keep = _row_mask(m, w, bug)
    dot = lambda a, b: _dot(a, b, order, keep)
    if jacobi:
        dv = np.full(m, dinv[0]) if bug == "jacobi_row0_everywhere" else dinv
        prec = lambda Rm: Rm * dv[:, None]
    else:
        prec = lambda Rm: Rm
    Rm = B.copy()
    RH = Rm.copy()
    X, P, V = np.zeros_like(Rm), np.zeros_like(Rm), np.zeros_like(Rm)
    out = Steps()
    out.bb = dot(Rm, Rm)
    rho = out.bb.copy()
    zero = np.zeros(w, dtype=dtype)
    alpha, beta, omega = zero, zero, zero
    for k in range(K):
        P = Rm + beta[None, :] * (P if bug == "p_without_omega_v" else P - omega[None, :] * V)
        PH = prec(P)
        V = mul(PH)
        rhv = dot(RH, V)
        assert np.all(rhv != 0)
        alpha = rho / rhv
        if bug == "alpha_from_neighbour":
            alpha = _neighbour(alpha)
        S = Rm - alpha[None, :] * V
        SH = prec(S)
        T = mul(SH)
        ts, tt = dot(T, S), dot(T, T)
        assert np.all(tt != 0)
        omega = ts / tt
        X = (X + alpha[None, :] * (P if bug == "x_with_p_not_dinv_p" else PH)) + omega[None, :] * SH
        Rm = S - omega[None, :] * T
        rhr = dot(RH, Rm)
        rr = dot(S, S) if bug == "rr_before_omega_t" else dot(Rm, Rm)
        out.append((X.copy(), rr))
        assert np.all(rhr != 0) and np.all(omega != 0)
        beta = (rhr / rho) * (alpha / omega)
        if bug == "beta_from_neighbour":
            beta = _neighbour(beta)
        rho = rhr
    return out


def _by_groups(run_group, B, chunk):
    """the columns are systems of their own: run the groups of 32 (the geometry, and so the mistakes that drop rows, goes by the group's
    width) and put the columns together again.  chunk: columns at a time where no mistake depends on the group (a large longdouble
    product's temporary)"""
    B = np.asarray(B, dtype=np.float64)
    B = B.reshape(B.shape[0], -1)
    parts = []
    for g0, gw in groups(B.shape[1]):
        step = gw if chunk is None else chunk
        parts += [run_group(B[:, g0 + c0:g0 + min(c0 + step, gw)]) for c0 in range(0, gw, step)]
    out = Steps()
    out.bb = np.concatenate([p.bb for p in parts])
    for k in range(len(parts[0])):
        out.append((np.hstack([p[k][0] for p in parts]), np.concatenate([p[k][1] for p in parts])))
    return out


def cg_steps(A, B, K, jacobi=True, trans=False, dtype=np.float64, order="numpy", poly=0, bug=None, chunk=None):
    """conjugate gradients on every column of B from x = 0: Steps of K entries.  trans is ignored (a symmetric operator), as the library
    does.  poly: degree of the Chebyshev polynomial preconditioner (cheb_reference.polynomial; Gershgorin bound, POLY_RATIO)."""
    assert bug is None or (bug in MISTAKES and chunk is None)
    return _by_groups(lambda Bg: _cg_group(A, Bg, K, jacobi, dtype, order, poly, bug), B, chunk)


def bicgstab_steps(A, B, K, jacobi=True, trans=False, dtype=np.float64, order="numpy", bug=None, chunk=None):
    """right-preconditioned BiCGStab on every column of B from x = 0: Steps of K entries"""
    assert bug is None or (bug in MISTAKES and chunk is None)
    return _by_groups(lambda Bg: _bi_group(A, Bg, K, jacobi, trans, dtype, order, bug), B, chunk)


# ------------------------------------------------------------------------------------------------------------------ the cases
# rows -> (widths, steps, what the shape reaches)
SHAPES = {
    5: ((2, 3), (1, 2, 3), "fewer rows than row classes"),
    72: ((1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32, 70), (1, 2, 3, 8), "every tx_bits, odd last columns, one slab; 70: three groups"),
    2181: ((3, 17, 32, 33), (1, 2, 3, 8), "17 ragged slabs at 17 and 32 (the strands' second trip), 2 at 3; 33: groups of 32 and 1"),
    4231: ((16, 32), (1, 2), "exactly 16 slabs; 33 slabs"),
    131168: ((32,), (1, 2), "the cap of 1024 slabs"),
}
# the geometry the shapes were chosen for: (rows, width of the group) -> (TY, slabs, rows per slab, rows of the last slab)
GEOMETRY = {
    (5, 2): (256, 1, 5, 5), (5, 3): (128, 1, 5, 5),
    (72, 1): (256, 1, 72, 72), (72, 2): (256, 1, 72, 72), (72, 3): (128, 1, 72, 72), (72, 4): (128, 1, 72, 72), (72, 5): (64, 1, 72, 72),
    (72, 8): (64, 1, 72, 72), (72, 9): (32, 1, 72, 72), (72, 16): (32, 1, 72, 72), (72, 17): (16, 1, 72, 72), (72, 31): (16, 1, 72, 72),
    (72, 32): (16, 1, 72, 72), (72, 6): (64, 1, 72, 72),
    (2181, 3): (128, 2, 1091, 1090), (2181, 17): (16, 17, 129, 117), (2181, 32): (16, 17, 129, 117), (2181, 1): (256, 1, 2181, 2181),
    (4231, 16): (32, 16, 265, 256), (4231, 32): (16, 33, 129, 103),
    (131168, 32): (16, 1017, 129, 104),
}
# (name, method, Jacobi, transposed, negated, polynomial degree, fused step, rows it runs at (None: all))
VARIANTS = (
    ("cg-jacobi", "cg", True, False, False, 0, True, None),
    ("cg-plain", "cg", False, False, False, 0, True, None),
    ("bicgstab-jacobi", "bicgstab", True, False, False, 0, True, None),
    ("bicgstab-plain", "bicgstab", False, False, False, 0, True, None),  # k_bi_update reads s^ through the pointer it writes r to
    ("bicgstab-jacobi-trans", "bicgstab", True, True, False, 0, True, (72, 2181)),
    ("bicgstab-plain-trans", "bicgstab", False, True, False, 0, True, (72, 2181)),
    ("cg-negated-jacobi", "cg", True, False, True, 0, True, (72,)),
    ("cg-negated-plain", "cg", False, False, True, 0, True, (72,)),  # defsign = -1
    ("cg-poly-fused", "cg", True, False, False, POLY_DEGREE, True, (72, 2181)),
    ("cg-poly-unfused", "cg", True, False, False, POLY_DEGREE, False, (72, 2181)),
)
POLY_WIDTHS = (3, 32)
# Cases with fewer steps than their shape's: (variant, rows, width) -> steps.  In each, one column of the shared right-hand side comes close
# to a breakdown of BiCGStab at the first step left out: the float64 restatement's orders of summation differ so much there that the bound
# of the relative residual would be 1.1 to 350 times the cap of condition 1 (test_iter_steps_host.py shows it for each), and a solve of
# more steps passes through that step; the steps kept are those before it.
LOWERED = {
    ("bicgstab-jacobi", 72, 9): (1, 2), ("bicgstab-jacobi", 72, 16): (1, 2), ("bicgstab-jacobi", 72, 70): (1,),
    ("bicgstab-jacobi", 2181, 33): (1,),
    ("bicgstab-jacobi-trans", 72, 9): (1,), ("bicgstab-jacobi-trans", 72, 17): (1,), ("bicgstab-jacobi-trans", 72, 31): (1,),
    ("bicgstab-jacobi-trans", 72, 70): (1,), ("bicgstab-jacobi-trans", 2181, 33): (1, 2),
}
# mistake -> the smallest cases that can show it (test_iter_steps_host.py: each is rejected there)
CAUGHT_BY = {
    "dot_skips_last_row_of_slab": ("cg-jacobi-m5-w2", "bicgstab-jacobi-m5-w2"),
    "reduce_skips_last_slab": ("cg-jacobi-m2181-w17", "bicgstab-jacobi-m2181-w17"),  # the first shape of more than 16 slabs
    "beta_from_neighbour": ("cg-jacobi-m5-w2", "bicgstab-jacobi-m5-w2"),
    "alpha_from_neighbour": ("cg-jacobi-m5-w2", "bicgstab-jacobi-m5-w2"),
    "p_without_omega_v": ("bicgstab-jacobi-m5-w2", "bicgstab-plain-m5-w2"),
    "x_with_p_not_dinv_p": ("bicgstab-jacobi-m5-w2",),
    "rr_before_omega_t": ("bicgstab-jacobi-m5-w2", "bicgstab-plain-m5-w2"),
    "jacobi_row0_everywhere": ("cg-jacobi-m5-w2", "bicgstab-jacobi-m5-w2"),
}


class Case:
    def __init__(self, variant, m, w, steps):
        self.variant, self.method, self.jacobi, self.trans, self.negated, self.poly, self.fused, _ = variant
        self.m, self.w, self.steps = m, w, tuple(steps)
        self.id = "%s-m%d-w%d" % (self.variant, m, w)

    def matrix(self):
        return matrix(self.method, self.m, self.negated)

    def rhs(self):
        return rhs(self.m, self.w)

    def run(self, dtype=np.float64, order="numpy", bug=None, K=None):
        A, B, K = self.matrix(), self.rhs(), K or max(self.steps)
        chunk = 8 if (bug is None and self.m * self.w > 1 << 20) else None
        if self.method == "cg":
            return cg_steps(A, B, K, self.jacobi, self.trans, dtype, order, poly=self.poly, bug=bug, chunk=chunk)
        return bicgstab_steps(A, B, K, self.jacobi, self.trans, dtype, order, bug=bug, chunk=chunk)


def _cases():
    out = []
    for variant in VARIANTS:
        for m, (widths, steps, _) in SHAPES.items():
            if variant[7] is not None and m not in variant[7]:
                continue
            for w in widths:
                if variant[5] and w not in POLY_WIDTHS:
                    continue
                out.append(Case(variant, m, w, LOWERED.get((variant[0], m, w), steps)))
    return out


CASES = _cases()


def case(case_id):
    return next(c for c in CASES if c.id == case_id)


# ------------------------------------------------------------------------------------------------------------------ the expectation
class Expected:
    """of one case, for every step k of it: x[k] (longdouble), relres[k] (longdouble), the bounds bound_x[k], bound_r[k] per column
    (float64), the float64 restatement's worst errors err_x[k], err_r[k] per column and per order, and the longdouble rr_k / bb"""

    def __init__(self, c):
        ref = c.run(dtype=LD)
        runs = {order: c.run(order=order) for order in ORDERS}
        self.case, self.x, self.relres, self.bound_x, self.bound_r, self.err_x, self.err_r, self.xmax, self.decay = c, {}, {}, {}, {}, {}, {}, {}, {}
        for k in c.steps:
            xl, rl = ref[k - 1][0], ref.relres(k)
            self.x[k], self.relres[k] = xl, rl
            self.xmax[k] = np.abs(xl).max(0).astype(np.float64)
            self.decay[k] = (ref[k - 1][1] / ref.bb).astype(np.float64)
            self.err_x[k] = {o: np.abs(r[k - 1][0] - xl).max(0).astype(np.float64) for o, r in runs.items()}
            self.err_r[k] = {o: np.abs(r.relres(k) - rl).astype(np.float64) for o, r in runs.items()}
            self.bound_x[k] = np.maximum(FLOOR * self.xmax[k], MARGIN * np.max(list(self.err_x[k].values()), axis=0))
            self.bound_r[k] = np.maximum(FLOOR, MARGIN * np.max(list(self.err_r[k].values()), axis=0))

    def ratios(self, k, x, relres):
        """(error / bound of x, of the relative residual), the worst over the columns; NaN counts as outside"""
        ex = np.abs(np.asarray(x) - self.x[k]).max(0).astype(np.float64) / self.bound_x[k]
        er = np.abs(np.asarray(relres) - self.relres[k]).astype(np.float64) / self.bound_r[k]
        worst = lambda v: float("inf") if not np.all(np.isfinite(v)) else float(v.max())
        return worst(ex), worst(er)


_expected, _large = {}, {}


def expected(c):
    """computed once per case; of the cases too large to keep (the longdouble iterates of 131168 x 32) only the last one is kept"""
    if c.id in _expected:
        return _expected[c.id]
    if c.id in _large:
        return _large[c.id]
    e = Expected(c)
    if c.m * c.w > 1 << 20:
        _large.clear()
        _large[c.id] = e
    else:
        _expected[c.id] = e
    return e
