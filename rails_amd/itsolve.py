"""Iterative solves on the device as a library object (include/rails_hip.h: rails_iter_*, rails_amd/csrc/itsolve.hip with iter_setup.hip and
iter_hierarchy.hip): the approximate A^-1
the reference allows for its inverse and extended Krylov projections (opts.Ainv of matlab/RAILSsolver.m:19-23, "This can be approximate")
where a sparse LU is latency-bound or cannot be formed.  Conjugate gradients for a definite matrix, BiCGStab for a general one, Jacobi
preconditioning, for conjugate gradients also a Chebyshev polynomial in the Jacobi-scaled matrix; every column is a system of its own and
all scalars stay on the device."""
import ctypes as C

import numpy as np

from ._lib import check
from .wrappers import HipMultiVectorWrapper, HipOperatorWrapper, _Handle

_dp, _i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)

METHODS = {"cg": 1, "bicgstab": 2}
FLAGS = {"active": 1, "converged": 2, "max_iterations": 4, "breakdown": 8, "nonfinite": 16}
ENOCONV = -7


class IterativeInverse:
    """A^-1 by iteration.

    A: a scipy sparse matrix, a (rowptr, col, val) CSR triple of a square matrix, or an operator wrapper (HipOperatorWrapper: a CSR
    operator, a callback operator such as SchurOperator.op).  method: "cg", "bicgstab" or "auto" -- conjugate gradients when a matrix
    equals its transpose, BiCGStab otherwise; for an operator wrapper the caller names the method.  diag: the diagonal for the Jacobi
    preconditioner when A is an operator that is not a CSR matrix (None: the CSR diagonal where there is one).  `.op` is an operator handle
    (HipOperatorWrapper) whose products are the solves: it goes wherever an operator goes (Solver.set_inverse, rails_spmm).
    poly_degree K > 0 (conjugate gradients only): precondition with the Chebyshev polynomial z = p_K(G A) G r, K products per application
    and no inner product between them, fitted to [hi / poly_ratio, hi]; hi is eig_max, or (None) a Gershgorin bound from the CSR arrays --
    an operator that is not a CSR matrix needs eig_max.  poly_ratio None: the library's default.
    amg=True (conjugate gradients on a CSR matrix, one GPU, not together with poly_degree): precondition with one V-cycle of
    smoothed-aggregation multigrid, whose iteration count does not grow with the grid: Chebyshev smoothing of degree amg_degree (1) on
    [hi / amg_ratio, hi] (4) per level, strength threshold amg_theta (0.08), levels until at most amg_coarse (256) rows are left, which
    are inverted densely.  None: the library's defaults.  The hierarchy is built by the first solve, or by amg_setup().
    block_jacobi (both methods, one GPU, not together with poly_degree or amg): precondition with the inverses of the b x b diagonal
    blocks instead of the diagonal's, for a matrix with b unknowns per cell whose coupling inside a cell is the stiff part.  True: the
    blocks of the operator -- a block-CSR operator's own, or for a CSR operator those of block_size=b; an array of shape (m / b, b, b):
    these blocks (any operator).  See block_jacobi().
    block_amg=True (conjugate gradients on a block-CSR operator, one GPU, not together with poly_degree, amg or block_jacobi):
    precondition with one V-cycle of smoothed aggregation on the cells, G the inverses of the diagonal blocks of every level; amg_degree,
    amg_ratio, amg_theta and amg_coarse serve it as they serve amg.  The hierarchy is built by the first solve, or by block_amg_setup().

    On a row-partitioned context (Context.set_partition with more than one rank) A is the rank's operator wrapper with its halo plan set,
    the all-reduce hook or the communicator is installed before the object is made, and making it, set(), solve() and precondition() are
    collective calls: every rank makes them in the same order with the same widths and settings.  The matrix forms are refused there
    (ValueError), and so is trans=True (the transposed product of a row block is single GPU)."""

    def __init__(self, ctx, A, method="auto", tol=1e-10, maxit=1000, jacobi=True, strict=False, diag=None, check_every=None, poly_degree=0,
                 poly_ratio=None, eig_max=None, amg=False, amg_degree=None, amg_ratio=None, amg_theta=None, amg_coarse=None, block_jacobi=False,
                 block_size=0, block_amg=False):
        self.ctx = ctx
        self._owned = None
        if isinstance(A, HipOperatorWrapper):
            if method == "auto":
                raise ValueError("IterativeInverse: name the method ('cg' or 'bicgstab') for an operator wrapper")
            if A.trans:
                raise ValueError("IterativeInverse: pass the operator itself and solve with trans=True")
            self.A = A
        else:
            if getattr(ctx, "nranks", 1) > 1:
                raise ValueError("IterativeInverse: the context is row-partitioned (%d ranks): pass the rank's operator wrapper, the one with its halo "
                                 "plan (HipOperatorWrapper.set_halo), and name the method" % ctx.nranks)
            import scipy.sparse as sp

            if isinstance(A, tuple):
                rowptr, col, val = A
                n = len(rowptr) - 1
                A = sp.csr_matrix((val, col, rowptr), shape=(n, n))
            A = sp.csr_matrix(A)
            if A.shape[0] != A.shape[1]:
                raise ValueError("IterativeInverse: A is %d x %d" % A.shape)
            A.sort_indices()
            if method == "auto":
                method = "cg" if (A != A.T).nnz == 0 else "bicgstab"
            self.A = self._owned = HipOperatorWrapper(ctx, A.indptr, A.indices, A.data)
        if method not in METHODS:
            raise ValueError("IterativeInverse: no method %r (cg, bicgstab, auto)" % (method,))
        self.method = method
        self.m = self.n = int(self.A.M())
        if block_jacobi is True and not block_size and self.A.block_size == 1:  # (b = 0 without blocks is the clearing call there)
            raise ValueError("IterativeInverse: block_jacobi=True on an operator that is not block-CSR needs block_size=b (2 .. 8), or pass the blocks")
        d = None if diag is None else np.ascontiguousarray(diag, dtype=np.float64)
        if d is not None and d.size != self.m:
            raise ValueError("IterativeInverse: the diagonal has %d entries, the operator %d rows" % (d.size, self.m))
        h = C.c_void_p()
        check(ctx.lib.rails_iter_create(ctx.h, self.A.h.h, METHODS[method], d.ctypes.data_as(_dp) if d is not None else None, C.byref(h)), "rails_iter_create")
        self.h = h
        self.set("tolerance", tol)
        self.set("max_iterations", maxit)
        self.set("jacobi", 1 if jacobi else 0)
        self.set("strict", 1 if strict else 0)
        if check_every is not None:
            self.set("check_every", check_every)
        if poly_ratio is not None:
            self.set("poly_ratio", poly_ratio)
        if eig_max is not None:
            self.set("eig_max", eig_max)
        if poly_degree:
            self.set("poly_degree", poly_degree)
        for name, value in (("amg_degree", amg_degree), ("amg_ratio", amg_ratio), ("amg_theta", amg_theta), ("amg_coarse", amg_coarse)):
            if value is not None:
                self.set(name, value)
        if amg:
            self.set("amg", 1)
        if block_jacobi is True:
            self.block_jacobi(b=block_size)
        elif block_jacobi is not False and block_jacobi is not None:
            self.block_jacobi(block_jacobi, b=block_size)
        if block_amg:
            self.set("block_amg", 1)
        oh = C.c_void_p()
        check(ctx.lib.rails_csr_create_iter(ctx.h, h, C.byref(oh)), "rails_csr_create_iter")
        self.op = HipOperatorWrapper(ctx, None, None, None, _handle=_Handle(ctx, oh))
        self.op.h._iter = self  # the solve object (and the operator it iterates on) outlives every copy of the handle

    def set(self, name, value):
        """"tolerance", "max_iterations", "jacobi", "check_every", "strict"; the polynomial preconditioner: "poly_degree" (0 .. 64, 0 is
        off; conjugate gradients only), "poly_ratio" (hi / lo of its interval, above 1), "eig_max" (hi; 0: the Gershgorin bound),
        "poly_fused" (0: never the fused step kernel); the multigrid preconditioner: "amg" (1: on), "amg_degree" (0 .. 8), "amg_ratio"
        (above 1), "amg_theta" (in [0, 1)), "amg_coarse" (1 .. 1024); "block_jacobi" (1: the installed diagonal blocks precondition, 0: "jacobi"
        decides again; block_jacobi() installs them); "block_amg" (1: the block multigrid cycle, with the "amg_..." settings) (rails_iter_set)"""
        check(self.ctx.lib.rails_iter_set(self.h, name.encode(), float(value)), "rails_iter_set")

    def solve(self, X, Y=None, trans=False):
        """Y = A^-1 X (trans: A^-T X; CG ignores it) for a HipMultiVectorWrapper X of m rows (a new one when Y is None); X is left
        unchanged.  Columns that did not converge are flagged (columns()); with strict=True they raise."""
        if Y is None:
            Y = HipMultiVectorWrapper(self.ctx, self.m, X.n)
        assert Y.n == X.n
        check(self.ctx.lib.rails_iter_solve(self.ctx.h, self.h, 1 if trans else 0, X.panel.h, X.c0, X.n, Y.panel.h, Y.c0), "rails_iter_solve")
        return Y

    def precondition(self, X, Y=None):
        """Y = p_K(G A) G X, the preconditioner of the solve on its own (K = poly_degree; 0: G X, G the inverse diagonal or with block_jacobi
        on the inverse diagonal blocks; with amg on: one V-cycle), for a
        HipMultiVectorWrapper X of m rows (a new Y when None).  Queues its work and does not synchronise."""
        if Y is None:
            Y = HipMultiVectorWrapper(self.ctx, self.m, X.n)
        assert Y.n == X.n
        check(self.ctx.lib.rails_iter_precondition(self.ctx.h, self.h, X.panel.h, X.c0, X.n, Y.panel.h, Y.c0), "rails_iter_precondition")
        return Y

    def block_jacobi(self, blocks=None, b=0):
        """installs the block-Jacobi preconditioner and turns it on (rails_iter_block_jacobi).  blocks: the m / b diagonal blocks, shape
        (m / b, b, b) -- the library inverts them; None: those of the operator, a block-CSR operator's own (b 0 or its block size) or a
        CSR operator's for the block size b.  None with b = 0 on any other operator clears the blocks.  Returns block_jacobi_info()."""
        ptr = None
        if blocks is not None:
            blocks = np.ascontiguousarray(blocks, dtype=np.float64)
            if blocks.ndim != 3 or blocks.shape[1] != blocks.shape[2] or (b and b != blocks.shape[1]) or blocks.shape[0] * blocks.shape[1] != self.m:
                raise ValueError("IterativeInverse.block_jacobi: blocks of shape %s for %d rows and b = %d: (m / b, b, b) is wanted" % (blocks.shape, self.m, b))
            b = blocks.shape[1]
            ptr = blocks.ctypes.data_as(_dp)
        check(self.ctx.lib.rails_iter_block_jacobi(self.ctx.h, self.h, int(b), ptr), "rails_iter_block_jacobi")
        return self.block_jacobi_info()

    def block_jacobi_info(self):
        """{"blocks": how many diagonal blocks are installed (0: none), "b": their size, "inverse": their inverses exactly as the kernels
        read them, shape (blocks, b, b)} (rails_iter_block_jacobi_info)"""
        b = C.c_int(0)
        n = self.ctx.lib.rails_iter_block_jacobi_info(self.h, C.byref(b), None, 0)
        check(min(n, 0), "rails_iter_block_jacobi_info")
        inv = np.zeros((n, b.value, b.value))
        if n:
            self.ctx.lib.rails_iter_block_jacobi_info(self.h, C.byref(b), inv.ctypes.data_as(_dp), n)
        return {"blocks": int(n), "b": int(b.value), "inverse": inv}

    def amg_setup(self):
        """builds (or rebuilds) the multigrid hierarchy now and uploads it (rails_iter_amg_setup); returns amg_info()"""
        check(self.ctx.lib.rails_iter_amg_setup(self.ctx.h, self.h), "rails_iter_amg_setup")
        return self.amg_info()

    def block_amg_setup(self):
        """builds (or rebuilds) the block multigrid hierarchy now and uploads it (rails_iter_block_amg_setup); returns block_amg_info()"""
        check(self.ctx.lib.rails_iter_block_amg_setup(self.ctx.h, self.h), "rails_iter_block_amg_setup")
        return self.block_amg_info()

    def block_amg_info(self):
        """amg_info() of the block hierarchy (rails_iter_block_amg_info): "nnz" counts scalar entries, "hi" is the bound on G A"""
        return self._hierarchy_info(self.ctx.lib.rails_iter_block_amg_info, "rails_iter_block_amg_info")

    def amg_info(self):
        """the hierarchy and the last call (rails_iter_amg_info): "levels" (matrices, the dense last one included; 0: none built), per
        matrix "rows", "nnz" and "hi", "operator_complexity", the last call's "cycles", "cycle_products" and "cycle_launches", and the
        "host_seconds" and "upload_seconds" of the set-up"""
        return self._hierarchy_info(self.ctx.lib.rails_iter_amg_info, "rails_iter_amg_info")

    def _hierarchy_info(self, fn, who):
        cap = 20
        rows, nnz, hi = (C.c_int64 * cap)(), (C.c_int64 * cap)(), (C.c_double * cap)()
        n = fn(self.h, rows, nnz, hi, cap)
        check(min(n, 0), who)
        if n == 0:
            return {"levels": 0, "rows": [], "nnz": [], "hi": [], "operator_complexity": 0.0, "cycles": 0, "cycle_products": 0, "cycle_launches": 0,
                    "host_seconds": 0.0, "upload_seconds": 0.0}
        return {"levels": n, "rows": list(rows[:n]), "nnz": list(nnz[:n]), "hi": list(hi[:n]), "operator_complexity": hi[n + 1], "cycles": int(rows[n]),
                "cycle_products": int(nnz[n]), "cycle_launches": int(hi[n]), "host_seconds": rows[n + 1] * 1e-6, "upload_seconds": nnz[n + 1] * 1e-6}

    def solve_host(self, X, trans=False):
        """the same on a host array (m x nc): upload, solve, download"""
        X = np.asarray(X, dtype=np.float64)
        X2 = X.reshape(X.shape[0], -1)
        return self.solve(HipMultiVectorWrapper(self.ctx, data=X2), trans=trans).to_host().reshape(X.shape)

    def stats(self):
        """the last solve and the totals since creation (rails_iter_stats)"""
        info = (C.c_double * 19)()
        k = self.ctx.lib.rails_iter_stats(self.h, info, 19)
        names = ("max_iterations_of_a_column", "inner_products", "launches", "unconverged_columns", "breakdown_columns", "worst_relative_residual",
                 "workspace_columns", "products", "total_solves", "total_columns", "total_iterations", "total_flagged_columns", "total_products",
                 "poly_applications", "fused_launches", "eig_hi", "eig_lo", "allreduces", "halo_exchanges")
        out = {names[i]: info[i] for i in range(max(k, 0))}
        return {n: (v if n in ("worst_relative_residual", "eig_hi", "eig_lo") else int(v)) for n, v in out.items()}

    def columns(self):
        """per column of the last solve: (iterations, relative residual of the recurrence, flags -- FLAGS)"""
        n = self.ctx.lib.rails_iter_columns(self.h, None, None, None, 0)
        it, rel, fl = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1)), np.zeros(max(n, 1), dtype=np.int32)
        self.ctx.lib.rails_iter_columns(self.h, it.ctypes.data_as(_i32p), rel.ctypes.data_as(_dp), fl.ctypes.data_as(_i32p), n)
        return it[:n], rel[:n], fl[:n]

    def close(self):
        if self.h:
            if self.ctx.h:
                self.op.h._iter = None
                self.ctx.lib.rails_csr_destroy(self.op.h.h)
                self.op.h.h = None
                self.ctx.lib.rails_iter_destroy(self.h)
            self.h = None
            self._owned = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
