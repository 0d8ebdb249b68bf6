"""Sparse LU solves on the device as a library object (include/rails_hip.h: rails_lu_*, rails_amd/csrc/splu.hip): the A^-1 of RAILS'
inverse and extended Krylov projections ("Projection method", opts.Ainv of matlab/RAILSsolver.m:7-24) and the Sinv of a Schur
complement (matlab/RAILSschur.m:60-64).  The factorisation runs once on the host (scipy's SuperLU, as rails_amd/schur.py uses it);
every solve runs on the device."""
import ctypes as C

import numpy as np

from ._lib import check
from .wrappers import HipMultiVectorWrapper, HipOperatorWrapper, _Handle

_i64p, _i32p, _dp = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)


class SparseLU:
    """A^-1 (or, with `rows`, x -> (A^-1 E x)[rows], E putting x on those rows and zeros elsewhere) from splu(A).

    A: scipy sparse matrix or a (rowptr, col, val) CSR triple of a square matrix.  `.op` is an operator handle (HipOperatorWrapper)
    whose products are the solves: it goes wherever an operator goes (Solver.set_inverse, rails_spmm, both transposes)."""

    def __init__(self, ctx, A, rows=None, lu=None):
        import scipy.sparse as sp
        import scipy.sparse.linalg as spla

        self.ctx = ctx
        if isinstance(A, tuple):
            rowptr, col, val = A
            n = len(rowptr) - 1
            A = sp.csr_matrix((val, col, rowptr), shape=(n, n))
        self.n = A.shape[0]
        self.lu = lu if lu is not None else spla.splu(sp.csc_matrix(A))
        L, U = sp.csr_matrix(self.lu.L), sp.csr_matrix(self.lu.U)
        arrays = []
        for M in (L, U):
            M.sort_indices()
            arrays += [np.ascontiguousarray(M.indptr, dtype=np.int64), np.ascontiguousarray(M.indices, dtype=np.int32),
                       np.ascontiguousarray(M.data, dtype=np.float64)]
        pr = np.ascontiguousarray(self.lu.perm_r, dtype=np.int32)
        pc = np.ascontiguousarray(self.lu.perm_c, dtype=np.int32)
        self.rows = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
        self.m = self.n if rows is None else self.rows.size
        self._keep = arrays + [pr, pc, self.rows]
        h = C.c_void_p()
        ptr = lambda a, t: a.ctypes.data_as(t) if a is not None else None
        check(ctx.lib.rails_lu_create(ctx.h, self.n, ptr(arrays[0], _i64p), ptr(arrays[1], _i32p), ptr(arrays[2], _dp), ptr(arrays[3], _i64p),
                                      ptr(arrays[4], _i32p), ptr(arrays[5], _dp), ptr(pr, _i32p), ptr(pc, _i32p), ptr(self.rows, _i32p), self.m,
                                      C.byref(h)), "rails_lu_create")
        self.h = h
        oh = C.c_void_p()
        check(ctx.lib.rails_csr_create_lu(ctx.h, h, C.byref(oh)), "rails_csr_create_lu")
        self.op = HipOperatorWrapper(ctx, None, None, None, _handle=_Handle(ctx, oh))
        self.op.h._lu = self  # the solve object outlives every copy of the handle
        self.nnz = int(L.nnz - self.n + U.nnz)

    def solve(self, X, Y=None, trans=False):
        """Y = A^-1 X (trans: A^-T X) for a HipMultiVectorWrapper X of m rows (a new one when Y is None); X is left unchanged."""
        if Y is None:
            Y = HipMultiVectorWrapper(self.ctx, self.m, X.n)
        assert Y.n == X.n
        check(self.ctx.lib.rails_lu_solve(self.ctx.h, self.h, 1 if trans else 0, X.panel.h, X.c0, X.n, Y.panel.h, Y.c0), "rails_lu_solve")
        return Y

    def solve_host(self, X, trans=False):
        """the same on a host array (m x nc): upload, solve, download"""
        X = np.asarray(X, dtype=np.float64)
        X2 = X.reshape(X.shape[0], -1)
        return self.solve(HipMultiVectorWrapper(self.ctx, data=X2), trans=trans).to_host().reshape(X.shape)

    def stats(self):
        """levels of each triangle, nonzeros, launches of the last solve (rails_lu_stats)"""
        info = (C.c_int64 * 10)()
        k = self.ctx.lib.rails_lu_stats(self.h, info, 10)
        names = ("levels_L", "levels_U", "levels_Ut", "levels_Lt", "nnz_L", "nnz_U", "launches", "n", "m", "workspace_columns")
        return {names[i]: int(info[i]) for i in range(max(k, 0))}

    def close(self):
        if self.h:
            if self.ctx.h:
                self.op.h._lu = None
                self.ctx.lib.rails_csr_destroy(self.op.h.h)
                self.op.h.h = None
                self.ctx.lib.rails_lu_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
