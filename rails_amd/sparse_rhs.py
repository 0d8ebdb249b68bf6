"""The right-hand side B of A X M' + M X A' + B B' = 0 as a sparse m x p matrix on the device (include/rails_hip.h: rails_sprhs_*,
rails_amd/csrc/sprhs.hip): the operator form of the reference's MatrixOrMultiVectorWrapper (src/MatrixOrMultiVectorWrapper.hpp), which
its driver uses (src/main.cpp:67 reads B.mtx as a CrsMatrix, :98 hands it to the solver).  Single GPU only."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check
from .wrappers import HipMultiVectorWrapper, HipOperatorWrapper, _f, _Handle, _p

_i64p, _i32p, _dp = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)


def csr_transpose_host(n_rows, n_cols, rowptr, col, val):
    """rails_csr_transpose_host: the stable transpose of an n_rows x n_cols CSR matrix, on the host.  Returns (rc, t_rowptr, t_col, t_val)."""
    lib = _lib.load()
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
    col = np.ascontiguousarray(col, dtype=np.int32)
    val = np.ascontiguousarray(val, dtype=np.float64)
    assert rowptr.size == n_rows + 1 and col.size == val.size
    t_rowptr = np.zeros(n_cols + 1, dtype=np.int64)
    t_col = np.zeros(col.size, dtype=np.int32)
    t_val = np.zeros(col.size, dtype=np.float64)
    rc = lib.rails_csr_transpose_host(n_rows, n_cols, rowptr.ctypes.data_as(_i64p), col.ctypes.data_as(_i32p), val.ctypes.data_as(_dp),
                                      t_rowptr.ctypes.data_as(_i64p), t_col.ctypes.data_as(_i32p), t_val.ctypes.data_as(_dp))
    return rc, t_rowptr, t_col, t_val


def csr_gram_norm2_host(n_rows, n_cols, csr, t_csr):
    """rails_csr_gram_norm2_host: ||B'B||_F^2 from the CSR triples of B and of its transpose.  Returns (rc, value)."""
    lib = _lib.load()
    a = [np.ascontiguousarray(x, dtype=t) for x, t in zip(tuple(csr) + tuple(t_csr), (np.int64, np.int32, np.float64) * 2)]
    out = C.c_double(-1.0)
    rc = lib.rails_csr_gram_norm2_host(n_rows, n_cols, a[0].ctypes.data_as(_i64p), a[1].ctypes.data_as(_i32p), a[2].ctypes.data_as(_dp),
                                       a[3].ctypes.data_as(_i64p), a[4].ctypes.data_as(_i32p), a[5].ctypes.data_as(_dp), C.byref(out))
    return rc, out.value


class SparseRHS:
    """B (m x p) in CSR, uploaded with its transpose.  `.op` is an operator handle (HipOperatorWrapper) whose products are B X and,
    transposed, B'X; Solver(ctx, A, B) accepts the object in the place of a dense B."""

    def __init__(self, ctx, rowptr, col, val, p):
        self.ctx = ctx
        self.rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
        self.col = np.ascontiguousarray(col, dtype=np.int32)
        self.val = np.ascontiguousarray(val, dtype=np.float64)
        self.m, self.p = self.rowptr.size - 1, int(p)
        h = C.c_void_p()
        check(ctx.lib.rails_sprhs_create(ctx.h, self.m, self.p, self.rowptr.ctypes.data_as(_i64p), self.col.ctypes.data_as(_i32p),
                                         self.val.ctypes.data_as(_dp), C.byref(h)), "rails_sprhs_create")
        self.h = h
        oh = C.c_void_p()
        check(ctx.lib.rails_csr_create_sprhs(ctx.h, h, C.byref(oh)), "rails_csr_create_sprhs")
        self.op = HipOperatorWrapper(ctx, None, None, None, _handle=_Handle(ctx, oh))
        self.op.n_rows, self.op.n_cols = self.m, self.p
        self.op.h._sprhs = self  # the object outlives every copy of the handle

    @classmethod
    def from_scipy(cls, ctx, B):
        """from anything with .tocsr() (duplicates are kept as they are, in their order)"""
        B = B.tocsr()
        return cls(ctx, B.indptr, B.indices, B.data, B.shape[1])

    def M(self):
        return int(self.ctx.lib.rails_sprhs_rows(self.h))

    def N(self):
        return int(self.ctx.lib.rails_sprhs_cols(self.h))

    def nnz(self):
        return int(self.ctx.lib.rails_sprhs_nnz(self.h))

    def gram_norm2(self):
        """||B'B||_F^2, computed on the host when the object was made"""
        return float(self.ctx.lib.rails_sprhs_gram_norm2(self.h))

    def apply(self, X, Y=None, trans=False):
        """Y = B X (X of p rows) or, trans, Y = B'X (X of m rows); a new Y when none is given"""
        if Y is None:
            Y = HipMultiVectorWrapper(self.ctx, self.p if trans else self.m, X.n, capacity=max(1, X.n))
        check(self.ctx.lib.rails_sprhs_apply(self.ctx.h, self.h, 1 if trans else 0, X.panel.h, X.c0, X.n, Y.panel.h, Y.c0), "rails_sprhs_apply")
        return Y

    def toarray(self):
        out = np.zeros((self.m, self.p))
        rows = np.repeat(np.arange(self.m), np.diff(self.rowptr))
        np.add.at(out, (rows, self.col), self.val)
        return out

    def close(self):
        if self.h:
            if self.ctx.h:
                self.op.h._sprhs = None
                self.ctx.lib.rails_csr_destroy(self.op.h.h)
                self.op.h.h = None
                self.ctx.lib.rails_sprhs_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def resid_lanczos_sparse(ctx, AV, V, T, B, max_iter, MV=None):
    """rails_resid_lanczos_sparse: resid_lanczos with B a SparseRHS.  Returns dict(steps, H, eigenvalues, v)."""
    T = _f(T)
    k = AV.n
    H = np.zeros((max_iter + 1, max_iter + 1), order="F")
    steps = C.c_int(0)
    MVp = MV if MV is not None else V
    check(ctx.lib.rails_resid_lanczos_sparse(ctx.h, AV.panel.h, AV.c0, MVp.panel.h, MVp.c0, k, _p(T), max(1, k), B.h, max_iter, _p(H),
                                             max_iter + 1, C.byref(steps)), "rails_resid_lanczos_sparse")
    s = steps.value
    Hs = np.asfortranarray(H[:s, :s].copy())
    w = np.zeros(s)
    info = C.c_int(0)
    ctx.lib.rails_dsyev(b"V", b"U", s, _p(Hs), s, _p(w), C.byref(info))
    return dict(steps=s, H=H, eigenvalues=w, v=Hs)
