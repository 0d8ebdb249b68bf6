"""The solution object X = U S U' (include/rails_solution.h): what a user does with the low-rank solution of the solver -- pointwise
variance diag(X), trace, products, leading eigenpairs (the modes of the covariance and their share of the trace, as the reference's
driver prints them, src/main.cpp:140-170), entries -- with U staying on the device.

    sol = Solution(ctx, V, T)          # from host arrays (or a HipMultiVectorWrapper for V)
    sol = solver.solution()            # from the last solve, no host round trip
    sol = schur.lift(sol)              # the same on all unknowns of a descriptor system (rails_amd/schur.py)
"""
import ctypes as C

import numpy as np

from ._lib import check
from .wrappers import HipMultiVectorWrapper, _f, _p, index_array, index_ptr

_i32p = C.POINTER(C.c_int32)


class Solution:
    def __init__(self, ctx, U=None, S=None, copy=False, _handle=None):
        """U: host array (local rows x k) or a HipMultiVectorWrapper (borrowed unless copy=True); S: k x k symmetric host array"""
        self.ctx, self.lib = ctx, ctx.lib
        self._keep = None
        if _handle is None:
            if not isinstance(U, HipMultiVectorWrapper):
                U = HipMultiVectorWrapper(ctx, data=U)
            S = _f(S)
            if S.shape != (U.n, U.n):
                raise ValueError("S is %d x %d, U has %d columns" % (S.shape[0], S.shape[1], U.n))
            _handle = C.c_void_p()
            check(self.lib.rails_solution_create(ctx.h, U.panel.h, U.c0, U.n, _p(S), max(1, S.shape[0]), 1 if copy else 0, C.byref(_handle)), "rails_solution_create")
            if not copy:
                self._keep = U  # the object borrows the panel
        self.h = _handle
        self.k = self.lib.rails_solution_rank(self.h)
        self.m = self.lib.rails_solution_rows(self.h)
        ctx._solvers.add(self)  # closed before the context

    # ---- the factors ------------------------------------------------------------------------------------------------------------------
    def U(self):
        """the device factor as a (borrowed) HipMultiVectorWrapper view"""
        c0 = C.c_int(0)
        ptr = self.lib.rails_solution_panel(self.h, C.byref(c0))
        v = HipMultiVectorWrapper._borrow(self.ctx, ptr, c0.value, self.k, self.m)
        v._owner = self
        return v

    def S(self):
        return np.ctypeslib.as_array(self.lib.rails_solution_small(self.h), shape=(self.k, self.k)).T.copy(order="F")

    # ---- what one does with X -----------------------------------------------------------------------------------------------------------
    def variance(self, fetch=True):
        """diag(X): one pass over U on the device (rails_panel_rowquad).  fetch=False: the m x 1 device multivector"""
        out = HipMultiVectorWrapper(self.ctx, self.m, 1)
        check(self.lib.rails_solution_variance(self.h, out.panel.h, 0), "rails_solution_variance")
        return out.to_host()[:, 0] if fetch else out

    def trace(self):
        tr = C.c_double(0.0)
        check(self.lib.rails_solution_trace(self.h, C.byref(tr)), "rails_solution_trace")
        return tr.value

    def apply(self, W):
        """X W; W a host array (a host array comes back) or a HipMultiVectorWrapper (a new one comes back)"""
        host = not isinstance(W, HipMultiVectorWrapper)
        Wd = HipMultiVectorWrapper(self.ctx, data=W) if host else W
        Y = HipMultiVectorWrapper(self.ctx, self.m, Wd.n)
        check(self.lib.rails_solution_apply(self.h, Wd.panel.h, Wd.c0, Wd.n, Y.panel.h, 0), "rails_solution_apply")
        return Y.to_host() if host else Y

    def eigs(self, k=0, tol=0.0, fetch=True):
        """the k eigenpairs of largest modulus of X (k <= 0: all), those with |lambda| <= tol max|lambda| dropped; sorted by decreasing
        modulus.  Returns (values, vectors); fetch=False leaves the vectors on the device (HipMultiVectorWrapper)"""
        cap = self.k if (k <= 0 or k > self.k) else k
        values = np.zeros(cap)
        Z = HipMultiVectorWrapper(self.ctx, self.m, cap)
        found = C.c_int(0)
        check(self.lib.rails_solution_eigs(self.h, int(k), float(tol), _p(values), Z.panel.h, C.byref(found)), "rails_solution_eigs")
        Z.n = found.value
        return values[:found.value].copy(), (Z.to_host() if fetch else Z)

    def truncate(self, tol):
        """the same X to relative accuracy tol in an orthonormal basis of its numerical rank: Solution(Z, diag(lambda))"""
        lam, Z = self.eigs(0, tol, fetch=False)
        return Solution(self.ctx, Z, np.diag(lam))

    def block(self, rows, cols=None):
        """X[rows, cols] (local row indices) as a host array"""
        rows = np.ascontiguousarray(rows, dtype=np.int32).ravel()
        cols = rows if cols is None else np.ascontiguousarray(cols, dtype=np.int32).ravel()
        out = np.zeros((rows.size, cols.size), order="F")
        check(self.lib.rails_solution_block(self.h, rows.ctypes.data_as(_i32p), rows.size, cols.ctypes.data_as(_i32p), cols.size, _p(out), max(1, rows.size)),
              "rails_solution_block")
        return out

    def covariance(self, ia, ib=None, fetch=True):
        """X[ia[i], ib[i]] for every pair: local row indices as numpy integer arrays of one length; one of the two may be None = the
        identity (pair i is (ia[i], i), or (i, ib[i])).  One pass over the gathered rows on the device (rails_panel_rowpair), nothing
        of U comes to the host.  fetch=False: the n x 1 device multivector"""
        ia, ib = index_array(ia, self.m, "ia"), index_array(ib, self.m, "ib")
        if ia is None and ib is None:
            raise ValueError("covariance: give ia, ib or both (variance() is the case of neither)")
        if ia is not None and ib is not None and ia.size != ib.size:
            raise ValueError("covariance: %d indices in ia, %d in ib" % (ia.size, ib.size))
        n = (ia if ia is not None else ib).size
        if (ia is None or ib is None) and n > self.m:
            raise ValueError("covariance: a missing index array is the identity, and %d pairs exceed the %d rows" % (n, self.m))
        out = HipMultiVectorWrapper(self.ctx, n, 1)
        check(self.lib.rails_solution_pairs(self.h, index_ptr(ia), index_ptr(ib), n, out.panel.h, 0), "rails_solution_pairs")
        return out.to_host()[:, 0] if fetch else out

    def maps(self, rows, correlation=False, fetch=True):
        """One-point maps: column j is X[:, rows[j]] (or the correlation of every unknown with unknown rows[j]; 0 where a variance is not
        positive, 1 at the unknown itself).  rows: up to 64 LOCAL row indices; on a row partition -1 on every rank but the owner.
        fetch=False: the m x q device multivector"""
        rows = index_array(rows, self.m, "rows", lowest=-1)
        if rows is None or rows.size > 64:
            raise ValueError("maps: between 0 and 64 reference unknowns, got %s" % (None if rows is None else rows.size))
        out = HipMultiVectorWrapper(self.ctx, self.m, rows.size)
        check(self.lib.rails_solution_maps(self.h, index_ptr(rows), rows.size, 1 if correlation else 0, out.panel.h, 0, -1), "rails_solution_maps")
        return out.to_host() if fetch else out

    def std(self, fetch=True):
        """sqrt(diag(X)), the pointwise standard deviation; 0 where the computed variance is not > 0 (the rule of the correlation maps).
        The root is taken on the host; fetch=False uploads it into a new m x 1 device multivector"""
        v = self.variance()
        s = np.sqrt(np.where(v > 0.0, v, 0.0))
        return s if fetch else HipMultiVectorWrapper(self.ctx, data=s.reshape(-1, 1))

    def close(self):
        if self.h:
            if self.ctx.h:
                self.lib.rails_solution_destroy(self.h)
            self.h = None
            self._keep = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
