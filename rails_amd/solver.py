"""Python mirror of the reference's solver interface (src/LyapunovSolverDecl.hpp:13-35) over the C ABI of
include/rails_solver.h: `Solver(A, B, M)`, `set_parameters(dict)`, `solve(V0=None)` -> (code, V, T).

Parameter names and defaults are the reference's (src/LyapunovSolver.hpp:27-36,76-87); return codes too
(0 converged, -1 not converged, 1 loop exhausted; 2 = stopped by the max_trips extension)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check
from ._solver_sigs import TRIP_FN
from .wrappers import HipOperatorWrapper, _f, _p


class Solver:
    def __init__(self, ctx, A, B, M=None, m_global=None):
        """A, M: HipOperatorWrapper (M None = identity).  B: host array, local rows x p; or a rails_amd.SparseRHS, or anything with
        .tocsr() (a scipy sparse matrix), which is kept sparse (include/rails_solver.h: rails_solver_create_sparse; single GPU, direct
        back end)."""
        from .sparse_rhs import SparseRHS

        self.ctx = ctx
        self.lib = ctx.lib
        self.A, self.M = A, M
        h = C.c_void_p()
        if not isinstance(B, SparseRHS) and hasattr(B, "tocsr"):
            B = SparseRHS.from_scipy(ctx, B)
        if isinstance(B, SparseRHS):
            self.B = B  # the object must live as long as the solver uses it
            self.m_local, self.p = B.m, B.p
            check(self.lib.rails_solver_create_sparse(ctx.h, A.h.h, M.h.h if M is not None else None, B.h, m_global if m_global is not None else -1,
                                                      C.byref(h)), "rails_solver_create_sparse")
        else:
            B = _f(B)
            self.m_local, self.p = B.shape
            check(self.lib.rails_solver_create(ctx.h, A.h.h, M.h.h if M is not None else None, _p(B), B.shape[0], B.shape[1],
                                               m_global if m_global is not None else -1, C.byref(h)), "rails_solver_create")
        self.h = h
        self._cb = None
        self.k = 0
        ctx._solvers.add(self)

    def set_parameters(self, params):
        for name, value in params.items():
            check(self.lib.rails_solver_set_parameter(self.h, name.encode(), float(value)), "rails_solver_set_parameter")
        code = C.c_int(0)
        check(self.lib.rails_solver_apply_parameters(self.h, C.byref(code)), "rails_solver_apply_parameters")
        return code.value

    def set_option(self, name, value):
        check(self.lib.rails_solver_set_option(self.h, name.encode(), float(value)), "rails_solver_set_option")

    def set_inverse(self, op):
        """opts.Ainv of matlab/RAILSsolver.m:18-22 for the "Projection method" parameter (1.1 .. 2.3): any operator of A's row count --
        a SparseLU's .op, a SchurOperator.inverse(), a HipOperatorWrapper (the object itself may be passed when it has an .op)."""
        op = getattr(op, "op", op)
        check(self.lib.rails_solver_set_inverse(self.h, op.h.h), "rails_solver_set_inverse")
        self._inverse = op  # the handle must live as long as the solver uses it

    def set_nullspace(self, N):
        """opts.nullspace of matlab/RAILSsolver.m:33-34,221-222,538-616: N (numpy, the local rows x q) spans a space projected out of
        every space that joins V (the known kernel of a singular A).  None clears it.  See include/rails_solver.h."""
        if N is None:
            check(self.lib.rails_solver_set_nullspace(self.h, None, max(1, self.m_local), 0), "rails_solver_set_nullspace")
            return
        N = _f(N)
        if N.shape[0] != self.m_local:
            raise ValueError("the nullspace has %d rows, the solver %d local rows" % (N.shape[0], self.m_local))
        check(self.lib.rails_solver_set_nullspace(self.h, _p(N), max(1, N.shape[0]), N.shape[1]), "rails_solver_set_nullspace")

    @property
    def nullspace_rank(self):
        """columns of the nullspace the last solve kept after orthonormalisation (0 without one)"""
        return self.lib.rails_solver_nullspace_rank(self.h)

    def set_start_space(self, X):
        """opts.space of matlab/RAILSsolver.m:25-28: the columns of X -- a HipMultiVectorWrapper, a Solution (its device factor, no host
        round trip) or a host array (uploaded once) -- become the start space of the next solve.  They need not be orthonormal or
        independent; the solve orthonormalises them, drops dependent columns and projects the nullspace out.  The next solve is a warm
        start whatever "Restart from solution" says, and consumes the space.  See include/rails_solver.h."""
        from .solution import Solution
        from .wrappers import HipMultiVectorWrapper

        if isinstance(X, Solution):
            c0 = C.c_int(0)
            panel = self.lib.rails_solution_panel(X.h, C.byref(c0))
            c0, k = c0.value, self.lib.rails_solution_rank(X.h)
        else:
            if not isinstance(X, HipMultiVectorWrapper):
                X = HipMultiVectorWrapper(self.ctx, data=X)
            panel, c0, k = X.panel.h, X.c0, X.n
        check(self.lib.rails_solver_set_start_space(self.h, panel, c0, k), "rails_solver_set_start_space")

    @property
    def start_rank(self):
        """columns the last solve kept of its start space (1 after a cold start)"""
        return self.lib.rails_solver_start_rank(self.h)

    def set_trip_callback(self, fn):
        if fn is None:
            self._cb = None
            check(self.lib.rails_solver_set_trip_callback(self.h, TRIP_FN(0), None), "rails_solver_set_trip_callback")
            return

        def tramp(user, trip):
            try:
                fn(trip)
            except Exception:
                import traceback
                traceback.print_exc()
        self._cb = TRIP_FN(tramp)
        check(self.lib.rails_solver_set_trip_callback(self.h, self._cb, None), "rails_solver_set_trip_callback")

    def solve(self, V0=None, fetch=True):
        if V0 is not None:
            V0 = _f(V0)
            check(self.lib.rails_solver_set_V(self.h, _p(V0), V0.shape[0], V0.shape[1]), "rails_solver_set_V")
        code, k = C.c_int(0), C.c_int(0)
        check(self.lib.rails_solver_solve(self.h, C.byref(code), C.byref(k)), "rails_solver_solve")
        self.k = k.value
        if not fetch:
            return code.value, None, None
        return code.value, self.V(), self.T()

    def V(self):
        V = np.zeros((self.m_local, self.k), order="F")
        check(self.lib.rails_solver_get_V(self.h, _p(V), max(1, self.m_local)), "rails_solver_get_V")
        return V

    def T(self):
        T = np.zeros((self.k, self.k), order="F")
        check(self.lib.rails_solver_get_T(self.h, _p(T), max(1, self.k)), "rails_solver_get_T")
        return T

    def solution(self):
        """the solution object X = V T V' of the last solve (rails_amd.Solution): a device copy of V, no host round trip"""
        from .solution import Solution

        h = C.c_void_p()
        check(self.lib.rails_solution_from_solver(self.h, C.byref(h)), "rails_solution_from_solver")
        return Solution(self.ctx, _handle=h)

    def trips(self):
        return self.lib.rails_solver_trips(self.h)

    def scale(self):
        """||B||_2^2 as the last solve computed it (the scale of the stopping test), on either back end; 0 before the first solve"""
        out = C.c_double(0.0)
        check(self.lib.rails_solver_scale(self.h, C.byref(out)), "rails_solver_scale")
        return out.value

    def history(self):
        n = self.trips()
        out = np.zeros(max(n, 1))
        self.lib.rails_solver_history(self.h, _p(out), out.size)
        return out[:n]

    def profile(self):
        """Host wall-clock seconds per solver section of the last solve (reference's profile section names)."""
        import json
        buf = C.create_string_buffer(4096)
        check(self.lib.rails_solver_profile(self.h, buf, 4096), "rails_solver_profile")
        return json.loads(buf.value.decode())

    def relative_residual(self):
        """||A X M' + M X A' + B B'||_F / ||B B'||_F from Gram products on the device; bottoms out near 1e-8 (include/rails_solver.h)"""
        rel = C.c_double(0.0)
        check(self.lib.rails_solver_relative_residual(self.h, C.byref(rel)), "rails_solver_relative_residual")
        return rel.value

    def backend_stats(self):
        """counters of the coordinate-space back end for the last solve ({} when the direct back end ran)"""
        import json

        return json.loads(self.lib.rails_solver_backend_stats(self.h).decode())

    def close(self):
        if self.h:
            if self.ctx.h:  # after the context is gone the handle cannot be released safely any more
                self.lib.rails_solver_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
