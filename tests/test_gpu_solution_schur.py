"""SchurOperator.lift: the solution object on all unknowns of a descriptor system, on the reference's application problem (the MOC ocean
model with its border, tests/moc_problem.py; n = 1538).  The solver is stopped by max_trips: the post-processing does not need a
converged (V, T).  The lifted object is the reference's SchurOperator with a solution set (src/SchurOperator.cpp:191-342) in factored
form: its trace is SchurOperator::Trace."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("device_solve", [True, False])
def test_lift_on_the_moc_problem(device_solve):
    import moc_problem

    import rails_amd
    from rails_amd.schur import SchurOperator

    A, mdiag, B = moc_problem.add_border(*moc_problem.load())
    n = A.shape[0]
    assert n == 1538
    ctx = rails_amd.Context(device=0, seed=7)
    schur = SchurOperator(ctx, (A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data.astype(np.float64)), mdiag, tol=1e-12, device_solve=device_solve)
    B2 = schur.restrict(B)
    d2 = schur.mass22
    Mop = rails_amd.HipOperatorWrapper(ctx, np.arange(schur.m2 + 1, dtype=np.int64), np.arange(schur.m2, dtype=np.int32), d2)
    solver = rails_amd.Solver(ctx, schur.op, B2, M=Mop)
    assert solver.set_parameters({"Expand size": 3, "Lanczos iterations": 10, "Tolerance": 1e-8}) == 0
    solver.set_option("verbose", 0)
    solver.set_option("mass", 1)
    solver.set_option("max_trips", 12)
    code, V, T = solver.solve()
    assert code in (0, 2) and V.shape[1] >= 10
    sol = solver.solution()
    full = schur.lift(sol)
    assert (full.m, full.k) == (n, sol.k)
    Vf = schur.prolongate(V)
    Uf = full.U().to_host()
    assert np.abs(Uf - Vf).max() <= 1e-12 * np.abs(Vf).max()
    np.testing.assert_array_equal(Uf[schur.idx2], V)
    X = Vf @ T @ Vf.T
    nX = np.linalg.norm(X, 2)
    assert abs(full.trace() - np.trace(X)) <= 1e-11 * nX
    # the reference's formula, src/SchurOperator.cpp:322-342: trace(T) + trace(T V'A12'A11^-T A11^-1 A12 V) (V orthonormal or not: T V'V)
    Z = schur.lu.solve(np.ascontiguousarray(schur.A12 @ V))
    want = np.trace(T @ (V.T @ V)) + np.trace(T @ (Z.T @ Z))
    assert abs(full.trace() - want) <= 1e-11 * nX
    assert np.abs(full.variance() - np.diag(X)).max() <= 1e-11 * nX
    w = np.linalg.eigvalsh(X)
    w = w[np.argsort(-np.abs(w))][:10]
    lam, Zv = full.eigs(10)
    print("lift (%s solve): |U - prolongate| %.2e, eigenvalue error %.2e |X|, residual %.2e |X|" % ("device" if device_solve else "host", np.abs(Uf - Vf).max() / np.abs(Vf).max(),
                                                                                                 np.abs(lam - w).max() / nX, np.linalg.norm(X @ Zv - Zv * lam, axis=0).max() / nX))
    assert np.abs(lam - w).max() <= 1e-11 * nX
    assert np.linalg.norm(X @ Zv - Zv * lam, axis=0).max() <= 1e-11 * nX
    with pytest.raises(ValueError):
        schur.lift(full)  # not a solution on the Schur rows
    full.close()
    sol.close()
    solver.close()
    ctx.close()
