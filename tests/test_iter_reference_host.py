"""The numpy restatement of the iterative A^-1 operator (tests/iter_reference.py) against scipy's splu on the problems the GPU tests use,
and the iteration counts those tests depend on (tests/test_gpu_iter.py bounds the device's counts by 1.5 times these).  CPU only."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import iter_reference as R

TOL = 1e-10

# (problem, Jacobi) -> the counts of the three shared columns lie in [lo, hi] (measured with this restatement; a few iterations of slack for
# another BLAS' order of summation)
COUNTS = {
    ("a", True): (113, 117), ("b", True): (116, 122), ("b", False): (1150, 1260), ("c", True): (58, 67), ("c4", True): (105, 121),
    ("c'", True): (55, 69), ("c'", False): (420, 700), ("d", True): (60, 66), ("e", True): (22, 27), ("e", False): (26, 30),
}


@pytest.mark.parametrize("tag,jacobi", sorted(COUNTS))
def test_restatement_solves_and_counts(tag, jacobi):
    A, Bm, X, c = R.reference(tag, 3, jacobi=jacobi)
    assert np.all(c.flags == R.CONVERGED), c.flags
    rel = R.true_relres(A, X, Bm)
    print(tag, jacobi, "iterations", c.iter, "true relative residual %.2e" % rel.max())
    assert rel.max() <= 1.0 * TOL  # the recurrence's residual is the true one to well below the tolerance on these problems
    assert np.all(c.relres() <= TOL)
    Xs = spla.splu(sp.csc_matrix(A)).solve(Bm)
    # against splu's solution without a condition number: A (X - Xs) is the restatement's residual minus splu's, which is at rounding level
    assert (np.linalg.norm(A @ (X - Xs), axis=0) / np.linalg.norm(Bm, axis=0)).max() <= 2.0 * TOL
    lo, hi = COUNTS[(tag, jacobi)]
    assert lo <= c.iter.min() and c.iter.max() <= hi, (c.iter, lo, hi)


def test_jacobi_is_what_keeps_the_scaled_problems_fast():
    """without the preconditioner the scaled problems take many times the iterations: the factor 1.5 of the GPU tests tells a working
    Jacobi path from a missing one"""
    for tag in ("b", "c'"):
        with_j, without = R.reference(tag, 3, jacobi=True)[3].iter, R.reference(tag, 3, jacobi=False)[3].iter
        assert without.min() >= 6 * with_j.max(), (tag, with_j, without)


def test_transposed_bicgstab():
    A, Bm, X, c = R.reference("c", 3, trans=True)
    assert np.all(c.flags == R.CONVERGED)
    Xs = spla.splu(sp.csc_matrix(A.T)).solve(Bm)
    assert (np.linalg.norm(A.T @ (X - Xs), axis=0) / np.linalg.norm(Bm, axis=0)).max() <= 2.0 * TOL
    assert R.true_relres(A, X, Bm, trans=True).max() <= TOL


def test_columns_of_different_speed_and_the_freeze():
    """a random column, a zero column, an eigenvector, a random column in one solve: [~115, 0, 1, ~115]; the frozen columns stay as they
    were while the others go on"""
    A, _ = R.problem("a")
    n = A.shape[0]
    k = int(round(np.sqrt(n)))
    s = np.sin(np.pi * np.arange(1, k + 1) / (k + 1))
    Bm = R.rhs(n, 4)
    Bm[:, 1] = 0.0
    Bm[:, 2] = np.kron(s, s)
    X, c = R.cg(A, Bm, tol=TOL)
    assert c.iter[1] == 0 and c.iter[2] == 1 and 113 <= c.iter[0] <= 117 and 113 <= c.iter[3] <= 117, c.iter
    assert np.all(X[:, 1] == 0.0) and np.all(np.isfinite(X))
    assert np.all(c.flags == R.CONVERGED)
    assert R.true_relres(A, X[:, [0, 2, 3]], Bm[:, [0, 2, 3]]).max() <= TOL
    # stopping the host's loop early and going on changes nothing for a column that had already stopped
    X5, c5 = R.cg(A, Bm, tol=TOL, stop_after=5)
    assert np.array_equal(X5[:, 2], X[:, 2]) and c5.iter[2] == 1


def test_iteration_cap_and_breakdown_rules():
    A, _ = R.problem("a")
    n = A.shape[0]
    Bm = R.rhs(n, 2)
    X, c = R.cg(A, Bm, tol=TOL, maxit=5)
    assert np.all(c.flags == R.MAXIT) and np.all(c.iter == 5)
    # CG on an indefinite diagonal matrix without the preconditioner: p.q < 0 where rho > 0
    d = np.array([2.0] * 10 + [-1.0] * (n - 10))
    b = np.ones((n, 1))
    assert (d * b[:, 0] ** 2).sum() < 0
    X, c = R.cg(sp.diags(d).tocsr(), b, tol=TOL, jacobi=False)
    assert c.flags[0] == R.BREAKDOWN and c.iter[0] == 1 and np.all(X == 0.0)
    X, c = R.cg(sp.diags(d).tocsr(), b, tol=TOL, jacobi=True)
    assert c.flags[0] == R.CONVERGED and c.iter[0] == 1 and np.allclose(X[:, 0], b[:, 0] / d, rtol=1e-15)
    # a NaN right-hand side is flagged at the start and never iterates
    b2 = np.ones((n, 2))
    b2[3, 1] = np.nan
    X, c = R.cg(A, b2, tol=TOL)
    assert c.flags[1] == R.NONFINITE and c.iter[1] == 0 and c.flags[0] == R.CONVERGED
    X, c = R.bicgstab(A, b2, tol=TOL)
    assert c.flags[1] == R.NONFINITE and c.iter[1] == 0 and c.flags[0] == R.CONVERGED
