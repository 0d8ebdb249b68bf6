"""The numpy restatement of the Chebyshev polynomial preconditioner and of conjugate gradients preconditioned with it
(tests/cheb_reference.py): the polynomial against its closed form on the eigenvalues, float64 against longdouble, the solves against
scipy's splu, the iteration counts tests/test_gpu_iter_poly.py leans on, and the choice of the default "poly_ratio".  CPU only."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import cheb_reference as C
import iter_reference as R

TOL = 1e-10


def cheb_t(n, x):
    t0, t1 = np.ones_like(x), x
    if n == 0:
        return t0
    for _ in range(n - 1):
        t0, t1 = t1, 2 * x * t1 - t0
    return t1


@pytest.mark.parametrize("K", [1, 2, 5, 8])
def test_polynomial_is_the_chebyshev_residual_polynomial(K):
    """on the 9 x 8 Laplacian (constant diagonal, so G A is symmetric): G r - G A z = T_{K+1}((theta - G A) / delta) / T_{K+1}(sigma) G r"""
    A = C.problem("lap9x8")
    g = C.g_of(A, True)
    hi, ratio = C.gershgorin(A, g), 30.0
    assert hi == 2.0
    lam, Q = np.linalg.eigh(-0.25 * A.toarray())
    assert lam.min() > 0 and lam.max() < hi
    Rm = R.rhs(A.shape[0], 3)
    Z = C.polynomial(A, Rm, K, hi, ratio, g)
    lo = hi / ratio
    theta, delta = (hi + lo) / 2, (hi - lo) / 2
    factor = cheb_t(K + 1, (theta - lam) / delta) / cheb_t(K + 1, np.array(theta / delta))
    want = Q @ (factor[:, None] * (Q.T @ (g[:, None] * Rm)))
    got = g[:, None] * Rm - g[:, None] * (A @ Z)
    assert np.abs(got - want).max() <= 1e-13 * np.abs(Rm).max()
    # inside [lo, hi] the factor is at most 1 / T_{K+1}(sigma), below lo it lies in (0, 1): p(G A) G A is definite
    assert np.all(factor[lam < lo] > 0) and np.all(factor < 1)


@pytest.mark.parametrize("tag,jacobi", [("lap9x8", True), ("lap9x8", False), ("stencil27", True), ("banded41", True), ("neg_banded41", False), ("one", True)])
def test_float64_against_longdouble(tag, jacobi):
    A = C.problem(tag)
    g = C.g_of(A, jacobi)
    hi = C.gershgorin(A, g)
    Rm = R.rhs(A.shape[0], 3)
    for K in (0, 1, 2, 5):
        Z = C.polynomial(A, Rm, K, hi, 30.0, g)
        Zl = C.polynomial(A, Rm, K, hi, 30.0, g, dtype=np.longdouble)
        assert Zl.dtype == np.longdouble and Z.dtype == np.float64
        err = np.abs(Z - Zl).max(0).astype(float)
        print(tag, jacobi, K, "float64 against longdouble, per column:", err)
        assert np.all(err <= 64 * np.finfo(float).eps * np.abs(Zl).max(0).astype(float))
    # G A has a positive spectrum whatever the sign of A: the polynomial makes a definite preconditioner of A's own sign
    Z = C.polynomial(A, Rm, 5, hi, 30.0, g)
    assert np.all(((Rm * Z).sum(0) > 0) == (A.diagonal()[0] > 0))


# (problem, K, ratio) -> the iteration counts of the two shared columns lie in [lo, hi] (measured with this restatement, some slack for
# another BLAS' order of summation)
COUNTS = {("lap9x8", 0, 30): (36, 40), ("lap9x8", 2, 30): (20, 24), ("lap9x8", 4, 30): (12, 16), ("lap9x8", 2, 10): (15, 17), ("lap9x8", 2, 100): (34, 40),
          ("lap64", 0, 30): (220, 232), ("lap64", 2, 30): (76, 82), ("lap64", 4, 30): (49, 53), ("lap64", 4, 100): (46, 50), ("lap64", 8, 100): (27, 29),
          ("stencil27", 4, 30): (10, 14), ("banded41", 4, 30): (10, 14)}


@pytest.mark.parametrize("tag,K,ratio", sorted(COUNTS))
def test_preconditioned_solves_and_counts(tag, K, ratio):
    A, Bm, X, c = C.reference(tag, 2, K, ratio=float(ratio))
    assert np.all(c.flags == R.CONVERGED), c.flags
    rel = R.true_relres(A, X, Bm)
    print(tag, K, ratio, "iterations", c.iter, "products", C.products(c, K), "true relative residual %.2e" % rel.max())
    assert rel.max() <= 2.0 * TOL
    Xs = spla.splu(sp.csc_matrix(A)).solve(Bm)
    assert (np.linalg.norm(A @ (X - Xs), axis=0) / np.linalg.norm(Bm, axis=0)).max() <= 3.0 * TOL
    lo, hi = COUNTS[(tag, K, ratio)]
    assert lo <= c.iter.min() and c.iter.max() <= hi, (c.iter, lo, hi)


def test_the_point_of_the_polynomial():
    """64 x 64, K = 4, ratio 30: about the same products, about a fifth of the inner products (3 per iteration and column either way)"""
    plain, poly = C.reference("lap64", 2, 0)[3], C.reference("lap64", 2, 4)[3]
    assert poly.iter.max() <= 0.25 * plain.iter.max()
    assert C.products(poly, 4) <= 1.15 * C.products(plain, 0)


def test_negative_definite_without_jacobi_and_a_bound_set_too_low():
    A = C.problem("lap9x8")
    Bm = R.rhs(A.shape[0], 2)
    X, c = C.pcg(A, Bm, 2, ratio=30.0, jacobi=False)  # G = -I
    assert np.all(c.flags == R.CONVERGED) and R.true_relres(A, X, Bm).max() <= 2 * TOL
    # hi a quarter of the Gershgorin bound: above it the residual polynomial T_{K+1} is large with the sign (-1)^(K+1), so an odd K makes
    # an indefinite preconditioner (breakdown in the first iteration: p.Ap and r.z of different signs) and an even K a definite, poor one
    low = 0.25 * C.gershgorin(A, C.g_of(A, True))
    for K in (2, 3):
        X, c = C.pcg(A, Bm, K, ratio=30.0, hi=low)
        print("bound too low, K", K, ": flags", c.flags, "iterations", c.iter)
        assert np.all(c.flags == (R.BREAKDOWN if K == 3 else R.CONVERGED))
        assert np.all(np.isfinite(X))


def test_choice_of_the_default_ratio():
    """the ratio with the smallest worst case of products relative to plain CG.  (The table of DESIGN.md section 15 also has the 128 x 128
    Laplacian; its rows repeat those of 64 x 64 to two digits and it is left out here for the time it takes.)"""
    table, worst = C.ratio_table(tags=("lap9x8", "lap64"))
    print({r: round(w, 2) for r, w in worst.items()})
    assert min(worst, key=worst.get) == 10
    assert table[("lap64", 4, 30)][:2] == (51, 255) or abs(table[("lap64", 4, 30)][0] - 51) <= 2
