"""The solution object X = U S U' on the device (include/rails_solution.h, rails_amd/solution.py): the one-pass kernel
rails_panel_rowquad = diag(U S U') against numpy, and trace / apply / block / eigs of the object against dense algebra.

Kernel bound, componentwise and derived, not tuned: out_i is an inner product of 2k terms (k for a row of U S, k for the reduction
against the row of U), so its rounding error is at most gamma_2k (|U||S||U|')_ii with gamma_n = n eps / (1 - n eps) whatever the order of
summation; 8 k eps leaves a factor 4 for the MFMA's internal summation order and the reference value's own error.

Object bound: eigenvalues within 1e-11 max|lambda| and residuals within 1e-11 |X|_2, the bound this project uses for device
orthogonalisation against the oracle (tests/test_gpu_kernels.py).  U has condition about 1e2; test_object_bound_holds_for_numpy_on_the_host
(no GPU) confirms that the same computation in numpy -- QR, then a small symmetric eigensolve -- stays inside it for the chosen seed."""
import ctypes as C

import numpy as np
import pytest

EPS = 2.0 ** -52


def _object_problem(deficient=False):
    g = np.random.default_rng(41)
    m, k = 1500, 40
    Q1 = np.linalg.qr(g.standard_normal((m, k)))[0]
    Q2 = np.linalg.qr(g.standard_normal((k, k)))[0]
    U = (Q1 * np.logspace(0, 2, k)) @ Q2.T  # singular values 1 .. 100: condition 1e2, not orthonormal
    if deficient:
        U[:, 11] = U[:, 2]
        U[:, 30] = U[:, 5] - 2.0 * U[:, 6]
    S = g.standard_normal((k, k))
    S = S + S.T
    return U, S


def test_object_bound_holds_for_numpy_on_the_host():
    U, S = _object_problem()
    X = U @ S @ U.T
    Q, R = np.linalg.qr(U)
    M = R @ S @ R.T
    lam, Zs = np.linalg.eigh((M + M.T) / 2)
    Z = Q @ Zs
    w = np.linalg.eigvalsh(X)
    big = np.sort(np.abs(w))[::-1][:U.shape[1]]
    nX = np.linalg.norm(X, 2)
    assert np.linalg.cond(U) < 1.1e2
    assert np.abs(np.sort(np.abs(lam))[::-1] - big).max() <= 1e-11 * big[0]
    assert np.linalg.norm(X @ Z - Z * lam, axis=0).max() <= 1e-11 * nX
    assert np.abs(Z.T @ Z - np.eye(Z.shape[1])).max() <= 1e-11


def _kernel_case(g, m, k):
    U = g.standard_normal((m, k)) * 10.0 ** g.uniform(-3, 3, (m, 1))  # rows scaled over six decades
    S = g.standard_normal((k, k))
    S = S + S.T  # symmetric indefinite
    return U, S


@pytest.mark.gpu
@pytest.mark.parametrize("m,k", [(1, 1), (17, 5), (1000, 16), (4099, 33), (20000, 128), (3000, 500)])
def test_rowquad_against_einsum(m, k):
    import rails_amd
    from rails_amd.wrappers import HipMultiVectorWrapper as MV, _p

    ctx = rails_amd.Context(device=0, seed=1)
    U, S = _kernel_case(np.random.default_rng(1000 * k + m), m, k)
    want = np.einsum("ij,jl,il->i", U, S, U)
    bound = 8 * k * EPS * np.einsum("ij,jl,il->i", np.abs(U), np.abs(S), np.abs(U))
    Ud, out = MV(ctx, data=U), MV(ctx, m, 1)
    before = ctx.stats()["rowquad"]
    rails_amd._lib.check(ctx.lib.rails_panel_rowquad(ctx.h, Ud.panel.h, 0, k, _p(np.asfortranarray(S)), k, out.panel.h, 0), "rails_panel_rowquad")
    got = out.to_host()[:, 0]
    assert ctx.stats()["rowquad"] == before + 1
    ratio = np.abs(got - want) / bound
    print("m = %d, k = %d: max |err| / bound = %.3f" % (m, k, ratio.max()))
    assert np.all(np.abs(got - want) <= bound), ratio.max()
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("c0", [3, 16, 7])
def test_rowquad_on_a_window_of_a_wider_panel(c0):
    """columns [c0, c0 + k) of a wider panel (an odd c0 takes the scalar loads), the result into a column of another wide panel"""
    import rails_amd
    from rails_amd.wrappers import HipMultiVectorWrapper as MV, _p

    ctx = rails_amd.Context(device=0, seed=1)
    g = np.random.default_rng(c0)
    m, k = 2500, 45
    U, S = _kernel_case(g, m, k)
    wide = g.standard_normal((m, c0 + k + 6))
    wide[:, c0:c0 + k] = U
    Wd = MV(ctx, data=wide)
    out = MV(ctx, data=np.full((m, 5), 7.0))
    Spad = np.asfortranarray(np.pad(S, ((0, 3), (0, 0))))  # leading dimension k + 3
    rails_amd._lib.check(ctx.lib.rails_panel_rowquad(ctx.h, Wd.panel.h, c0, k, _p(Spad), k + 3, out.panel.h, 2), "rails_panel_rowquad")
    got = out.to_host()
    want = np.einsum("ij,jl,il->i", U, S, U)
    bound = 8 * k * EPS * np.einsum("ij,jl,il->i", np.abs(U), np.abs(S), np.abs(U))
    assert np.all(np.abs(got[:, 2] - want) <= bound)
    assert np.all(got[:, [0, 1, 3, 4]] == 7.0)  # the neighbours of the output column are untouched
    # into the input's own panel, outside the window; inside it is refused
    rails_amd._lib.check(ctx.lib.rails_panel_rowquad(ctx.h, Wd.panel.h, c0, k, _p(Spad), k + 3, Wd.panel.h, c0 + k + 1), "rails_panel_rowquad")
    assert np.all(np.abs(Wd.to_host()[:, c0 + k + 1] - want) <= bound)
    assert ctx.lib.rails_panel_rowquad(ctx.h, Wd.panel.h, c0, k, _p(Spad), k + 3, Wd.panel.h, c0 + 1) != 0
    ctx.close()


@pytest.mark.gpu
def test_object_against_dense_numpy():
    import rails_amd

    ctx = rails_amd.Context(device=0, seed=3)
    U, S = _object_problem()
    m, k = U.shape
    X = U @ S @ U.T
    nX = np.linalg.norm(X, 2)
    sol = rails_amd.Solution(ctx, U, S)
    assert (sol.k, sol.m) == (k, m)
    np.testing.assert_array_equal(sol.S(), (S + S.T) / 2)
    # trace, variance, products, entries: sums of m k^2 (or fewer) products of entries
    bound = m * k * k * EPS * np.abs(U).max() ** 2 * np.abs(S).max()
    assert abs(sol.trace() - np.trace(X)) <= bound
    assert np.abs(sol.variance() - np.diag(X)).max() <= bound
    W = np.random.default_rng(5).standard_normal((m, 16))
    assert np.abs(sol.apply(W) - X @ W).max() <= bound * m * np.abs(W).max()
    rows, cols = np.array([0, 7, 1499, 7, 300]), np.array([1499, 2, 3])
    assert np.abs(sol.block(rows, cols) - X[np.ix_(rows, cols)]).max() <= bound
    assert np.abs(sol.block(rows) - X[np.ix_(rows, rows)]).max() <= bound
    with pytest.raises(rails_amd.RailsError):
        sol.block([0, m])
    # eigenpairs
    w = np.linalg.eigvalsh(X)
    w = w[np.argsort(-np.abs(w))]
    for want in (10, 0):
        lam, Z = sol.eigs(want)
        n = want if want else k
        assert lam.shape == (n,) and Z.shape == (m, n)
        assert np.all(np.abs(lam[:-1]) >= np.abs(lam[1:]))
        err, resid, orth = np.abs(lam - w[:n]).max(), np.linalg.norm(X @ Z - Z * lam, axis=0).max(), np.abs(Z.T @ Z - np.eye(n)).max()
        print("eigs(%d): eigenvalue error %.2e max|lambda|, residual %.2e |X|, |Z'Z - I| %.2e" % (want, err / abs(w[0]), resid / nX, orth))
        assert err <= 1e-11 * abs(w[0]) and resid <= 1e-11 * nX and orth <= 1e-11
    sol.close()
    ctx.close()


@pytest.mark.gpu
def test_eigs_truncates_a_rank_deficient_solution():
    import rails_amd

    ctx = rails_amd.Context(device=0, seed=3)
    U, S = _object_problem(deficient=True)
    X = U @ S @ U.T
    sol = rails_amd.Solution(ctx, U, S)
    lam, Z = sol.eigs(0, tol=1e-8)
    assert lam.size == np.linalg.matrix_rank(U) == U.shape[1] - 2
    assert np.linalg.norm(Z @ np.diag(lam) @ Z.T - X, 2) <= 1e-8 * np.linalg.norm(X, 2)
    small = sol.truncate(1e-8)
    assert small.k == lam.size
    assert abs(small.trace() - np.trace(X)) <= 1e-8 * np.linalg.norm(X, 2) * lam.size
    small.close()
    sol.close()
    ctx.close()
