"""The solution object X = U S U' on the device (include/rails_solution.h, rails_amd/solution.py): the one-pass kernel
rails_panel_rowquad = diag(U S U') against numpy, and trace / apply / block / eigs of the object against dense algebra.

Kernel bound, componentwise and derived, not tuned: out_i is an inner product of 2k terms (k for a row of U S, k for the reduction
against the row of U), so its rounding error is at most gamma_2k (|U||S||U|')_ii with gamma_n = n eps / (1 - n eps) whatever the order of
summation; 8 k eps leaves a factor 4 for the MFMA's internal summation order and the reference value's own error.

Object bound: eigenvalues within 1e-11 max|lambda| and residuals within 1e-11 |X|_2, the bound this project uses for device
orthogonalisation against the oracle (tests/test_gpu_kernels.py).  U has condition about 1e2; test_object_bound_holds_for_numpy_on_the_host
(no GPU) confirms that the same computation in numpy -- QR, then a small symmetric eigensolve -- stays inside it for the chosen seed.

variance, block, apply and trace of the object are also held to componentwise bounds against longdouble references at m = 300, k = 40
(tests/solution_reference.py states and derives them; tests/test_solution_reference_host.py shows numpy in double meets them)."""
import ctypes as C

import numpy as np
import pytest

import solution_reference as R

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


# ---- the object at derived bounds (tests/solution_reference.py) ---------------------------------------------------------------------------


@pytest.fixture(scope="module")
def small_object():
    import rails_amd

    ctx = rails_amd.Context(device=0, seed=3)
    U, S = R.object_problem()
    sol = rails_amd.Solution(ctx, U, S)
    assert np.array_equal(sol.S(), S)  # S is symmetric: the object's (S + S')/2 is S itself
    yield ctx, sol, U, S
    sol.close()
    ctx.close()


def _err(got, want):
    return np.abs(np.asarray(got - want, dtype=np.float64))


@pytest.mark.gpu
def test_object_variance_trace_and_blocks_at_derived_bounds(small_object):
    import rails_amd

    ctx, sol, U, S = small_object
    m, k = U.shape
    err, bound = _err(sol.variance(), R.rowquad(U, S)), R.rowquad_bound(U, S)
    print("variance: max |err| / bound = %.3g" % (err / bound).max())
    assert np.all(err <= bound)
    terr, tbound = abs(float(sol.trace() - R.trace(U, S))), R.trace_bound(U, S)
    print("trace: |err| / bound = %.3g" % (terr / tbound))
    assert terr <= tbound
    for rows, cols in R.block_cases(m):
        got = sol.block(rows, cols)
        err, bound = _err(got, R.block(U, S, rows, cols)), R.block_bound(U, S, rows, cols)
        print("block %s x %s: max |err| / bound = %.3g" % (rows, cols, (err / bound).max()))
        assert got.shape == (len(rows), len(cols)) and np.all(err <= bound)
    rows = R.block_cases(m)[0][0]
    assert np.all(_err(sol.block(rows), R.block(U, S, rows, rows)) <= R.block_bound(U, S, rows, rows))
    for bad in ([0, m], [-1]):
        with pytest.raises(rails_amd.RailsError):
            sol.block(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("nc", R.APPLY_NC)
@pytest.mark.parametrize("wc0,yc0", [(3, 2), (2, 5)])
def test_object_apply_on_windows_at_the_derived_bound(small_object, nc, wc0, yc0):
    """W and Y are windows, at an odd and an even offset each, of wider panels; nc = 257 takes rails_panel_gemm_wide"""
    import rails_amd
    from rails_amd.wrappers import HipMultiVectorWrapper as MV

    ctx, sol, U, S = small_object
    m = U.shape[0]
    W = R.apply_rhs(m, nc)
    wide = np.full((m, wc0 + nc + 3), np.nan)  # nothing outside the window is read
    wide[:, wc0:wc0 + nc] = W
    Wd, Yd = MV(ctx, data=wide), MV(ctx, data=np.full((m, yc0 + nc + 2), 7.0))
    rails_amd._lib.check(ctx.lib.rails_solution_apply(sol.h, Wd.panel.h, wc0, nc, Yd.panel.h, yc0), "rails_solution_apply")
    got = Yd.to_host()
    err, bound = _err(got[:, yc0:yc0 + nc], R.apply(U, S, W)), R.apply_bound(U, S, W)
    print("apply nc = %d, W at %d, Y at %d: max |err| / bound = %.3g" % (nc, wc0, yc0, (err / bound).max()))
    assert np.all(err <= bound)
    assert np.all(got[:, :yc0] == 7.0) and np.all(got[:, yc0 + nc:] == 7.0)  # the columns around Y are untouched


@pytest.mark.gpu
def test_object_apply_no_columns_and_refusals(small_object):
    from rails_amd.wrappers import HipMultiVectorWrapper as MV

    ctx, sol, U, S = small_object
    m, k = U.shape
    Wd, Yd = MV(ctx, data=R.apply_rhs(m, 16)), MV(ctx, data=np.full((m, 4), 7.0))
    assert ctx.lib.rails_solution_apply(sol.h, Wd.panel.h, 3, 0, Yd.panel.h, 1) == 0  # nc = 0: nothing happens
    assert np.all(Yd.to_host() == 7.0)
    own = sol.U()
    before = R.bits(own.to_host())
    assert ctx.lib.rails_solution_apply(sol.h, Wd.panel.h, 0, 16, own.panel.h, 0) != 0  # Y is the solution's own panel
    assert ctx.lib.rails_solution_apply(sol.h, Wd.panel.h, 0, 16, Yd.panel.h, 0) != 0  # 16 columns into a capacity of 4
    assert ctx.lib.rails_solution_apply(sol.h, Wd.panel.h, 1, 16, Yd.panel.h, 0) != 0  # W's window leaves its capacity
    short = MV(ctx, data=np.zeros((m - 1, 16)))
    assert ctx.lib.rails_solution_apply(sol.h, short.panel.h, 0, 16, short.panel.h, 0) != 0  # row mismatch
    assert np.array_equal(R.bits(own.to_host()), before) and np.all(Yd.to_host() == 7.0)


@pytest.mark.gpu
def test_borrowed_window_agrees_bitwise_with_a_copy(small_object):
    """copy=False on columns [3, 3 + k) of a wider panel and copy=True (its own aligned panel) hold the same numbers: the same bits out"""
    import rails_amd
    from rails_amd.wrappers import HipMultiVectorWrapper as MV

    ctx, _, U, S = small_object
    m, k = U.shape
    wide = np.random.default_rng(8).standard_normal((m, 3 + k + 2))
    wide[:, 3:3 + k] = U
    Wd = MV(ctx, data=wide)
    view = Wd.view(3, 3 + k - 1)
    assert (view.c0, view.n) == (3, k)
    borrowed, copied = rails_amd.Solution(ctx, view, S, copy=False), rails_amd.Solution(ctx, view, S, copy=True)
    c0 = C.c_int(-1)
    assert ctx.lib.rails_solution_panel(borrowed.h, C.byref(c0)) == Wd.panel.h.value and c0.value == 3
    assert ctx.lib.rails_solution_panel(copied.h, C.byref(c0)) != Wd.panel.h.value and c0.value == 0
    assert np.array_equal(R.bits(borrowed.U().to_host()), R.bits(U)) and np.array_equal(R.bits(copied.U().to_host()), R.bits(U))
    assert np.array_equal(R.bits(borrowed.variance()), R.bits(copied.variance()))
    assert np.all(_err(borrowed.variance(), R.rowquad(U, S)) <= R.rowquad_bound(U, S))
    assert borrowed.trace() == copied.trace()
    for nc in (16, 257):
        W = R.apply_rhs(m, nc)
        assert np.array_equal(R.bits(borrowed.apply(W)), R.bits(copied.apply(W))), nc
    rows, cols = R.block_cases(m)[0]
    assert np.array_equal(R.bits(borrowed.block(rows, cols)), R.bits(copied.block(rows, cols)))
    assert np.array_equal(R.bits(Wd.to_host()), R.bits(wide))  # the borrowed panel is unchanged, its other columns included
    borrowed.close()
    copied.close()
