"""The one-point maps of the solution object X = U S U' (rails_solution_maps; rails_amd/solution.py: Solution.maps) and its pairs on the
device against tests/covariance_reference.py: covariance maps within 8 k eps (|U_i||S||U_r|'), correlation maps within the derived
first-order bound, exact zeros for an all-zero row of U, a unit diagonal, agreement of pairs, maps and rails_solution_block with each
other, the variance column bit for bit, the refusals, and pairs across the two row sets of a lifted descriptor-system solution."""
import ctypes as C
import functools

import numpy as np
import pytest

import covariance_reference as CR
import solution_reference as R

pytestmark = pytest.mark.gpu

_i32p = C.POINTER(C.c_int32)
EINVAL = -1


@pytest.fixture(scope="module")
def ctx():
    import rails_amd

    c = rails_amd.Context(device=0, seed=1)
    yield c
    c.close()


def _err(got, want):
    return np.abs(np.asarray(got - want, dtype=np.float64))


@functools.lru_cache(maxsize=None)
def cov_case(m, k):
    """U with rows over six decades, S symmetric indefinite; the longdouble maps for 64 reference unknowns and their bound: computed once,
    the smaller q take the leading columns"""
    U, S = R.kernel_case(np.random.default_rng(17 * m + k), m, k)
    rows = CR.map_rows(m, 64)
    want, bound = CR.maps(U, S, rows), CR.maps_bound(U, S, rows)
    for a in (U, S, rows, want, bound):
        a.setflags(write=False)
    return U, S, rows, want, bound


@functools.lru_cache(maxsize=None)
def corr_case(m, k):
    zero = 5 if m > 5 else None
    U, S = CR.corr_problem(m, k, zero)
    rows = CR.map_rows(m, 64).copy()
    if zero is not None:
        rows[[7, 20]] = zero  # the all-zero row as a reference unknown, inside q = 16 and beyond it
    want, bound = CR.correlations(U, S, rows), CR.correlations_bound(U, S, rows)
    premise = CR.variance_ratio(U, S).max()
    for a in (rows, want, bound):
        a.setflags(write=False)
    return U, S, rows, want, bound, zero, premise


@pytest.mark.parametrize("k", CR.MAP_K)
@pytest.mark.parametrize("m", CR.MAP_M)
def test_covariance_maps(ctx, m, k):
    import rails_amd

    U, S, rows, want, bound = cov_case(m, k)
    sol = rails_amd.Solution(ctx, U, S)
    for q in CR.MAP_Q:
        got = sol.maps(rows[:q])
        err = _err(got, want[:, :q])
        print("covariance maps m = %d, k = %d, q = %d: max |err| / bound = %.3g" % (m, k, q, (err / bound[:, :q]).max()))
        assert got.shape == (m, q) and np.all(np.isfinite(got)) and np.all(err <= bound[:, :q])
    sol.close()


@pytest.mark.parametrize("k", CR.MAP_K)
@pytest.mark.parametrize("m", CR.MAP_M)
def test_correlation_maps(ctx, m, k):
    import rails_amd

    U, S, rows, want, bound, zero, premise = corr_case(m, k)
    assert premise < 1e-6  # tau Vbar / v: the first-order bound applies
    sol = rails_amd.Solution(ctx, U, S)
    for q in CR.MAP_Q:
        got = sol.maps(rows[:q], correlation=True)
        err = _err(got, want[:, :q])
        live = bound[:, :q] > 0
        print("correlation maps m = %d, k = %d, q = %d: max |err| / bound = %.3g" % (m, k, q, (err[live] / bound[:, :q][live]).max() if live.any() else 0.0))
        assert np.all(np.isfinite(got)) and np.all(err <= bound[:, :q])
        for j, r in enumerate(rows[:q]):
            if r == zero:
                assert np.all(got[:, j] == 0.0)  # a reference unknown without variance: an exact zero column
            else:
                assert abs(got[r, j] - 1.0) <= 4 * CR.EPS  # corr(r, r)
        if zero is not None:
            assert np.all(got[zero] == 0.0)  # a map row without variance: exact zeros
    sol.close()


def test_pairs_maps_and_block_agree(ctx):
    import rails_amd

    m, k, q = 129, 33, 17
    U, S, rows, want, bound = cov_case(m, k)
    sol = rails_amd.Solution(ctx, U, S)
    maps = sol.maps(rows[:q])
    every = np.arange(m, dtype=np.int32)
    blk = sol.block(every, rows[:q])
    blk_bound = R.block_bound(U, S, every, rows[:q])
    assert np.all(_err(blk, want[:, :q]) <= blk_bound)
    for j, r in enumerate(rows[:q]):
        ib = np.full(m, r, dtype=np.int32)
        col = sol.covariance(every, ib)
        pb = CR.pairs_bound(U, S, every, ib)
        assert np.all(_err(col, want[:, j]) <= pb)
        assert np.all(np.abs(col - maps[:, j]) <= pb + bound[:, j])
        assert np.all(np.abs(col - blk[:, j]) <= pb + blk_bound[:, j])
        assert np.all(np.abs(col - sol.covariance(None, ib)) == 0.0)  # a NULL side is the identity
        # S symmetric: X[i, r] and X[r, i] are the same number to both bounds
        assert np.all(np.abs(col - sol.covariance(ib, every)) <= 2 * pb)
    sol.close()


def _maps_raw(sol, rows, q, corr, out, oc0, var_col):
    return sol.lib.rails_solution_maps(sol.h, rows.ctypes.data_as(_i32p), q, corr, out.panel.h, oc0, var_col)


@pytest.mark.parametrize("corr", [0, 1])
def test_variance_column_and_untouched_columns(ctx, corr):
    import rails_amd
    from rails_amd._lib import check

    m, k, q = 129, 33, 16
    U, S, rows, _, _, zero, _ = corr_case(m, k)
    sol = rails_amd.Solution(ctx, U, S)
    var = sol.variance()
    plain = sol.maps(rows[:q], correlation=bool(corr))
    for oc0, vc in ((1, 0), (0, q), (2, q + 3)):
        out = rails_amd.HipMultiVectorWrapper(ctx, data=np.full((m, q + 5), 7.0))
        check(_maps_raw(sol, rows, q, corr, out, oc0, vc), "rails_solution_maps")
        got = out.to_host()
        assert np.array_equal(R.bits(got[:, vc]), R.bits(var))  # bit for bit variance()
        assert np.array_equal(R.bits(got[:, oc0:oc0 + q]), R.bits(plain))  # the same maps with and without the column
        rest = [j for j in range(q + 5) if j != vc and not oc0 <= j < oc0 + q]
        assert np.all(got[:, rest] == 7.0)
    sol.close()


def test_refusals_write_nothing(ctx):
    import rails_amd

    m, k = 40, 9
    U, S = CR.corr_problem(m, k)
    sol = rails_amd.Solution(ctx, U, S)
    out = rails_amd.HipMultiVectorWrapper(ctx, data=np.full((m, 6), 7.0))
    rows = np.array([0, 5, 39], dtype=np.int32)

    def refused(rc):
        assert rc == EINVAL, rc
        assert sol.lib.rails_last_error()
        assert np.all(out.to_host() == 7.0)

    for corr in (0, 1):
        refused(_maps_raw(sol, np.array([0, -1, 39], dtype=np.int32), 3, corr, out, 0, -1))  # one rank: nobody owns it
        refused(_maps_raw(sol, np.array([0, m, 39], dtype=np.int32), 3, corr, out, 0, -1))
        refused(_maps_raw(sol, np.array([0, -2, 39], dtype=np.int32), 3, corr, out, 0, -1))
        refused(_maps_raw(sol, rows, 3, corr, out, 0, 1))  # the variance column inside the maps
        refused(_maps_raw(sol, rows, 3, corr, out, 0, 6))  # ... or outside the panel
        refused(_maps_raw(sol, rows, 3, corr, out, 4, -1))  # the maps outside the panel
    refused(_maps_raw(sol, np.zeros(65, dtype=np.int32), 65, 0, rails_amd.HipMultiVectorWrapper(ctx, m=m, n=65), 0, -1))
    short = rails_amd.HipMultiVectorWrapper(ctx, data=np.full((m - 1, 6), 7.0))
    assert _maps_raw(sol, rows, 3, 0, short, 0, -1) == EINVAL and np.all(short.to_host() == 7.0)
    assert _maps_raw(sol, rows, 3, 0, sol.U(), 0, -1) == EINVAL  # the solution's own panel
    with pytest.raises(IndexError):
        sol.maps(np.array([m]))
    with pytest.raises(ValueError):
        sol.maps(np.zeros(65, dtype=np.int32))
    assert sol.maps(np.zeros(0, dtype=np.int32)).shape == (m, 0)
    sol.close()


def test_pairs_across_the_row_sets_of_a_lifted_solution():
    """a small descriptor system as in tests/test_gpu_schur.py: set-1 (algebraic) and set-2 unknowns scattered through the index range,
    a solution object on the set-2 rows lifted to all unknowns.  Pairs with one unknown in each set, maps for reference unknowns of both
    sets and the variance agree with the dense X of the lifted factor within the kernels' bounds, and the lifted factor is the host
    prolongation of V"""
    import scipy.sparse as sp

    import rails_amd
    from rails_amd.schur import SchurOperator

    g = np.random.default_rng(0)
    n1, n2, k = 40, 150, 12
    n = n1 + n2
    mask1 = np.zeros(n, dtype=bool)
    mask1[np.sort(g.permutation(n)[:n1])] = True
    A = (0.3 * sp.random(n, n, density=0.04, random_state=np.random.RandomState(0), format="lil")).tolil()
    A.setdiag(np.where(mask1, 2.0 + g.uniform(0, 1, n), -4.0 - g.uniform(0, 1, n)))
    A = A.tocsr()
    A.sort_indices()
    Ad = A.toarray()
    ctx = rails_amd.Context(device=0, seed=4)
    schur = SchurOperator(ctx, (A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data.astype(np.float64)), np.where(mask1, 0.0, 1.0))
    V = np.linalg.qr(g.standard_normal((n2, k)))[0]
    L = g.integers(-2, 3, (k, k)).astype(np.float64)
    T = L @ L.T + np.eye(k)
    small = rails_amd.Solution(ctx, V, T)
    full = schur.lift(small)
    assert full.m == n
    i1, i2 = np.flatnonzero(mask1), np.flatnonzero(~mask1)
    Vf = np.zeros((n, k))
    Vf[i2] = V
    Vf[i1] = -np.linalg.solve(Ad[np.ix_(i1, i1)], Ad[np.ix_(i1, i2)] @ V)
    Uf, Sf = full.U().to_host(), full.S()
    assert np.abs(Uf - Vf).max() <= 1e-10 * np.abs(Vf).max()  # the sparse solves of the lift, as tests/test_gpu_solution_schur.py bounds them
    # pairs across the sets, both orders, plus pairs within each set
    ia = np.concatenate([i1, i2[:n1], i1[::-1], i2[:7]]).astype(np.int32)
    ib = np.concatenate([i2[:n1], i1, i1, i2[7:14]]).astype(np.int32)
    cov = full.covariance(ia, ib)
    assert np.all(_err(cov, CR.pairs(Uf, Sf, ia, ib)) <= CR.pairs_bound(Uf, Sf, ia, ib))
    X = Vf @ T @ Vf.T  # the dense host X
    assert np.abs(cov - X[ia, ib]).max() <= 1e-9 * np.abs(X).max()
    rows = np.array([i1[0], i2[0], i1[-1], i2[-1]], dtype=np.int32)
    assert np.all(_err(full.maps(rows), CR.maps(Uf, Sf, rows)) <= CR.maps_bound(Uf, Sf, rows))
    corr = full.maps(rows, correlation=True)
    assert np.all(_err(corr, CR.correlations(Uf, Sf, rows)) <= CR.correlations_bound(Uf, Sf, rows))
    assert np.abs(corr - X[:, rows] / np.sqrt(np.outer(np.diag(X), np.diag(X)[rows]))).max() <= 1e-9
    full.close()
    small.close()
    ctx.close()
