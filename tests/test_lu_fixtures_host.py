"""The fixtures of tests/lu_fixtures.py on the host: the level patterns that tests/test_gpu_lu_levels.py relies on to reach every
launch form of rails_amd/csrc/splu.hip and sptrsv.hip, Pr A Pc = L U, the host substitution against the matrix itself, and the
exactness of the dyadic fixture in fp64."""
import numpy as np
import pytest
import scipy.sparse as sp

import lu_fixtures as F

W3 = [1100, 1100, 1100]
BORDER_L = W3 + [1] * 6


@pytest.fixture(scope="module")
def fixtures():
    return {"blocks1100": F.block_factors(1100, 3, seed=1), "blocks1000": F.block_factors(1000, 3, seed=1),
            "bordered": F.bordered_blocks(seed=3), "dyadic": F.dyadic_factors(3400, seed=1)}


def four_plans(fx):
    (pl, pu), (put, plt) = fx.plans(False), fx.plans(True)
    return pl, pu, put, plt


def test_level_plan_restates_the_segment_rule():
    """a chain, a diagonal and a hand-made two-level triangle with a 1025-row level"""
    n = 5
    chain = sp.diags([np.ones(n), np.ones(n - 1)], [0, -1]).tocsr()
    p = F.level_plan(chain, True)
    assert p.widths == [1] * n and p.pattern == "r" and p.launches == 1
    p = F.level_plan(chain.T, False)
    assert p.widths == [1] * n and [int(o[0]) for o in p.order] == [4, 3, 2, 1, 0]
    p = F.level_plan(sp.identity(1025, format="csr"), True)
    assert p.widths == [1025] and p.pattern == "W"
    assert F.level_plan(sp.identity(1024, format="csr"), True).pattern == "r"  # the threshold is "more than 1024"
    # rows 1 .. 1025 name row 0, row 1026 names row 1: levels 1, 1025, 1
    rows = list(range(1, 1026)) + [1026]
    cols = [0] * 1025 + [1]
    T = sp.coo_matrix((np.ones(1026), (rows, cols)), shape=(1027, 1027)).tocsr() + sp.identity(1027)
    p = F.level_plan(T, True)
    assert p.widths == [1, 1025, 1] and p.pattern == "rWr" and p.launches == 3
    assert F.sptrsv_plan(T, True, 1) == "rWr" and F.sptrsv_plan(T, True, 2) == "rWr" and F.sptrsv_plan(chain, True, 1025) == "W" * n


def test_block_fixture_levels(fixtures):
    for plans in (four_plans(fixtures["blocks1100"]),):
        assert [p.widths for p in plans] == [W3] * 4 and [p.pattern for p in plans] == ["WWW"] * 4
    assert fixtures["blocks1100"].launches(False) == 6 and fixtures["blocks1100"].launches(True) == 6
    plans = four_plans(fixtures["blocks1000"])
    assert [p.widths for p in plans] == [[1000] * 3] * 4 and [p.pattern for p in plans] == ["r"] * 4
    assert fixtures["blocks1000"].launches(False) == 2
    # the 1000 blocks are the leading blocks of the 1100, entry for entry
    big, small = fixtures["blocks1100"], fixtures["blocks1000"]
    for a, b in ((big.L, small.L), (big.U, small.U)):
        assert (sp.csr_matrix(a)[:3000][:, :3000] != sp.csr_matrix(b)).nnz == 0
        assert sp.csr_matrix(a)[:3000][:, 3000:].nnz == 0 and sp.csr_matrix(a)[3000:][:, :3000].nnz == 0
    # the permutations are not near the identity
    for fx in (big, small):
        assert (fx.perm_r == np.arange(fx.n)).mean() < 0.01 and (fx.perm_c == np.arange(fx.n)).mean() < 0.01 and np.any(fx.perm_r != fx.perm_c)


def test_bordered_fixture_levels(fixtures):
    """L and U': the blocks' three wide levels, then the border rows one by one ('WWWr'); U and L': one wide level between two runs"""
    fx = fixtures["bordered"]
    assert fx.n == 3306
    pl, pu, put, plt = four_plans(fx)
    assert pl.widths == BORDER_L and put.widths == BORDER_L and pl.pattern == "WWWr" and put.pattern == "WWWr"
    for p in (pu, plt):
        assert p.pattern == "rWr" and len(p.widths) == 9, p.widths
        wide = [w for w in p.widths if w > F.NARROW]
        assert len(wide) == 1 and p.widths[0] <= 16 and max(w for w in p.widths if w <= F.NARROW) > 256, p.widths
    assert fx.launches(False) == 7 and fx.launches(True) == 7
    # the older path's threshold is rows * columns: at one column only the wide levels are launches of their own, at 40 columns
    # the levels of U and L' from 36 rows on are, and the border rows of L and U' still make a chain
    plans = [(F.sptrsv_plan(T, lower, 1), F.sptrsv_plan(T, lower, 40)) for T, lower in fx.triangles(False) + fx.triangles(True)]
    assert plans == [("WWWr", "WWWr"), ("rWr", "r" + "W" * 6), ("WWWr", "WWWr"), ("rWr", "r" + "W" * 6)]


def test_dyadic_fixture_levels(fixtures):
    fx = fixtures["dyadic"]
    pl, pu, put, plt = four_plans(fx)
    assert pl.widths == [1500, 900, 1000] and pl.pattern == "Wr"
    assert pu.widths == [900, 1500, 1000] and pu.pattern == "rWr"
    assert put.widths == [1000, 1500, 900] and put.pattern == "rWr"
    assert plt.widths == [1000, 900, 1500] and plt.pattern == "rW"
    assert fx.launches(False) == 5 and fx.launches(True) == 5
    for T in (fx.L, fx.U):
        per_row = np.diff(sp.csr_matrix(T).indptr) - 1
        per_col = np.diff(sp.csc_matrix(T).indptr) - 1
        assert per_row.max() > 32 and per_col.max() > 16 and per_row.min() == 0 and np.any(per_row == 17)
    off = lambda T: sp.csr_matrix(T - sp.diags(T.diagonal()))
    assert set(np.abs(off(fx.L).data)) | set(np.abs(off(fx.U).data)) <= {0.0, 0.25, 0.5}
    assert np.all(fx.L.diagonal() == 1.0) and set(np.abs(fx.U.diagonal())) == {0.5, 1.0, 2.0, 4.0}


@pytest.mark.parametrize("name", ["blocks1100", "blocks1000", "bordered", "dyadic"])
def test_factors_and_host_solve(fixtures, name):
    """Pr A Pc = L U with scipy's permutation matrices, and the host substitution solves with A itself"""
    fx = fixtures[name]
    Pr, Pc = F.permutation_matrices(fx)
    LU = sp.csr_matrix(fx.L @ fx.U)
    assert abs(Pr @ fx.A @ Pc - LU).max() <= 8 * np.finfo(float).eps * abs(LU).max()
    assert sp.tril(fx.U, -1).nnz == 0 and sp.triu(fx.L, 1).nnz == 0 and np.all(fx.L.diagonal() == 1.0)
    assert np.finfo(np.longdouble).eps < 1e-18  # the reference type is wider than fp64 here
    g = np.random.default_rng(3)
    B = g.uniform(-1.0, 1.0, (fx.n, 3))
    for trans in (False, True):
        X = fx.solve(B, trans=trans)
        assert X.dtype == np.longdouble
        X = X.astype(np.float64)
        At = fx.A.T if trans else fx.A
        # the factors hold A to fp64 rounding and the residual is formed in fp64: a few roundings of |A| |X|
        assert np.abs(At @ X - B).max() <= 64 * np.finfo(float).eps * (abs(At) @ np.abs(X)).max(), (name, trans)
    # the restriction: (A^-1 E x)[rows]
    rows = np.sort(g.choice(fx.n, fx.n * 2 // 5, replace=False))
    E = np.zeros((fx.n, 3))
    E[rows] = B[rows]
    for trans in (False, True):
        assert np.array_equal(fx.solve(B[rows], trans=trans, rows=rows), fx.solve(E, trans=trans)[rows])


def test_dyadic_solve_is_exact_in_fp64(fixtures):
    """integer right-hand sides in [-8, 8]: substitution in fp64, in longdouble and with each row's sum in the opposite order give
    the same numbers, both transposes, with and without a restriction -- no operation of the solve rounds"""
    fx = fixtures["dyadic"]
    g = np.random.default_rng(11)
    rows = np.sort(g.choice(fx.n, fx.n * 2 // 5, replace=False))
    for r in (None, rows):
        B = g.integers(-8, 9, (fx.n if r is None else r.size, 4)).astype(np.float64)
        for trans in (False, True):
            x64 = fx.solve(B, trans=trans, rows=r, dtype=np.float64)
            xld = fx.solve(B, trans=trans, rows=r, dtype=np.longdouble)
            xrev = fx.solve(B, trans=trans, rows=r, dtype=np.float64, reverse=True)
            assert x64.dtype == np.float64 and np.array_equal(x64.astype(np.longdouble), xld) and np.array_equal(x64, xrev), (trans, r is None)
            assert np.abs(x64).max() < 2.0 ** 25 and np.array_equal(x64 * 2.0 ** 14, np.round(x64 * 2.0 ** 14))
            assert np.count_nonzero(x64) > 0.9 * x64.size
