"""The device LU solves (rails_amd/csrc/splu.hip: k_lu_level, k_lu_run; sptrsv.hip: k_sptrsv_level, k_sptrsv_chain) on factors whose
level structure is known (tests/lu_fixtures.py, checked on the host by tests/test_lu_fixtures_host.py): wide levels in first, middle
and last position of both sweeps and both transposes, a wide level between two runs, column windows of wider panels, the workspace,
and the four permutation maps exactly.  The reference is a level-by-level substitution on the host in np.longdouble with the same
factors and permutations (lu_fixtures.Factors.solve): not the code under test and not SuperLU's solve.

Tolerance.  The same host substitution in fp64 lies this far from the longdouble reference (relative Frobenius error, X uniform in
(-1, 1), worst over the widths 1, 3, 16, 17, 40, 64, 130 and both transposes; measured on the host):
    blocks1100 6.79e-17    blocks1000 6.93e-17    bordered 7.52e-17
The device sums a row's products in another order (16 lanes and a butterfly), so it gets 4 times that: 2.72e-16, 2.77e-16 and
3.01e-16.  The tests compute the figure again from the fixture they run on (host_error below) instead of trusting these digits."""
import numpy as np
import pytest

import lu_fixtures as F

pytestmark = pytest.mark.gpu

WIDTHS = (1, 3, 16, 17, 40, 64, 130)
ORDER_FACTOR = 4.0  # device bound = this times the host fp64 solve's own error against the longdouble reference


@pytest.fixture(scope="module")
def ctx():
    import rails_amd

    c = rails_amd.Context(device=0, seed=1)
    yield c
    c.close()


class Case:
    """a fixture, its 130-column right-hand side and, per transpose, the longdouble reference and the host fp64 solve (computed once)"""

    def __init__(self, fx, seed):
        self.fx = fx
        self.X = np.random.default_rng(seed).uniform(-1.0, 1.0, (fx.n, max(WIDTHS)))
        self._ref = {}

    def ref(self, trans):
        if trans not in self._ref:
            self._ref[trans] = (self.fx.solve(self.X, trans=trans), self.fx.solve(self.X, trans=trans, dtype=np.float64))
        return self._ref[trans]

    def error(self, Y, trans, nc):
        """relative Frobenius error of an n x nc result against the reference's leading nc columns (the reference computes every
        column by itself, so those are the reference of the nc-column solve)"""
        ref = self.ref(trans)[0][:, :nc]
        return float(np.linalg.norm((Y - ref).astype(np.float64)) / np.linalg.norm(ref.astype(np.float64)))

    def host_error(self, widths=WIDTHS):
        return max(self.error(self.ref(trans)[1][:, :nc], trans, nc) for trans in (False, True) for nc in widths)


@pytest.fixture(scope="module")
def cases():
    return {"blocks1100": Case(F.block_factors(1100, 3, seed=1), 5), "blocks1000": Case(F.block_factors(1000, 3, seed=1), 5),
            "bordered": Case(F.bordered_blocks(seed=3), 5)}


@pytest.fixture(scope="module")
def dyadic():
    return F.dyadic_factors(3400, seed=1)


def make_lu(ctx, fx, rows=None):
    import rails_amd

    return rails_amd.SparseLU(ctx, fx.A, rows=rows, lu=fx)


def dev(ctx, X):
    import rails_amd

    return rails_amd.HipMultiVectorWrapper(ctx, data=X)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.mark.parametrize("name", ["blocks1100", "blocks1000", "bordered", "dyadic"])
def test_launch_forms_are_reached(ctx, cases, dyadic, name):
    """launches of a solve and levels of each triangle are what the host plan says: 6 launches, all k_lu_level, for the 1100-block
    factors; 2, all k_lu_run, for the 1000-block ones; 7 for the bordered matrix ('WWWr' + 'rWr'); 5 for the dyadic factors"""
    fx = dyadic if name == "dyadic" else cases[name].fx
    expect = {"blocks1100": 6, "blocks1000": 2, "bordered": 7, "dyadic": 5}[name]
    lu = make_lu(ctx, fx)
    X = dev(ctx, np.ones((fx.n, 2)))
    for trans in (False, True):
        assert fx.launches(trans) == expect
        lu.solve(X, trans=trans)
        assert lu.stats()["launches"] == expect, (name, trans, lu.stats())
    st = lu.stats()
    (pl, pu), (put, plt) = fx.plans(False), fx.plans(True)
    assert [st[k] for k in ("levels_L", "levels_U", "levels_Ut", "levels_Lt")] == [len(p.widths) for p in (pl, pu, put, plt)]
    assert st["n"] == fx.n and st["m"] == fx.n
    lu.close()


@pytest.mark.parametrize("name", ["blocks1100", "blocks1000", "bordered"])
def test_accuracy_against_longdouble(ctx, cases, name):
    """every width, both transposes, within ORDER_FACTOR times the host fp64 solve's own error (module docstring: 2.72e-16 for
    blocks1100, 2.77e-16 for blocks1000, 3.01e-16 for bordered)"""
    case = cases[name]
    bound = ORDER_FACTOR * case.host_error()
    assert 1e-17 < bound < 1e-15  # the measurement itself is sane: a few units of fp64 rounding
    lu = make_lu(ctx, case.fx)
    for trans in (False, True):
        for nc in WIDTHS:
            Xd = dev(ctx, case.X[:, :nc])
            Y = lu.solve(Xd, trans=trans).to_host()
            err = case.error(Y, trans, nc)
            print("%s trans=%d nc=%d: device error %.3e, bound %.3e" % (name, trans, nc, err, bound))
            assert err <= bound, (name, trans, nc, err, bound)
            assert same_bits(Xd.to_host(), case.X[:, :nc])  # the input panel is unchanged
    lu.close()


def test_restriction_through_wide_levels(ctx, cases):
    """rows = a random 40 % on the 1100-block factors: the zero fill (in_map = -1) and the skipped rows of the scatter (out_pos = -1)
    in k_lu_level, against the longdouble reference of the same restricted solve, bound as above"""
    case = cases["blocks1100"]
    fx = case.fx
    bound = ORDER_FACTOR * case.host_error()
    rows = np.sort(np.random.default_rng(8).choice(fx.n, fx.n * 2 // 5, replace=False))
    lu = make_lu(ctx, fx, rows=rows)
    X = case.X[rows][:, :17]
    for trans in (False, True):
        ref = fx.solve(X, trans=trans, rows=rows)
        Y = lu.solve(dev(ctx, X), trans=trans).to_host()
        err = float(np.linalg.norm((Y - ref).astype(np.float64)) / np.linalg.norm(ref.astype(np.float64)))
        print("restricted blocks1100 trans=%d: device error %.3e, bound %.3e" % (trans, err, bound))
        assert err <= bound, (trans, err, bound)
    assert lu.stats()["launches"] == 6 and lu.stats()["m"] == rows.size
    lu.close()


@pytest.mark.parametrize("restricted", [False, True])
def test_dyadic_solve_is_exact(ctx, dyadic, restricted):
    """integer right-hand sides on the dyadic factors: no operation rounds in any summation order (test_lu_fixtures_host.py), so the
    device result IS the reference, entry for entry -- a wrong row of in_map or out_pos, a missing zero or a stray write shows as a
    different number, not as a larger error.  Both transposes; all rows and a random 40 % of them."""
    fx = dyadic
    g = np.random.default_rng(21)
    rows = np.sort(g.choice(fx.n, fx.n * 2 // 5, replace=False)) if restricted else None
    lu = make_lu(ctx, fx, rows=rows)
    B = g.integers(-8, 9, (fx.n if rows is None else rows.size, 19)).astype(np.float64)
    for trans in (False, True):
        exact = fx.solve(B, trans=trans, rows=rows, dtype=np.float64)
        assert np.array_equal(exact.astype(np.longdouble), fx.solve(B, trans=trans, rows=rows))  # exact here as well
        Y = lu.solve(dev(ctx, B), trans=trans).to_host()
        assert np.array_equal(Y, exact), (trans, restricted, int((Y != exact).sum()))
    assert lu.stats()["launches"] == 5
    lu.close()


def test_one_arithmetic_in_both_launch_forms(ctx, cases):
    """the 1100-block factors run through k_lu_level only, their leading 1000 blocks through k_lu_run only; with the same
    right-hand side on the shared rows of L U y = c, the shared part of y is bitwise the same"""
    big, small = cases["blocks1100"].fx, cases["blocks1000"].fx
    nc, ns = 5, small.n
    Cf = np.random.default_rng(31).uniform(-1.0, 1.0, (big.n, nc))  # the right-hand side in the factors' own row order
    lus = [make_lu(ctx, big), make_lu(ctx, small)]
    for trans in (False, True):
        ys = []
        for fx, lu, c in ((big, lus[0], Cf), (small, lus[1], Cf[:ns])):
            pin, pout = (fx.perm_c, fx.perm_r) if trans else (fx.perm_r, fx.perm_c)
            x = lu.solve(dev(ctx, c[pin]), trans=trans).to_host()  # b[i] = c[pin[i]];  x[j] = y[pout[j]]
            y = np.empty_like(x)
            y[pout] = x
            ys.append(y)
        assert lus[0].stats()["launches"] == 6 and lus[1].stats()["launches"] == 2
        assert same_bits(ys[0][:ns], ys[1]), (trans, int((ys[0][:ns] != ys[1]).sum()))
    for lu in lus:
        lu.close()


def test_columns_are_independent_bitwise_across_launch_forms(ctx, cases):
    """bordered matrix (both kernels in every sweep): column j of a 40-column solve is bitwise the one-column solve of column j"""
    case = cases["bordered"]
    lu = make_lu(ctx, case.fx)
    X = case.X[:, :40]
    for trans in (False, True):
        Y = lu.solve(dev(ctx, X), trans=trans).to_host()
        for j in (0, 1, 17, 39):
            y = lu.solve(dev(ctx, X[:, j:j + 1]), trans=trans).to_host()
            assert same_bits(Y[:, j:j + 1], y), (trans, j)
    lu.close()


@pytest.mark.parametrize("xc0,yc0", [(1, 1), (1, 3), (2, 1), (2, 3)])
def test_column_windows_of_wider_panels(ctx, cases, xc0, yc0):
    """X a view at column xc0 of a panel whose other columns hold NaN, Y a view at column yc0 of a panel whose other columns hold a
    sentinel: the result is bitwise the solve at offset 0, and nothing else changes"""
    case = cases["bordered"]
    fx, nc = case.fx, 5
    lu = make_lu(ctx, fx)
    X = case.X[:, :nc]
    Xbig = np.full((fx.n, xc0 + nc + 2), np.nan)
    Xbig[:, xc0:xc0 + nc] = X
    Ybig = np.full((fx.n, yc0 + nc + 1), -7.25)
    for trans in (False, True):
        Y0 = lu.solve(dev(ctx, X), trans=trans).to_host()
        Px, Py = dev(ctx, Xbig), dev(ctx, Ybig)
        out = lu.solve(Px.view(xc0, xc0 + nc - 1), Y=Py.view(yc0, yc0 + nc - 1), trans=trans)
        assert out.c0 == yc0 and out.n == nc
        got = Py.to_host()
        assert same_bits(got[:, yc0:yc0 + nc], Y0), (trans, xc0, yc0)
        expect = Ybig.copy()
        expect[:, yc0:yc0 + nc] = Y0
        assert same_bits(got, expect)  # the sentinels beside the window are untouched
        assert same_bits(Px.to_host(), Xbig)
        assert np.all(np.isfinite(Y0))
    lu.close()


def test_windows_of_one_panel(ctx, cases):
    """X and Y as disjoint windows of one panel work (either order); overlapping windows are refused and nothing is written"""
    import rails_amd

    case = cases["bordered"]
    fx, nc = case.fx, 4
    lu = make_lu(ctx, fx)
    X = case.X[:, :nc]
    for trans in (False, True):
        Y0 = lu.solve(dev(ctx, X), trans=trans).to_host()
        for xa, ya in ((1, 1 + nc), (2 + nc, 1)):  # Y right behind X; Y before X with a column between
            big = np.full((fx.n, 2 * nc + 3), 3.5)
            big[:, xa:xa + nc] = X
            P = dev(ctx, big)
            lu.solve(P.view(xa, xa + nc - 1), Y=P.view(ya, ya + nc - 1), trans=trans)
            expect = big.copy()
            expect[:, ya:ya + nc] = Y0
            assert same_bits(P.to_host(), expect), (trans, xa, ya)
        for xa, ya in ((1, 2), (2, 1), (1, 1), (1, nc), (nc, 1)):  # by one column, the same window, by the last column
            big = np.full((fx.n, 2 * nc + 3), 3.5)
            big[:, xa:xa + nc] = X
            P = dev(ctx, big)
            with pytest.raises(rails_amd.RailsError, match="alias"):
                lu.solve(P.view(xa, xa + nc - 1), Y=P.view(ya, ya + nc - 1), trans=trans)
            assert same_bits(P.to_host(), big), (trans, xa, ya)
    lu.close()


def test_workspace_grows_and_stays(ctx, cases):
    """after a 130-column solve a 3-column solve on the same object is bitwise that of a fresh object (the workspace's leading
    dimension is no part of the arithmetic), and workspace_columns never shrinks"""
    case = cases["bordered"]
    used, fresh = make_lu(ctx, case.fx), make_lu(ctx, case.fx)
    assert used.stats()["workspace_columns"] == 0
    used.solve(dev(ctx, case.X[:, :130]))
    w130 = used.stats()["workspace_columns"]
    assert w130 >= 130
    for trans in (False, True):
        a = used.solve(dev(ctx, case.X[:, 7:10]), trans=trans).to_host()
        b = fresh.solve(dev(ctx, case.X[:, 7:10]), trans=trans).to_host()
        assert same_bits(a, b), trans
        assert used.stats()["workspace_columns"] == w130 and 3 <= fresh.stats()["workspace_columns"] < 130
    fresh.solve(dev(ctx, case.X[:, :40]))
    w40 = fresh.stats()["workspace_columns"]
    fresh.solve(dev(ctx, case.X[:, :1]))
    assert 40 <= w40 < 130 and fresh.stats()["workspace_columns"] == w40
    used.close()
    fresh.close()


@pytest.mark.parametrize("name", ["blocks1100", "bordered"])
def test_older_path_device_lu(ctx, cases, name):
    """DeviceLU (sptrsv.hip; the Schur operator's A11 solve) on the same factors at 1 and 40 columns.  A level goes to k_sptrsv_level
    when rows * columns exceed 1024 and to the one-workgroup chain otherwise: the 1100-row levels are launches of their own at either
    width, the bordered matrix's narrower levels change sides between 1 and 40 columns and its border rows stay a chain
    (test_lu_fixtures_host.py).  Same reference, same rule for the bound."""
    import rails_amd
    from rails_amd.schur import DeviceLU

    case = cases[name]
    fx = case.fx
    bound = ORDER_FACTOR * case.host_error()
    dlu = DeviceLU(ctx, fx)
    for trans in (False, True):
        for nc in (1, 40):
            B = dev(ctx, case.X[:, :nc])
            tmp, out = rails_amd.HipMultiVectorWrapper(ctx, fx.n, nc), rails_amd.HipMultiVectorWrapper(ctx, fx.n, nc)
            dlu.solve(B, tmp, out, trans=trans)
            err = case.error(out.to_host(), trans, nc)
            print("DeviceLU %s trans=%d nc=%d: device error %.3e, bound %.3e" % (name, trans, nc, err, bound))
            assert err <= bound, (name, trans, nc, err, bound)
            assert same_bits(B.to_host(), case.X[:, :nc])
    dlu.close()
