"""rails_panel_rowpair, out[i] = U[ia[i],:] S U[ib[i],:]' = X[ia[i], ib[i]] (rails_amd/csrc/solution.hip: the body of k_panel_rowquad<TR> on
gathered rows), at every instantiation, slice pair and chunk edge, against tests/covariance_reference.py: exact integer cases over the
index patterns, bit-for-bit agreement with rails_panel_rowquad on identity indices, the derived bound 8 k eps (|U_a||S||U_b|') against
longdouble, pairs that must not notice where in the launch they sit, poisoned neighbours, stale context buffers, and the refusals."""
import ctypes as C

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


def MV(ctx, data=None, **kw):
    import rails_amd

    return rails_amd.HipMultiVectorWrapper(ctx, data=data, **kw)


def _plan(ctx):
    n, tr = C.c_int(-1), (C.c_int * 4)(-1, -1, -1, -1)
    assert ctx.lib.rails_panel_rowquad_last_plan(ctx.h, C.byref(n), tr, 4) == 0
    return [tr[q] for q in range(n.value)]


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_i32p)


def _raw(ctx, Ud, c0, k, S, ia, ib, n, out, oc0=0, lds=None):
    from rails_amd.wrappers import _p

    Sf = np.asfortranarray(S if k else np.zeros((1, 1)))
    return ctx.lib.rails_panel_rowpair(ctx.h, Ud.panel.h, c0, k, _p(Sf), lds or max(1, k), _ptr(ia), _ptr(ib), n, out.panel.h, oc0)


def _call(ctx, Ud, c0, k, S, ia, ib, n, out, oc0=0, lds=None):
    """one rails_panel_rowpair; the plan it reports must be the restated rule's (none when nothing is launched)"""
    from rails_amd._lib import check

    check(_raw(ctx, Ud, c0, k, S, ia, ib, n, out, oc0, lds), "rails_panel_rowpair")
    plan = _plan(ctx)
    assert plan == ([tr for _, _, tr in R.slice_rule(k)] if n and Ud.M() else []), (k, n, plan)
    return plan


def _rowpair(ctx, Ud, k, S, ia, ib, n, extra=3):
    """the n results and the `extra` rows behind them, which must keep their sevens"""
    out = MV(ctx, data=np.full((n + extra, 1), 7.0))
    plan = _call(ctx, Ud, 0, k, S, ia, ib, n, out)
    got = out.to_host()[:, 0]
    assert np.all(got[n:] == 7.0)
    return got[:n], plan


def _panel(ctx, U):
    m, k = U.shape
    return MV(ctx, data=U) if k else MV(ctx, m=m, n=0)


def test_the_sentinel_code():
    import rails_amd

    assert EINVAL == rails_amd.load().rails_panel_rowpair(None, None, 0, 0, None, 0, None, None, 0, None, 0)


@pytest.mark.parametrize("k", R.K_LIST)
def test_exact_integer_cases(ctx, k):
    for m in CR.PAIR_MS:
        U, S, _ = R.exact_case(m, k)
        Ud = _panel(ctx, U)
        for n in CR.pair_ns(m):
            for name in CR.PATTERNS:
                ia, ib, nn = CR.pattern(name, m, n)
                got, plan = _rowpair(ctx, Ud, k, S, ia, ib, nn)
                want = CR.exact_pairs(U, S, ia, ib, nn).astype(np.float64)
                assert np.array_equal(got, want), (m, k, nn, name, plan, np.flatnonzero(got != want)[:8])


@pytest.mark.parametrize("k", R.K_LIST)
def test_identity_indices_give_rowquads_bits(ctx, k):
    """both indices the identity, as arrays and as NULL: the bits of rails_panel_rowquad for a random real U, at every TR"""
    from rails_amd._lib import check
    from rails_amd.wrappers import _p

    m = 300
    U, S = R.kernel_case(np.random.default_rng(90 + k), m, k)
    Ud = _panel(ctx, U)
    ref = MV(ctx, data=np.full((m, 1), 7.0))
    Sf = np.asfortranarray(S if k else np.zeros((1, 1)))
    check(ctx.lib.rails_panel_rowquad(ctx.h, Ud.panel.h, 0, k, _p(Sf), max(1, k), ref.panel.h, 0), "rails_panel_rowquad")
    quad_plan, want = _plan(ctx), ref.to_host()[:, 0]
    i = np.arange(m, dtype=np.int32)
    for ia, ib in ((i, i), (None, None), (i, None), (None, i)):
        got, plan = _rowpair(ctx, Ud, k, S, ia, ib, m)
        assert plan == quad_plan
        assert np.array_equal(R.bits(got), R.bits(want)), (k, plan, ia is None, ib is None)


@pytest.mark.parametrize("k", R.K_LIST)
def test_bounded_against_longdouble(ctx, k):
    m = R.BOUNDED_M
    U, S = CR.pair_problem(m, k)  # S not symmetric: X[a, b] != X[b, a]
    Ud = _panel(ctx, U)
    for name in ("differ", "reversed", "ia_null"):
        ia, ib, n = CR.pattern(name, m, 2 * m)
        got, plan = _rowpair(ctx, Ud, k, S, ia, ib, n)
        want, bound = CR.pairs(U, S, ia, ib, n), CR.pairs_bound(U, S, ia, ib, n)
        err = np.abs(np.asarray(got - want, dtype=np.float64))
        ratio = (err / bound).max() if k else 0.0
        print("bounded %s m = %d, k = %d, n = %d: TR per slice %s, max |err| / bound = %.3g" % (name, m, k, n, plan, ratio))
        assert np.all(np.isfinite(got)) and np.all(err <= bound), ratio
    if k > 1:  # the form is that of S as given: swapping the indices gives another number
        ia, ib, n = CR.pattern("differ", m, 2 * m)
        swapped, _ = _rowpair(ctx, Ud, k, S, ib, ia, n)
        assert np.all(np.abs(np.asarray(swapped - CR.pairs(U, S, ib, ia, n), dtype=np.float64)) <= CR.pairs_bound(U, S, ib, ia, n))
        assert not np.array_equal(swapped, _rowpair(ctx, Ud, k, S, ia, ib, n)[0])


@pytest.mark.parametrize("k", [33, 129, 300])
def test_a_pair_does_not_notice_its_place_or_the_call(ctx, k):
    """the same 16 pairs as a call of their own, at positions 5..20 of 300 pairs (across two wave tiles), as the last 16 of 300 (the ragged
    last workgroup), reversed, in a call of 17 and with the other pairs' rows different: the same 16 bit patterns"""
    m = 200
    g = np.random.default_rng(800 + k)
    U, S = CR.pair_problem(m, k)
    Ud = _panel(ctx, U)
    pa, pb = g.integers(0, m, 16).astype(np.int32), g.integers(0, m, 16).astype(np.int32)
    own, _ = _rowpair(ctx, Ud, k, S, pa, pb, 16)
    ia, ib = g.integers(0, m, 300).astype(np.int32), g.integers(0, m, 300).astype(np.int32)
    for at in (5, 284):
        ia[at:at + 16], ib[at:at + 16] = pa, pb
    emb, _ = _rowpair(ctx, Ud, k, S, ia, ib, 300)
    rev, _ = _rowpair(ctx, Ud, k, S, pa[::-1].copy(), pb[::-1].copy(), 16)
    one_more, _ = _rowpair(ctx, Ud, k, S, np.concatenate([[m - 1], pa]).astype(np.int32), np.concatenate([[0], pb]).astype(np.int32), 17)
    assert np.array_equal(R.bits(emb[5:21]), R.bits(own))
    assert np.array_equal(R.bits(emb[284:]), R.bits(own))
    assert np.array_equal(R.bits(rev[::-1]), R.bits(own))
    assert np.array_equal(R.bits(one_more[1:]), R.bits(own))
    err = np.abs(np.asarray(own - CR.pairs(U, S, pa, pb), dtype=np.float64))
    assert np.all(err <= CR.pairs_bound(U, S, pa, pb))


@pytest.mark.parametrize("c0", R.WINDOW_C0)
def test_windows_of_poisoned_panels(ctx, c0):
    """U is columns [c0, c0 + k) of a wider panel (an odd c0 takes the scalar loads) whose other columns are NaN, S has leading dimension
    k + 3 with NaN in the padding rows; the result goes to column 2 of a 5-column panel of sevens with more rows than pairs"""
    for m, k in R.WINDOW_CASES:
        U, S = CR.pair_problem(m, k)
        ia, ib, n = CR.pattern("differ", m, 100)
        wide = np.full((m, c0 + k + 6), np.nan)
        wide[:, c0:c0 + k] = U
        Spad = np.full((k + 3, k), np.nan, order="F")
        Spad[:k] = S
        Wd, out = MV(ctx, data=wide), MV(ctx, data=np.full((n + 30, 5), 7.0))
        _call(ctx, Wd, c0, k, Spad, ia, ib, n, out, oc0=2, lds=k + 3)
        got = out.to_host()
        want, bound = CR.pairs(U, S, ia, ib), CR.pairs_bound(U, S, ia, ib)
        err = np.abs(np.asarray(got[:n, 2] - want, dtype=np.float64))
        print("window c0 = %d, m = %d, k = %d: max |err| / bound = %.3g" % (c0, m, k, (err / bound).max()))
        assert np.all(np.isfinite(got[:n, 2])) and np.all(err <= bound)
        assert np.all(got[:, [0, 1, 3, 4]] == 7.0) and np.all(got[n:, 2] == 7.0)
        assert np.array_equal(R.bits(Wd.to_host()), R.bits(wide))  # the input panel is as it was
        # the output column in U's own panel, outside the window
        _call(ctx, Wd, c0, k, Spad, ia, ib, n, Wd, oc0=c0 + k + 1, lds=k + 3)
        back = Wd.to_host()
        assert np.array_equal(R.bits(back[:n, c0 + k + 1]), R.bits(got[:n, 2]))
        assert np.all(np.isnan(back[n:, c0 + k + 1])) and np.array_equal(R.bits(back[:, c0:c0 + k]), R.bits(U))


def test_k_zero_and_empty_calls(ctx):
    U = np.ones((20, 3))
    Ud, E = MV(ctx, data=U), MV(ctx, m=20, n=0)
    i = np.arange(9, dtype=np.int32)
    out = MV(ctx, data=np.full((12, 2), 7.0))
    _call(ctx, E, 0, 0, None, i, i, 9, out, oc0=1)  # k = 0: zeros in the n rows of that column, nothing else
    got = out.to_host()
    assert np.all(got[:9, 1] == 0.0) and np.all(got[9:, 1] == 7.0) and np.all(got[:, 0] == 7.0)
    assert _plan(ctx) == []
    out = MV(ctx, data=np.full((12, 2), 7.0))
    _call(ctx, Ud, 0, 3, np.eye(3), i, i, 0, out)  # n = 0
    none = MV(ctx, m=0, n=3)
    _call(ctx, none, 0, 3, np.eye(3), None, None, 0, out)  # a panel without rows
    assert np.all(out.to_host() == 7.0) and _plan(ctx) == []


def test_stale_workspace_and_staging():
    """One context runs k = 500, 33, 300, 5 with shrinking and growing index arrays -- the packed-S workspace, the staged S and the staged
    indices lie under data of the call before -- then a row move (its indices use the same staging buffers) and another rowpair back to
    back without a synchronisation.  Every result is bitwise what a fresh context gives for that call alone."""
    import rails_amd
    from rails_amd._lib import check

    m = 300
    ns = (600, 17, 300, 1000, 40)
    cases = []
    for k, n in zip(R.STALE_SEQUENCE + (33,), ns):
        U, S = CR.pair_problem(m, k)
        ia, ib, _ = CR.pattern("differ", m, n, seed=k)
        cases.append((U, S, ia, ib, n))

    def run(c, case):
        U, S, ia, ib, n = case
        return _rowpair(c, _panel(c, U), U.shape[1], S, ia, ib, n)[0]

    def alone(case):
        fresh = rails_amd.Context(device=0, seed=1)
        got = run(fresh, case)
        fresh.close()
        return got

    want = [alone(case) for case in cases]
    one = rails_amd.Context(device=0, seed=1)
    for case, w in zip(cases[:-1], want):
        assert np.array_equal(R.bits(run(one, case)), R.bits(w)), (case[0].shape[1], case[4])
    X = R.special_data(np.random.default_rng(9), m, 6)
    idx = np.array([299, 0, 17, 17, 128, 5, 299], dtype=np.int32)
    Xd, Yd = MV(one, data=X), MV(one, data=np.full((7, 6), 7.0))
    U, S, ia, ib, n = cases[-1]
    Ud, out = MV(one, data=U), MV(one, data=np.full((n, 1), 7.0))
    one.sync()
    check(one.lib.rails_panel_move_rows(one.h, Xd.panel.h, 0, 6, idx.ctypes.data_as(_i32p), idx.size, 0, Yd.panel.h, 0), "rails_panel_move_rows")
    _call(one, Ud, 0, U.shape[1], S, ia, ib, n, out)
    assert np.array_equal(R.bits(out.to_host()[:, 0]), R.bits(want[-1]))
    assert np.array_equal(R.bits(Yd.to_host()), R.bits(X[idx]))
    one.close()


def test_refusals_write_nothing(ctx):
    m, k = 40, 9
    U, S = CR.pair_problem(m, k)
    wide = np.full((m, k + 2), 7.0)
    wide[:, :k] = U
    Wd = MV(ctx, data=wide)
    out = MV(ctx, data=np.full((30, 2), 7.0))
    good = np.arange(20, dtype=np.int32)

    def refused(rc):
        assert rc == EINVAL, rc
        assert ctx.lib.rails_last_error()
        assert np.all(out.to_host() == 7.0) and np.array_equal(R.bits(Wd.to_host()), R.bits(wide))

    for bad in (-1, m):
        for pos in (0, 19):
            idx = good.copy()
            idx[pos] = bad
            refused(_raw(ctx, Wd, 0, k, S, idx, good, 20, out))
            refused(_raw(ctx, Wd, 0, k, S, good, idx, 20, out))
            refused(_raw(ctx, Wd, 0, k, S, None, idx, 20, out))
    big = np.zeros(31, dtype=np.int32)
    refused(_raw(ctx, Wd, 0, k, S, big, big, 31, out))  # more pairs than Out has rows
    tall = MV(ctx, data=np.full((m + 5, 1), 7.0))
    idx = np.zeros(m + 1, dtype=np.int32)
    for ia, ib in ((None, idx), (idx, None), (None, None)):  # a NULL index with n > m
        assert _raw(ctx, Wd, 0, k, S, ia, ib, m + 1, tall) == EINVAL
    assert np.all(tall.to_host() == 7.0)
    for oc0 in (0, k - 1):  # an output column inside the window of the same panel
        refused(_raw(ctx, Wd, 0, k, S, good, good, 20, Wd, oc0=oc0))
    refused(_raw(ctx, Wd, 0, k, S, good, good, -1, out))
    # and the column next to the window is fine
    from rails_amd._lib import check

    check(_raw(ctx, Wd, 0, k, S, good, good, 20, Wd, oc0=k), "rails_panel_rowpair")
    got = Wd.to_host()
    err = np.abs(np.asarray(got[:20, k] - CR.pairs(U, S, good, good), dtype=np.float64))
    assert np.all(err <= CR.pairs_bound(U, S, good, good)) and np.all(got[20:, k] == 7.0) and np.all(got[:, k + 1] == 7.0)


def test_python_entry_points(ctx):
    """HipMultiVectorWrapper.rowpair beside rowquad, and Solution.covariance / std on top of them"""
    import rails_amd

    m, k = 129, 33
    U, S = CR.corr_problem(m, k)
    Ud = MV(ctx, data=U)
    ia, ib, n = CR.pattern("differ", m, 2 * m)
    got = Ud.rowpair(S, ia.astype(np.int64), ib).to_host()[:, 0]  # int64 input is converted, not reinterpreted
    assert np.all(np.abs(np.asarray(got - CR.pairs(U, S, ia, ib), dtype=np.float64)) <= CR.pairs_bound(U, S, ia, ib))
    assert np.array_equal(R.bits(Ud.rowpair(S, None, None).to_host()), R.bits(Ud.rowquad(S).to_host()))
    with pytest.raises(IndexError, match="ia: index %d at position 0" % m):
        Ud.rowpair(S, np.array([m]), np.array([0]))
    with pytest.raises(TypeError):
        Ud.rowpair(S, np.array([0.5]), np.array([0]))
    with pytest.raises(ValueError, match="1 indices in ia, 2 in ib"):
        Ud.rowpair(S, np.array([0]), np.array([0, 1]))
    sol = rails_amd.Solution(ctx, Ud, S)
    cov = sol.covariance(ia, ib)
    assert np.array_equal(R.bits(cov), R.bits(got))
    assert np.array_equal(R.bits(sol.covariance(ia, ib, fetch=False).to_host()[:, 0]), R.bits(got))
    half = sol.covariance(None, ib[:m])
    assert np.all(np.abs(np.asarray(half - CR.pairs(U, S, None, ib[:m]), dtype=np.float64)) <= CR.pairs_bound(U, S, None, ib[:m]))
    v = sol.variance()
    assert np.array_equal(sol.std(), np.sqrt(np.where(v > 0, v, 0.0)))
    assert np.array_equal(sol.std(fetch=False).to_host()[:, 0], sol.std())
    with pytest.raises(ValueError):
        sol.covariance(None, None)
    with pytest.raises(IndexError):
        sol.covariance(np.array([-1]), np.array([0]))
    sol.close()
