"""rails_panel_rowquad = diag(U S U') (rails_amd/csrc/solution.hip) at every instantiation k_panel_rowquad<TR>, every slice pair and the
edges of its chunks, tiles, slices and workgroups, against tests/solution_reference.py: exact integer cases, the derived bound
8 k eps (|U||S||U|')_ii against longdouble, windows of poisoned panels, a context whose workspace and staging buffers hold an earlier
call's data, and rows that must not notice where in the launch they sit.  rails_panel_rowquad_last_plan says which instantiations ran;
after every call it must be what the restated slice rule gives."""
import ctypes as C

import numpy as np
import pytest

import solution_reference as R

pytestmark = pytest.mark.gpu

_i32p = C.POINTER(C.c_int32)


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


def _call(ctx, Ud, c0, k, S, out, oc0=0, lds=None):
    """one rails_panel_rowquad; the plan it reports must be the restated rule's"""
    from rails_amd._lib import check
    from rails_amd.wrappers import _p

    Sf = np.asfortranarray(S if k else np.zeros((1, 1)))
    check(ctx.lib.rails_panel_rowquad(ctx.h, Ud.panel.h, c0, k, _p(Sf), lds or max(1, k), out.panel.h, oc0), "rails_panel_rowquad")
    plan = _plan(ctx)
    assert plan == [tr for _, _, tr in R.slice_rule(k)], (k, plan)
    return plan


def _rowquad(ctx, U, S):
    m, k = U.shape
    Ud = MV(ctx, data=U) if k else MV(ctx, m=m, n=0)
    out = MV(ctx, data=np.full((m, 1), 7.0))
    plan = _call(ctx, Ud, 0, k, S, out)
    return out.to_host()[:, 0], plan


def test_last_plan_before_any_call_and_its_arguments():
    import rails_amd

    fresh = rails_amd.Context(device=0, seed=1)
    assert _plan(fresh) == []
    U, S, _ = R.exact_case(17, 257)
    _rowquad(fresh, U, S)
    n, tr = C.c_int(-1), (C.c_int * 2)(-5, -5)
    assert fresh.lib.rails_panel_rowquad_last_plan(fresh.h, C.byref(n), tr, 1) == 0  # room for one: the second is not written
    assert (n.value, tr[0], tr[1]) == (2, 12, -5)
    assert fresh.lib.rails_panel_rowquad_last_plan(fresh.h, C.byref(n), None, 0) == 0 and n.value == 2
    assert fresh.lib.rails_panel_rowquad_last_plan(fresh.h, None, tr, 2) != 0
    _rowquad(fresh, *R.exact_case(17, 0)[:2])
    assert _plan(fresh) == []  # k = 0 launches no slice
    fresh.close()


@pytest.mark.parametrize("k", R.K_LIST)
def test_exact_integer_cases(ctx, k):
    for m in R.exact_ms(k):
        U, S, want = R.exact_case(m, k)
        got, plan = _rowquad(ctx, U, S)
        print("exact m = %d, k = %d: TR per slice %s" % (m, k, plan))
        assert np.array_equal(got, want.astype(np.float64)), (m, k, np.flatnonzero(got != want)[:8])


@pytest.mark.parametrize("k", R.SINGLE_ENTRY_K)
def test_single_entry_of_s(ctx, k):
    """S[a, b] = 1 and nothing else: out_i = U[i, a] U[i, b], one rounding (every other term is a zero), whatever U holds"""
    m = 129
    U = np.random.default_rng(k).standard_normal((m, k)) * 10.0 ** np.random.default_rng(k + 1).uniform(-3, 3, (m, 1))
    Ud, out = MV(ctx, data=U), MV(ctx, data=np.full((m, 1), 7.0))
    for a, b in R.single_entry_pairs(k):
        S = np.zeros((k, k))
        S[a, b] = 1.0
        _call(ctx, Ud, 0, k, S, out)
        got = out.to_host()[:, 0]
        assert np.array_equal(got, U[:, a] * U[:, b]), (k, a, b, np.flatnonzero(got != U[:, a] * U[:, b])[:8])


@pytest.mark.parametrize("k", R.K_LIST)
def test_bounded_against_longdouble(ctx, k):
    U, S, want, bound = R.bounded_case(R.BOUNDED_M, k)
    got, plan = _rowquad(ctx, U, S)
    err = np.abs(np.asarray(got - want, dtype=np.float64))
    ratio = (err / bound).max() if k else 0.0
    print("bounded m = %d, k = %d: TR per slice %s, max |err| / bound = %.3g" % (R.BOUNDED_M, k, plan, ratio))
    assert np.all(np.isfinite(got)) and np.all(err <= bound), ratio


@pytest.mark.parametrize("c0", R.WINDOW_C0)
def test_windows_of_poisoned_panels(ctx, c0):
    """U is columns [c0, c0 + k) of a wider panel (an odd c0 takes the scalar loads) whose other columns are NaN, S has leading dimension
    k + 3 with NaN in the padding rows, the result goes to column 2 of a 5-column panel of sevens"""
    for m, k in R.WINDOW_CASES:
        U, S, want, bound = R.bounded_case(m, k)
        wide = np.full((m, c0 + k + 6), np.nan)
        wide[:, c0:c0 + k] = U
        Spad = np.full((k + 3, k), np.nan, order="F")
        Spad[:k] = S
        Wd, out = MV(ctx, data=wide), MV(ctx, data=np.full((m, 5), 7.0))
        _call(ctx, Wd, c0, k, Spad, out, oc0=2, lds=k + 3)
        got = out.to_host()
        err = np.abs(np.asarray(got[:, 2] - want, dtype=np.float64))
        print("window c0 = %d, m = %d, k = %d: max |err| / bound = %.3g" % (c0, m, k, (err / bound).max()))
        assert np.all(np.isfinite(got[:, 2])) and np.all(err <= bound)
        assert np.all(got[:, [0, 1, 3, 4]] == 7.0)
        assert np.array_equal(R.bits(Wd.to_host()), R.bits(wide))  # the input panel is as it was


def test_stale_workspace_and_staging():
    """One context runs k = 500, 33, 300, 5 -- the packed-S workspace and the staged S shrink and grow under data of the call before --
    then a row move (its indices go through the same staging buffers) and another rowquad back to back with no synchronisation
    between them.  Every result is bitwise what a fresh context gives for that call alone."""
    import rails_amd
    from rails_amd._lib import check

    m = 300
    cases = [R.kernel_case(np.random.default_rng(60 + k), m, k) for k in R.STALE_SEQUENCE + (33,)]

    def alone(U, S):
        fresh = rails_amd.Context(device=0, seed=1)
        got, _ = _rowquad(fresh, U, S)
        fresh.close()
        return got

    want = [alone(U, S) for U, S in cases]
    one = rails_amd.Context(device=0, seed=1)
    for (U, S), w in zip(cases[:-1], want):
        got, plan = _rowquad(one, U, S)
        assert np.array_equal(R.bits(got), R.bits(w)), (U.shape[1], plan)
    # row move, then rowquad, queued without a synchronisation in between (the uploads and the panels are made before)
    X = R.special_data(np.random.default_rng(9), m, 6)
    idx = np.array([299, 0, 17, 17, 128, 5, 299], dtype=np.int32)
    Xd, Yd = MV(one, data=X), MV(one, data=np.full((7, 6), 7.0))
    U, S = cases[-1]
    Ud, out = MV(one, data=U), MV(one, data=np.full((m, 1), 7.0))
    one.sync()
    check(one.lib.rails_panel_move_rows(one.h, Xd.panel.h, 0, 6, idx.ctypes.data_as(_i32p), idx.size, 0, Yd.panel.h, 0), "rails_panel_move_rows")
    _call(one, Ud, 0, U.shape[1], S, out)
    assert np.array_equal(R.bits(out.to_host()[:, 0]), R.bits(want[-1]))
    assert np.array_equal(R.bits(Yd.to_host()), R.bits(X[idx]))
    one.close()


@pytest.mark.parametrize("k", [33, 129, 300])
def test_a_row_does_not_notice_its_place_in_the_launch(ctx, k):
    """solution.hip: "the result does not depend on the launch".  The same 16 rows as a panel of their own, at rows 5..20 of a panel of
    300 rows (across two wave tiles), as its last 16 rows (the ragged last workgroup), and in reverse order: the same 16 bit patterns"""
    g = np.random.default_rng(700 + k)
    rows, S = R.kernel_case(g, 16, k)
    own, _ = _rowquad(ctx, rows, S)
    big = R.kernel_case(g, 300, k)[0]
    big[5:21] = rows
    big[284:] = rows
    emb, _ = _rowquad(ctx, big, S)
    rev, _ = _rowquad(ctx, rows[::-1].copy(), S)
    assert np.array_equal(R.bits(emb[5:21]), R.bits(own))
    assert np.array_equal(R.bits(emb[284:]), R.bits(own))
    assert np.array_equal(R.bits(rev[::-1]), R.bits(own))
    err = np.abs(np.asarray(own - R.rowquad(rows, S), dtype=np.float64))
    assert np.all(err <= R.rowquad_bound(rows, S))
