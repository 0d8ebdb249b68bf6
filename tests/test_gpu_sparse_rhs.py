"""The sparse right-hand side on the device: rails_sprhs_apply in both directions against scipy under a componentwise bound, and
rails_resid_lanczos_sparse checked step by step from the device's own stored vectors against the longdouble reference and the derived
bounds of tests/lanczos_reference.py (with parts["B"] = B.toarray(): a sparse sum has fewer terms than the dense one the bounds were
derived for).  Matrices, cases and the numpy emulation: tests/sparse_rhs_reference.py; tests/test_sparse_rhs_host.py shows on the host
that a correct fp64 implementation stays within a quarter of the bounds and that seeded mistakes exceed them tenfold."""
import ctypes as C

import numpy as np
import pytest

import lanczos_reference as R
import lanczos_steps_device as D
import sparse_rhs_reference as S

pytestmark = pytest.mark.gpu

LD = R.LD
RAILS_EINVAL = -1


@pytest.fixture(scope="module")
def ctx():
    import rails_amd

    c = rails_amd.Context(device=0, seed=4321)
    yield c
    c.close()


def MV(ctx, data=None, **kw):
    import rails_amd

    return rails_amd.HipMultiVectorWrapper(ctx, data=data, **kw)


def sprhs(ctx, Bs):
    import rails_amd

    return rails_amd.SparseRHS.from_scipy(ctx, Bs)


# ----------------------------------------------------------------------------------------------------------- rails_sprhs_apply
APPLY = {"mixed": ("mixed", 741, 300), "selection": ("selection", 330, 200), "wide": ("random3", 63, 130), "one_column": ("dense", 65, 1)}


@pytest.mark.parametrize("name", sorted(APPLY))
def test_apply_both_directions_in_windows(ctx, name):
    """1, 3, 16 and 17 columns at non-zero first columns of NaN-filled panels; |err| <= gamma(row nnz + 2) |B| |X| per entry"""
    form, m, p = APPLY[name]
    Bs = S.make_B(form, m, p, lanczos=True)
    B = sprhs(ctx, Bs)
    assert (B.M(), B.N(), B.nnz()) == (m, p, Bs.nnz)
    assert ctx.lib.rails_csr_rows(B.op.h.h) == m and ctx.lib.rails_csr_cols(B.op.h.h) == p
    rng = np.random.default_rng(5)
    worst = 0.0
    for trans, Op in ((False, Bs), (True, Bs.T.tocsr())):
        xr, yr = Op.shape[1], Op.shape[0]
        nnz_row = np.diff(Op.indptr)
        Oabs = abs(Op)
        for nc, xc0, yc0 in ((1, 2, 5), (3, 3, 0), (16, 4, 7), (17, 1, 6)):
            Xh = np.full((xr, 32), np.nan)
            Xh[:, xc0:xc0 + nc] = rng.uniform(-1, 1, (xr, nc))
            X, Y = MV(ctx, data=Xh, capacity=32), MV(ctx, data=np.full((yr, 32), np.nan), capacity=32)
            Xw, Yw = X._alias(xc0, nc, True), Y._alias(yc0, nc, True)
            if trans == (nc % 2 == 0):  # through the object, and through the operator handle's rails_spmm
                B.apply(Xw, Yw, trans=trans)
            else:
                (B.op.transpose() if trans else B.op).apply(Xw, Yw)
            got = Y.to_host()
            outside = np.ones(32, dtype=bool)
            outside[yc0:yc0 + nc] = False
            assert np.isnan(got[:, outside]).all(), (name, trans, nc)
            Xc = Xh[:, xc0:xc0 + nc]
            want = Op @ Xc
            bound = np.array([R.gamma(n + 2) for n in nnz_row])[:, None] * (Oabs @ np.abs(Xc))
            err = np.abs(got[:, yc0:yc0 + nc] - want)
            assert np.all(err <= bound), (name, trans, nc, float((err - bound).max()))
            worst = max(worst, R._ratio(err, bound))
    print("%s: max |err| / bound = %.3g" % (name, worst))
    B.close()


def test_apply_with_no_columns_and_no_entries(ctx):
    for Bs in (S.make_B("none", 200, 0), S.make_B("mixed", 64, 3, lanczos=True)):  # p = 0; nnz = 0
        m, p = Bs.shape
        B = sprhs(ctx, Bs)
        assert B.nnz() == 0 and B.gram_norm2() == 0.0
        Y = MV(ctx, data=np.full((m, 16), np.nan), capacity=16)
        B.apply(MV(ctx, data=np.ones((p, 2)), capacity=16) if p else MV(ctx, m=0, n=2, capacity=16), Y._alias(4, 2, True))
        got = Y.to_host()
        assert np.all(got[:, 4:6] == 0.0) and np.isnan(got[:, :4]).all() and np.isnan(got[:, 6:]).all()
        Z = B.apply(MV(ctx, data=np.ones((m, 3)), capacity=16), trans=True)
        assert Z.to_host().shape == (p, 3) and np.all(Z.to_host() == 0.0)
        B.close()


def test_refusals(ctx):
    import rails_amd

    Bs = S.make_B("selection", 330, 200)
    B = sprhs(ctx, Bs)
    lib = ctx.lib
    X, Y = MV(ctx, m=200, n=2, capacity=16), MV(ctx, m=330, n=2, capacity=16)
    assert lib.rails_sprhs_apply(ctx.h, B.h, 1, X.panel.h, 0, 2, Y.panel.h, 0) == RAILS_EINVAL  # the shapes of the other direction
    assert lib.rails_sprhs_apply(ctx.h, B.h, 0, X.panel.h, 15, 2, Y.panel.h, 0) == RAILS_EINVAL
    rowptr, col, val = S.csr_arrays(Bs)
    col[7] = 200
    with pytest.raises(rails_amd.RailsError, match="out of range"):
        rails_amd.SparseRHS(ctx, rowptr, col, val, 200)
    two = rails_amd.Context(device=0, seed=1)
    try:
        two.set_partition(0, 2, 0, 660)
        with pytest.raises(rails_amd.RailsError, match="single GPU only"):
            rails_amd.SparseRHS.from_scipy(two, Bs)
    finally:
        two.close()
    B.close()


# ------------------------------------------------------------------------------------------------- rails_resid_lanczos_sparse
def _upload(ctx, c, parts):
    dev = {pn: MV(ctx, data=host, capacity=host.shape[1]) for pn, host in parts["panels"].items()}
    for pn, host in parts["panels"].items():
        assert ctx.lib.rails_panel_ld(dev[pn].panel.h) == host.shape[1]
    return tuple(dev[pn]._alias(c0, c["k"], True) for pn, c0 in (c["av"], c["mv"]))


def _call(ctx, AV, MVw, B, T, L, avc0=None):
    k = AV.n
    T = np.asfortranarray(np.asarray(T, dtype=np.float64).reshape(k, k))
    H = np.full((L + 1, L + 1), np.nan, order="F")
    steps = C.c_int(-1)
    rc = ctx.lib.rails_resid_lanczos_sparse(ctx.h, AV.panel.h, AV.c0 if avc0 is None else avc0, MVw.panel.h, MVw.c0, k, D._ptr(T), max(1, k), B.h, L,
                                            D._ptr(H), L + 1, C.byref(steps))
    return rc, H, steps.value


def _rng_next(ctx):
    seed, nxt = C.c_uint64(0), C.c_uint64(0)
    ctx.lib.rails_ctx_rng_state(ctx.h, C.byref(seed), C.byref(nxt))
    return nxt.value


def _run(ctx, c, parts, windows, B, check=R.check_run):
    from rails_amd._lib import check as ok

    ctx.set_seed(c["seed"], c["stream"])
    before = ctx.stats()["lanczos"]
    rc, H, steps = _call(ctx, windows[0], windows[1], B, parts["T"], c["L"])
    ok(rc, "rails_resid_lanczos_sparse")
    assert _rng_next(ctx) == c["stream"] + 1 and ctx.stats()["lanczos"] == before + 1  # one RNG stream, one run
    assert 1 <= steps <= c["L"] and not np.isnan(H).any()
    Q = D.stored_vectors(ctx, c["m"], steps)
    worst = check(parts, c["L"], H, steps, Q)
    print("%s: steps %d, <%d,%d> on %d blocks, error / bound: alpha %.3g, beta %.3g, r %.3g, norm %.3g" % (
        (S.case_id(c), steps) + D.last_launch(ctx) + (worst["alpha"], worst["beta"], worst["r"], worst["norm"])))
    return dict(H=H, steps=steps, Q=Q, worst=worst)


@pytest.mark.parametrize("c", S.CASES, ids=S.case_id)
def test_every_step_is_within_its_bounds(ctx, c):
    parts = S.make_case(c)
    windows = _upload(ctx, c, parts)
    B = sprhs(ctx, parts["Bs"])
    out = _run(ctx, c, parts, windows, B)
    R.assert_within(out["worst"], 1.0, S.case_id(c))
    assert D.last_launch(ctx)[:2] == D.expected_kernel(c["k"])
    # the same seed again: every reduction has a fixed order, so H and the vectors come back bit for bit
    again = _run(ctx, c, parts, windows, B)
    assert again["steps"] == out["steps"] and np.array_equal(again["H"], out["H"]) and np.array_equal(again["Q"], out["Q"])
    if c["p"] <= 128:  # the dense kernel on B.toarray() passes the same bounds; the two differ in their order of summation only
        Bd = MV(ctx, data=parts["B"], capacity=R.pad16(c["p"])) if c["p"] else MV(ctx, m=c["m"], n=0, capacity=16)
        dense = D.run_parts(ctx, windows + (Bd._alias(0, c["p"], True),), parts, c["L"], c["seed"], c["stream"])
        R.assert_within(dense["worst"], 1.0, S.case_id(c) + " (dense kernel)")
        assert dense["steps"] == out["steps"]
    B.close()


def test_grid_stride_loop_makes_a_second_trip(ctx):
    """more row groups than waves in the grid, 1000 columns of one entry; the dense form of this B would not fit, so the reference
    takes the products with B from its entries (sparse_rhs_reference.check_run_sparse: the same formulas and bounds)"""
    c = S.GRID_STRIDE
    parts = R.make_case(dict(c, p=0))
    parts["Bs"] = S.make_B(c["form"], c["m"], c["p"])
    del parts["B"]
    windows = _upload(ctx, c, parts)
    B = sprhs(ctx, parts["Bs"])
    out = _run(ctx, c, parts, windows, B, check=S.check_run_sparse)
    R.assert_within(out["worst"], 1.0, "grid_stride")
    nch, unroll, nblocks = D.last_launch(ctx)
    assert (c["m"] + 63) // 64 > 4 * nblocks and out["steps"] == c["L"]
    B.close()


def test_breakdown_with_no_panels_and_a_zero_B(ctx):
    """k = 0 and B = 0: R = 0, the first beta is zero and the run stops at step 1 with H = 0"""
    m = 64
    B = sprhs(ctx, S.make_B("mixed", m, 3, lanczos=True))  # every row emptied: three columns, no entries
    empty = (MV(ctx, data=np.full((m, 16), np.nan), capacity=16)._alias(0, 0, True), MV(ctx, data=np.full((m, 16), np.nan), capacity=16)._alias(0, 0, True))
    rc, H, steps = _call(ctx, empty[0], empty[1], B, np.zeros((0, 0)), 4)
    assert rc == 0 and steps == 1 and not H.any()
    Q = D.stored_vectors(ctx, m, 1)
    assert abs(float(Q[:, 0].astype(LD) @ Q[:, 0].astype(LD)) - 1.0) <= R.gamma(m + 8)
    B.close()


def test_lanczos_refusals_launch_nothing(ctx):
    import rails_amd

    c = S.CASES[0]
    parts = S.make_case(c)
    AV, MVw = _upload(ctx, c, parts)
    B = sprhs(ctx, parts["Bs"])
    before = (ctx.stats()["lanczos"], _rng_next(ctx))
    rc, H, steps = _call(ctx, AV, MVw, B, parts["T"], c["L"], avc0=1)
    assert rc == RAILS_EINVAL and "even columns" in ctx.lib.rails_last_error().decode() and np.isnan(H).all() and steps == -1
    short = MV(ctx, m=c["m"] - 1, n=c["k"], capacity=16)
    rc, H, steps = _call(ctx, AV, short, B, parts["T"], c["L"])
    assert rc == RAILS_EINVAL and "row mismatch" in ctx.lib.rails_last_error().decode()
    other = rails_amd.Context(device=0, seed=1)
    try:
        AV2, MV2 = MV(other, data=parts["AV"], capacity=16), MV(other, data=parts["MV"], capacity=16)
        rc, H, steps = _call(other, AV2, MV2, B, parts["T"], c["L"])
        assert rc == RAILS_EINVAL and "single GPU only" in other.lib.rails_last_error().decode()
    finally:
        other.close()
    assert (ctx.stats()["lanczos"], _rng_next(ctx)) == before
    B.close()
