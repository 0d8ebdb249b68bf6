"""The smoothed-aggregation multigrid preconditioner of the iterative A^-1 operator (include/rails_hip.h: "amg", rails_iter_amg_setup,
rails_iter_amg_info; rails_amd/csrc/amg_host.cpp and iter_hierarchy.hip for the set-up, itsolve.hip: Run::vcycle on the sweeps plan_call made, iter_kernels.inc:
k_amg_residual_csr, k_amg_prolong_add, k_amg_coarse_dense) on the GPU against the restatement of tests/amg_reference.py: one cycle against a longdouble evaluation on the shapes
at which the kernels take their different paths, the preconditioned solves against the restatement's iteration counts, "amg" 0 bit for
bit, determinism, the counts per cycle of DESIGN.md section 16, and the refusals."""
import numpy as np
import pytest

import amg_reference as M
import cheb_reference as C
import iter_reference as R

pytestmark = pytest.mark.gpu

TOL = 1e-10
EPS = np.finfo(float).eps
WIDTHS = (1, 2, 17, 32, 33, 70)  # 8 lanes per row up to 16 columns, 16 above; odd last columns and the pad column; two groups of 32 and a tail
DEGREES = (0, 1, 2)              # no smoother step beyond the first, and both parities of the fused step's ping-pong
PANEL, XC0, YC0 = 200, 37, 91    # windows at odd columns of panels 200 columns wide
SENTINEL = 7.25
# lap24: three levels, level rows (576, 102, 14) no multiple of 64; lap7_12: second-level rows of 40 entries (blocks of 64 rows beyond the
# 2048 staged entries) and rows of P of 13; the banded ones: rows of 41 and 63 entries, rows of P of 23, either sign; lap9x8: two levels;
# stencil27 and one: no level, the dense kernel alone
PROBLEMS = ["lap24", "lap7_12", "neg_banded41", "banded41", "lap9x8", "stencil27", "one"]


@pytest.fixture(scope="module")
def ctx():
    import rails_amd

    c = rails_amd.Context(device=0, seed=3)
    yield c
    c.close()


_inverses = {}


def inverse(ctx, tag):
    """one IterativeInverse (CG) per problem, shared by the tests of this module, with every setting at a known value and "amg" on"""
    import rails_amd

    A, coarse = M.problem(tag)
    if tag not in _inverses:
        _inverses[tag] = rails_amd.IterativeInverse(ctx, A, method="cg", tol=TOL)
    inv = _inverses[tag]
    for name, value in (("tolerance", TOL), ("jacobi", 1), ("max_iterations", 1000), ("strict", 0), ("check_every", 8), ("poly_degree", 0),
                        ("poly_fused", 1), ("amg_degree", M.DEGREE), ("amg_ratio", M.RATIO), ("amg_theta", M.THETA), ("amg_coarse", coarse), ("amg", 1)):
        inv.set(name, value)
    return inv


@pytest.fixture(scope="module", autouse=True)
def _close_inverses(ctx):
    yield
    for inv in _inverses.values():
        inv.close()
    _inverses.clear()


def window(mv, c0, nc):
    return mv.view(c0, c0 + nc - 1) if nc > 1 else mv.view(c0)


def levels_of(tag):
    return len(M.hierarchy(tag)[1]["levels"])


def cycle_counts(tag, S):
    """per cycle and multigrid level 2 S + 4 kernels of the object (the first smoother step from zero, S steps, the
    residual, the prolongation, 1 + S steps) and 2 S + 4 products (2 S + 2 with A_l, one with P', one with P), plus the dense kernel:
    (launches, products, fused steps)"""
    L = levels_of(tag)
    return L * (2 * S + 4) + 1, L * (2 * S + 4), L * (2 * S + 1)


def test_amg_is_a_setting(ctx):
    """(without the feature: RAILS_EINVAL, "no setting named")"""
    inv = inverse(ctx, "lap9x8")
    inv.set("amg", 1)
    inv.set("amg_degree", 2)
    inv.set("amg_ratio", 5)
    inv.set("amg_theta", 0.1)
    inv.set("amg_coarse", 16)
    A = C.problem("lap9x8")
    Bm = R.rhs(72, 2)
    assert R.true_relres(A, inv.solve_host(Bm), Bm).max() <= 10 * TOL
    info = inv.amg_info()
    assert info["levels"] >= 1 and info["rows"][0] == 72 and info["cycles"] > 0
    assert np.all(inv.columns()[2] == 2)


def test_info_is_the_restatements_hierarchy(ctx):
    for tag in PROBLEMS:
        inv = inverse(ctx, tag)
        info = inv.amg_setup()
        A, h = M.hierarchy(tag)
        assert info["levels"] == len(h["levels"]) + 1 and info["rows"] == M.rows_of(h)
        assert info["nnz"] == [lv["A"].nnz for lv in h["levels"]] + [h["coarse"].nnz]
        for got, lv in zip(info["hi"], h["levels"]):
            assert abs(got - lv["hi"]) <= 4 * EPS * lv["hi"]
        assert info["hi"][-1] == 0.0 and abs(info["operator_complexity"] - M.operator_complexity(h)) <= 1e-12


_longdouble = {}


def expected(tag, S):
    """the longdouble evaluation of one cycle on a shared input of the widest width (columns are independent: narrower widths take its
    first columns) and the allowed error per column: 4 times the largest error the float64 restatement shows against it, at least
    64 eps ||z||_inf (room for another order of summation within a row)"""
    if (tag, S) not in _longdouble:
        A, h = M.hierarchy(tag)
        Xm = R.rhs(A.shape[0], max(WIDTHS), seed=9)
        Zl = M.vcycle(h, Xm, S, dtype=np.longdouble)
        Z64 = M.vcycle(h, Xm, S)
        bound = np.maximum(4 * np.abs(Z64 - Zl).max(0), 64 * EPS * np.abs(Zl).max(0)).astype(float)
        _longdouble[(tag, S)] = (Xm, Zl, bound)
    return _longdouble[(tag, S)]


def precondition_both_ways(ctx, inv, Xm):
    """on full panels and on windows at odd columns (NaN beside X, sentinels beside Y); returns the two results"""
    import rails_amd

    n, nc = Xm.shape
    X = rails_amd.HipMultiVectorWrapper(ctx, data=Xm)
    full = inv.precondition(X).to_host()
    assert np.array_equal(X.to_host(), Xm)
    big = np.full((n, PANEL), np.nan)
    big[:, XC0:XC0 + nc] = Xm
    Xp = rails_amd.HipMultiVectorWrapper(ctx, data=big)
    Yp = rails_amd.HipMultiVectorWrapper(ctx, data=np.full((n, PANEL), SENTINEL))
    inv.precondition(window(Xp, XC0, nc), window(Yp, YC0, nc))
    assert np.array_equal(Xp.to_host(), big, equal_nan=True)
    Yh = Yp.to_host()
    assert np.all(Yh[:, :YC0] == SENTINEL) and np.all(Yh[:, YC0 + nc:] == SENTINEL)
    return full, Yh[:, YC0:YC0 + nc].copy()


@pytest.mark.parametrize("tag", PROBLEMS)
def test_one_cycle_against_longdouble(ctx, tag):
    inv = inverse(ctx, tag)
    worst = 0.0
    for S in DEGREES:
        Xall, Zall, ball = expected(tag, S)
        inv.set("amg_degree", S)
        launches, products, fused_steps = cycle_counts(tag, S)
        for nc in WIDTHS:
            Xm, Zl, bound = np.ascontiguousarray(Xall[:, :nc]), Zall[:, :nc], ball[:nc]
            groups = (nc + 31) // 32
            got = {}
            for fused in (1, 0):
                inv.set("poly_fused", fused)
                full, win = precondition_both_ways(ctx, inv, Xm)
                info, st = inv.amg_info(), inv.stats()
                assert info["cycles"] == groups and info["cycle_launches"] == groups * launches and info["cycle_products"] == groups * products, (info, S, nc)
                assert st["launches"] == groups * launches and st["products"] == groups * products
                assert st["fused_launches"] == (groups * fused_steps if fused else 0), (st, S, nc, fused)
                assert np.array_equal(full, win)  # the same bits through a window
                err = np.abs(full - Zl).astype(float)
                worst = max(worst, (err.max(0) / bound).max())
                assert np.all(err <= bound[None, :]), (tag, nc, S, fused, (err.max(0) / bound).max())
                got[fused] = full
            assert np.all(np.abs(got[1] - got[0]) <= bound[None, :])
    Xm, Zl, _ = expected(tag, 1)
    assert np.all(np.sign((Xm * Zl).sum(0)) == M.hierarchy(tag)[1]["defsign"])  # the cycle has the operator's own sign
    print("problem %s, rows %s: largest error / allowed error %.3f" % (tag, M.rows_of(M.hierarchy(tag)[1]), worst))


def solve_and_check(ctx, tag, nc):
    import rails_amd

    A, Bm, Xr, cr = M.reference(tag, nc)
    inv = inverse(ctx, tag)
    big = np.full((A.shape[0], PANEL), np.nan)
    big[:, XC0:XC0 + nc] = Bm
    Xp = rails_amd.HipMultiVectorWrapper(ctx, data=big)
    Yp = rails_amd.HipMultiVectorWrapper(ctx, data=np.full((A.shape[0], PANEL), SENTINEL))
    inv.solve(window(Xp, XC0, nc), window(Yp, YC0, nc))
    Yh = Yp.to_host()
    assert np.all(Yh[:, :YC0] == SENTINEL) and np.all(Yh[:, YC0 + nc:] == SENTINEL)
    Xg = Yh[:, YC0:YC0 + nc]
    it, rel, flags = inv.columns()
    st, info = inv.stats(), inv.amg_info()
    print("problem %s, %d columns: iterations %d..%d (restatement %d..%d), rows %s, cycles %d, products %d, launches %d" % (
        tag, nc, it.min(), it.max(), cr.iter.min(), cr.iter.max(), info["rows"], info["cycles"], st["products"], st["launches"]))
    assert np.all(np.isfinite(Xg)) and np.all(flags == 2), flags
    assert R.true_relres(A, Xg, Bm).max() <= 10 * TOL
    assert np.all(it <= 1.5 * cr.iter), (it, cr.iter)
    assert st["unconverged_columns"] == 0
    return st, info


@pytest.mark.parametrize("tag,nc", [(t, n) for t in PROBLEMS for n in (3, 33)] + [("lap128", 16)])
def test_preconditioned_solves_match_the_restatement(ctx, tag, nc):
    solve_and_check(ctx, tag, nc)


def test_launch_and_product_counts(ctx):
    """per group of columns a solve that queued q iterations ran q + 1 cycles; outside the cycles the start is 2 launches and an iteration
    6 launches and one product, as with the polynomial; q is a whole number of check_every's: the host reads back only there"""
    for tag, nc, every in (("lap24", 3, 8), ("lap24", 33, 3), ("lap7_12", 16, 8), ("one", 2, 8)):
        A, Bm, _, _ = M.reference(tag, nc)
        inv = inverse(ctx, tag)
        inv.set("check_every", every)
        inv.solve_host(Bm)
        st, info = inv.stats(), inv.amg_info()
        groups = (nc + 31) // 32
        launches, products, fused_steps = cycle_counts(tag, M.DEGREE)
        q = info["cycles"] - groups
        assert q > 0 and info["cycle_launches"] == info["cycles"] * launches and info["cycle_products"] == info["cycles"] * products
        assert st["launches"] - info["cycle_launches"] == 2 * groups + 6 * q
        assert st["products"] - info["cycle_products"] == q
        assert st["fused_launches"] == info["cycles"] * fused_steps
        if groups == 1:
            assert q % every == 0 and q - every < inv.columns()[0].max() <= q


def test_amg_off_is_the_solve_as_it_was(ctx):
    """"amg" 0 after "amg" 1 and a solve with it: the bits, launches and products of an object that never had it"""
    import rails_amd

    A, coarse = M.problem("lap24")
    Bm = R.rhs(A.shape[0], 5)
    for degree in (0, 4):
        for every in (1, 8, 1000):
            results, stats = [], []
            for had_it in (False, True):
                inv = rails_amd.IterativeInverse(ctx, A, method="cg", tol=TOL, check_every=every)
                if had_it:
                    inv.set("amg_coarse", coarse)
                    inv.set("amg", 1)
                    inv.solve_host(Bm)
                    assert inv.amg_info()["cycles"] > 0
                    inv.set("amg", 0)
                inv.set("poly_degree", degree)
                results.append(inv.solve_host(Bm))
                st = inv.stats()
                stats.append({k: st[k] for k in ("launches", "products", "inner_products", "poly_applications", "fused_launches", "max_iterations_of_a_column")})
                assert inv.amg_info()["cycles"] == 0
                inv.close()
            assert np.array_equal(results[0], results[1]), (degree, every)
            assert stats[0] == stats[1], (degree, every, stats)


def test_determinism_and_check_every(ctx):
    import rails_amd

    A, Bm, _, _ = M.reference("lap24", 5)
    inv = inverse(ctx, "lap24")
    X = rails_amd.HipMultiVectorWrapper(ctx, data=Bm)
    results, counts = [], []
    for every in (8, 8, 1, 1000):
        inv.set("check_every", every)
        results.append(inv.solve(X).to_host())
        counts.append(inv.columns()[0].copy())
    for Xg, it in zip(results, counts):
        assert np.array_equal(Xg, results[0])
        assert np.array_equal(it, counts[0])
    assert R.true_relres(A, results[0], Bm).max() <= 10 * TOL
    # a rebuilt hierarchy is the same hierarchy
    inv.amg_setup()
    assert np.array_equal(inv.solve(X).to_host(), results[0])


def test_columns_of_different_speed(ctx):
    A, h = M.hierarchy("lap24")
    Bm = R.rhs(A.shape[0], 4)
    Bm[:, 1] = 0.0
    _, cr = M.pcg(A, Bm, h, tol=TOL)
    assert cr.iter[1] == 0
    inv = inverse(ctx, "lap24")
    Xg = inv.solve_host(Bm)
    it, rel, flags = inv.columns()
    print("iterations", it, "restatement", cr.iter)
    assert it[1] == 0 and np.all(Xg[:, 1] == 0.0)
    assert np.all(it <= 1.5 * cr.iter) and np.all(flags == 2) and np.all(np.isfinite(Xg))
    assert R.true_relres(A, Xg[:, [0, 2, 3]], Bm[:, [0, 2, 3]]).max() <= 10 * TOL


def test_max_iterations_flags_a_column(ctx):
    A, Bm, _, cr = M.reference("lap24", 3)
    inv = inverse(ctx, "lap24")
    inv.set("max_iterations", 3)
    Xg = inv.solve_host(Bm)
    it, rel, flags = inv.columns()
    assert np.all(it == 3) and np.all(flags == 4) and np.all(np.isfinite(Xg)) and cr.iter.min() > 3
    assert inv.stats()["unconverged_columns"] == 3


def test_refusals(ctx):
    import rails_amd

    einval = r"\(code -1\)"
    A, coarse = M.problem("lap24")
    bi = rails_amd.IterativeInverse(ctx, A, method="bicgstab", tol=TOL)
    with pytest.raises(rails_amd.RailsError, match=einval + ".*BiCGStab"):
        bi.set("amg", 1)
    bi.set("amg", 0)  # off is no request
    with pytest.raises(rails_amd.RailsError, match=einval + ".*BiCGStab"):
        bi.amg_setup()
    bi.close()
    with pytest.raises(rails_amd.RailsError, match=einval + ".*BiCGStab"):
        rails_amd.IterativeInverse(ctx, A, method="bicgstab", amg=True)
    # together with the polynomial, in whichever order
    inv = rails_amd.IterativeInverse(ctx, A, method="cg", tol=TOL, poly_degree=2)
    with pytest.raises(rails_amd.RailsError, match=einval + ".*poly_degree"):
        inv.set("amg", 1)
    inv.set("poly_degree", 0)
    inv.set("amg", 1)
    with pytest.raises(rails_amd.RailsError, match=einval + ".*amg"):
        inv.set("poly_degree", 2)
    inv.set("poly_degree", 0)
    for name, bad in (("amg_degree", -1), ("amg_degree", 9), ("amg_degree", 1.5), ("amg_ratio", 1.0), ("amg_ratio", 0.0), ("amg_theta", -0.1), ("amg_theta", 1.0),
                      ("amg_coarse", 0), ("amg_coarse", 1025), ("amg_coarse", 2.5)):
        with pytest.raises(rails_amd.RailsError, match=einval + ".*" + name):
            inv.set(name, bad)
    Bm = R.rhs(A.shape[0], 2)
    assert R.true_relres(A, inv.solve_host(Bm), Bm).max() <= 10 * TOL  # the object still works
    inv.close()
    # a callback operator
    csr_op = rails_amd.HipOperatorWrapper(ctx, A.indptr, A.indices, A.data)

    def action(trans, X, Y):
        csr_op.apply(X, Y)
        return 0

    cb = rails_amd.HipOperatorWrapper.from_callback(ctx, A.shape[0], action)
    inv = rails_amd.IterativeInverse(ctx, cb, method="cg", tol=TOL, diag=A.diagonal())
    with pytest.raises(rails_amd.RailsError, match=einval + ".*callback"):
        inv.set("amg", 1)
    with pytest.raises(rails_amd.RailsError, match=einval + ".*callback"):
        inv.amg_setup()
    inv.close()
    # an iterative solve as the operator
    inner = rails_amd.IterativeInverse(ctx, A, method="cg", tol=TOL)
    outer = rails_amd.IterativeInverse(ctx, inner.op, method="cg", tol=TOL, diag=1.0 / A.diagonal())
    with pytest.raises(rails_amd.RailsError, match=einval + ".*LU or an iterative solve"):
        outer.set("amg", 1)
    outer.close()
    inner.close()
    # a context that reduces: an all-reduce hook
    c2 = rails_amd.Context(device=0, seed=3)
    try:
        c2.set_allreduce(lambda buf, n, stream: 0)  # (one rank: the sums are already complete)
        red = rails_amd.IterativeInverse(c2, rails_amd.HipOperatorWrapper(c2, A.indptr, A.indices, A.data), method="cg", tol=TOL)
        with pytest.raises(rails_amd.RailsError, match=einval + ".*single GPU"):
            red.set("amg", 1)
        red.close()
    finally:
        c2.close()
    # what the set-up refuses: an indefinite matrix, and one that does not coarsen below 1025 rows
    import scipy.sparse as sp

    ind = rails_amd.IterativeInverse(ctx, sp.csr_matrix(np.array([[1.0, 3.0], [3.0, 1.0]])), method="cg", amg=True)
    with pytest.raises(rails_amd.RailsError, match=einval + ".*not definite"):
        ind.amg_setup()
    with pytest.raises(rails_amd.RailsError, match=einval + ".*not definite"):
        ind.solve_host(np.ones((2, 1)))
    ind.close()
    dia = rails_amd.IterativeInverse(ctx, sp.diags(np.arange(1.0, 1101.0)).tocsr(), method="cg", amg=True)
    with pytest.raises(rails_amd.RailsError, match=einval + ".*does not coarsen"):
        dia.precondition(rails_amd.HipMultiVectorWrapper(ctx, data=np.ones((1100, 1))))
    dia.set("amg", 0)
    assert np.allclose(dia.solve_host(np.ones((1100, 1)))[:, 0], 1.0 / np.arange(1.0, 1101.0))
    dia.close()


def test_refuses_an_lu_operator(ctx):
    """rails_iter_create takes an LU handle (with a diagonal given); the multigrid set-up needs the entries of a matrix"""
    import rails_amd

    einval = r"\(code -1\)"
    A, _ = M.problem("lap9x8")
    lu = rails_amd.SparseLU(ctx, A)
    inv = rails_amd.IterativeInverse(ctx, lu.op, method="cg", tol=TOL, diag=1.0 / A.diagonal())
    with pytest.raises(rails_amd.RailsError, match=einval + ".*LU or an iterative solve"):
        inv.set("amg", 1)
    with pytest.raises(rails_amd.RailsError, match=einval + ".*LU or an iterative solve"):
        inv.amg_setup()
    assert inv.amg_info()["levels"] == 0
    inv.close()
    with pytest.raises(rails_amd.RailsError, match=einval + ".*LU or an iterative solve"):
        rails_amd.IterativeInverse(ctx, lu.op, method="cg", diag=1.0 / A.diagonal(), amg=True)
    lu.close()


def test_refuses_two_to_the_24_rows(ctx):
    """the cycle's kernels take 24-bit row numbers: a diagonal matrix of 2^24 rows (0.3 GB) is refused where "amg" is set and by the
    set-up, before any work; "amg" stays off, so a solve of the object is the Jacobi solve it was; one row fewer passes the gate"""
    import rails_amd

    einval = r"\(code -1\)"
    X = Y = None
    for n, refused in ((1 << 24, True), ((1 << 24) - 1, False)):
        op = rails_amd.HipOperatorWrapper(ctx, np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32), np.full(n, 2.0))
        inv = rails_amd.IterativeInverse(ctx, op, method="cg", tol=TOL)
        if refused:
            with pytest.raises(rails_amd.RailsError, match=einval + ".*fewer than 2\\^24"):
                inv.set("amg", 1)
            with pytest.raises(rails_amd.RailsError, match=einval + ".*fewer than 2\\^24"):
                inv.amg_setup()
            assert inv.amg_info()["levels"] == 0
            X = rails_amd.HipMultiVectorWrapper(ctx, n, 1)
            ctx.lib.rails_panel_fill(ctx.h, X.panel.h, X.c0, 1, 3.0)
            Y = inv.solve(X)  # "amg" is off: nothing of it runs
            assert inv.amg_info()["cycles"] == 0 and np.all(inv.columns()[2] == 2)
            assert np.all(Y.to_host() == 1.5)
        else:
            inv.set("amg", 1)  # (the set-up itself would refuse this matrix for another reason: it does not coarsen)
            inv.set("amg", 0)
        inv.close()
        X = Y = op = inv = None  # (the handles free their device memory when they go)
