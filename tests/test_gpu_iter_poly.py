"""The Chebyshev polynomial preconditioner of the iterative A^-1 operator (include/rails_hip.h: "poly_degree", rails_iter_precondition;
rails_amd/csrc/itsolve.hip: k_cheb_init, k_cheb_step_csr, k_cheb_pass; cheb_coef.h) on the GPU against the numpy restatement of
tests/cheb_reference.py: the preconditioner itself against a longdouble evaluation on the shapes at which the fused kernel takes its
different paths, the preconditioned solves against the restatement's iteration counts, what the polynomial is for (fewer inner products
for about the same products), degree 0 bit for bit, determinism, a callback operator, the refusals and a bound set too low."""
import ctypes

import numpy as np
import pytest

import cheb_reference as C
import iter_reference as R

pytestmark = pytest.mark.gpu

TOL = 1e-10
RATIO = 30.0
EPS = np.finfo(float).eps
WIDTHS = (1, 2, 3, 16, 17, 32, 33, 70)  # 8 lanes per row up to 16 columns, 16 lanes above; odd last columns; two groups of 32 and a tail
DEGREES = (0, 1, 2, 5)                  # off, and both parities of the fused step's ping-pong
PANEL, XC0, YC0 = 200, 37, 91           # windows at odd columns of panels 200 columns wide
SENTINEL = 7.25


@pytest.fixture(scope="module")
def ctx():
    import rails_amd

    c = rails_amd.Context(device=0, seed=3)
    yield c
    c.close()


_inverses = {}


def inverse(ctx, tag):
    """one IterativeInverse (CG) per problem, shared by the tests of this module, with every setting at a known value"""
    import rails_amd

    if tag not in _inverses:
        _inverses[tag] = rails_amd.IterativeInverse(ctx, C.problem(tag), method="cg", tol=TOL)
    inv = _inverses[tag]
    for name, value in (("tolerance", TOL), ("jacobi", 1), ("max_iterations", 1000), ("strict", 0), ("check_every", 8), ("poly_degree", 0),
                        ("poly_ratio", RATIO), ("eig_max", 0), ("poly_fused", 1)):
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


def test_poly_degree_is_a_setting(ctx):
    """(without the feature: RAILS_EINVAL, "no setting named")"""
    inv = inverse(ctx, "lap9x8")
    inv.set("poly_degree", 4)
    inv.set("poly_ratio", 30)
    inv.set("eig_max", 2.5)
    inv.set("poly_fused", 0)
    Bm = R.rhs(72, 2)
    assert R.true_relres(C.problem("lap9x8"), inv.solve_host(Bm), Bm).max() <= 10 * TOL
    st = inv.stats()
    assert st["poly_applications"] > 0 and st["eig_hi"] == 2.5 and st["eig_lo"] == 2.5 / 30


_longdouble = {}


def expected(tag, jacobi, K, nc):
    """the longdouble evaluation on the shared input and the allowed error per column: 4 times the largest error the float64 restatement
    shows against it, at least 64 eps ||y||_inf (room for another order of summation within a row)"""
    key = (tag, jacobi, K, nc)
    if key not in _longdouble:
        A = C.problem(tag)
        g = C.g_of(A, jacobi)
        hi = C.gershgorin(A, g)
        Xm = R.rhs(A.shape[0], nc, seed=9)
        Zl = C.polynomial(A, Xm, K, hi, RATIO, g, dtype=np.longdouble)
        Z64 = C.polynomial(A, Xm, K, hi, RATIO, g)
        bound = np.maximum(4 * np.abs(Z64 - Zl).max(0), 64 * EPS * np.abs(Zl).max(0)).astype(float)
        _longdouble[key] = (Xm, Zl, bound, hi)
    return _longdouble[key]


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


def check_preconditioner(ctx, tag, jacobi, widths, degrees=DEGREES):
    inv = inverse(ctx, tag)
    inv.set("jacobi", 1 if jacobi else 0)
    worst = 0.0
    for nc in widths:
        groups = (nc + 31) // 32
        for K in degrees:
            Xm, Zl, bound, hi = expected(tag, jacobi, K, nc)
            inv.set("poly_degree", K)
            got = {}
            for fused in (1, 0):
                inv.set("poly_fused", fused)
                full, win = precondition_both_ways(ctx, inv, Xm)
                st = inv.stats()
                assert st["poly_applications"] == groups and st["products"] == K * groups
                assert st["fused_launches"] == (K * groups if fused else 0), (st, K, nc, fused)
                if K > 0:  # (the library adds a row's entries in stored order, numpy in its own: the last bit may differ)
                    assert abs(st["eig_hi"] - hi) <= 4 * EPS * hi and abs(st["eig_lo"] - hi / RATIO) <= 4 * EPS * hi / RATIO
                assert np.array_equal(full, win)  # the same bits through a window
                err = np.abs(full - Zl).astype(float)
                worst = max(worst, (err.max(0) / bound).max())
                assert np.all(err <= bound[None, :]), (tag, jacobi, nc, K, fused, (err.max(0) / bound).max())
                got[fused] = full
            assert np.all(np.abs(got[1] - got[0]) <= bound[None, :])
    print("problem %s, jacobi %d: largest error / allowed error %.3f" % (tag, jacobi, worst))


@pytest.mark.parametrize("tag", ["lap9x8", "one", "stencil27", "banded41"])
def test_precondition_against_longdouble(ctx, tag):
    """72 rows (a partial second block of 64), one row, rows of 8 to 27 entries (the groups of eight and the tails of four), and blocks of
    2624 nonzeros (beyond what is staged in LDS: one entry at a time)"""
    check_preconditioner(ctx, tag, True, WIDTHS)


@pytest.mark.parametrize("tag,jacobi", [("neg_banded41", True), ("neg_banded41", False), ("lap9x8", False), ("banded41", False)])
def test_precondition_either_sign_with_and_without_jacobi(ctx, tag, jacobi):
    """a negative definite operator with Jacobi (negative G) and without (G = -I, the sign path), a positive one without (G = I)"""
    check_preconditioner(ctx, tag, jacobi, (1, 3, 17, 33))
    Xm, Zl, _, _ = expected(tag, jacobi, 5, 3)
    negative = C.problem(tag).diagonal()[0] < 0
    assert np.all(((Xm * Zl).sum(0) < 0) == negative)  # the preconditioner has the operator's own sign


def solve_and_check(ctx, tag, K, nc, jacobi=True):
    import rails_amd

    A, Bm, Xr, cr = C.reference(tag, nc, K, ratio=RATIO, jacobi=jacobi)
    inv = inverse(ctx, tag)
    inv.set("jacobi", 1 if jacobi else 0)
    inv.set("poly_degree", K)
    big = np.full((A.shape[0], PANEL), np.nan)
    big[:, XC0:XC0 + nc] = Bm
    Xp = rails_amd.HipMultiVectorWrapper(ctx, data=big)
    Yp = rails_amd.HipMultiVectorWrapper(ctx, data=np.full((A.shape[0], PANEL), SENTINEL))
    inv.solve(window(Xp, XC0, nc), window(Yp, YC0, nc))
    Yh = Yp.to_host()
    assert np.all(Yh[:, :YC0] == SENTINEL) and np.all(Yh[:, YC0 + nc:] == SENTINEL)
    Xg = Yh[:, YC0:YC0 + nc]
    it, rel, flags = inv.columns()
    st = inv.stats()
    print("problem %s, K %d, %d columns, jacobi %d: iterations %d..%d (restatement %d..%d), products %d, inner products %d, fused launches %d" % (
        tag, K, nc, jacobi, it.min(), it.max(), cr.iter.min(), cr.iter.max(), st["products"], st["inner_products"], st["fused_launches"]))
    assert np.all(np.isfinite(Xg)) and np.all(flags == 2), flags
    assert R.true_relres(A, Xg, Bm).max() <= 10 * TOL
    assert np.all(it <= 1.5 * cr.iter), (it, cr.iter)
    assert st["fused_launches"] > 0 and st["unconverged_columns"] == 0
    return st, cr


@pytest.mark.parametrize("nc", (1, 16, 33))
@pytest.mark.parametrize("K", (2, 4))
@pytest.mark.parametrize("tag", ["lap9x8", "lap64"])
def test_preconditioned_solves_match_the_restatement(ctx, tag, K, nc):
    solve_and_check(ctx, tag, K, nc)


def test_solve_without_jacobi_on_the_sign_path(ctx):
    solve_and_check(ctx, "lap9x8", 2, 3, jacobi=False)


def test_fewer_inner_products_for_about_the_same_products(ctx):
    """64 x 64, K = 4, ratio 30, the same right-hand side: fewer than half the inner products of K = 0 (the restatement: 0.22, and 1.5
    times that is 0.34), at most 1.5 times the restatement's products"""
    A, Bm, _, c0 = C.reference("lap64", 2, 0, ratio=RATIO)
    _, _, _, c4 = C.reference("lap64", 2, 4, ratio=RATIO)
    inv = inverse(ctx, "lap64")
    X0 = inv.solve_host(Bm)
    st0 = inv.stats()
    inv.set("poly_degree", 4)
    X4 = inv.solve_host(Bm)
    st4 = inv.stats()
    print("K = 0: %d inner products, %d products, %d launches; K = 4: %d, %d, %d (restatement: %d and %d products)" % (
        st0["inner_products"], st0["products"], st0["launches"], st4["inner_products"], st4["products"], st4["launches"], C.products(c0, 0), C.products(c4, 4)))
    assert R.true_relres(A, X0, Bm).max() <= 10 * TOL and R.true_relres(A, X4, Bm).max() <= 10 * TOL
    assert st4["inner_products"] < 0.5 * st0["inner_products"]
    assert st4["products"] <= 1.5 * C.products(c4, 4)


def test_degree_zero_is_the_solve_as_it_was(ctx):
    import rails_amd

    A = C.problem("lap9x8")
    Bm = R.rhs(A.shape[0], 5)
    results, stats = [], []
    for explicit in (False, True):
        inv = rails_amd.IterativeInverse(ctx, A, method="cg", tol=TOL)
        if explicit:
            inv.set("poly_degree", 0)
        results.append(inv.solve_host(Bm))
        info = (ctypes.c_double * 13)()
        assert ctx.lib.rails_iter_stats(inv.h, info, 13) == 13
        stats.append(list(info))
        full = inv.stats()
        assert full["poly_applications"] == 0 and full["fused_launches"] == 0 and full["eig_hi"] == 0 and full["eig_lo"] == 0
        inv.close()
    assert np.array_equal(results[0], results[1])
    assert stats[0] == stats[1]


def test_determinism_and_check_every(ctx):
    import rails_amd

    A, Bm, _, _ = C.reference("lap64", 5, 4, ratio=RATIO)
    inv = inverse(ctx, "lap64")
    inv.set("poly_degree", 4)
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


def test_columns_of_different_speed(ctx):
    A = C.problem("lap64")
    n = A.shape[0]
    s = np.sin(np.pi * np.arange(1, 65) / 65)
    Bm = R.rhs(n, 4)
    Bm[:, 1] = 0.0
    Bm[:, 2] = np.kron(s, s)  # an eigenvector of A, and of p(G A) G
    Xr, cr = C.pcg(A, Bm, 4, ratio=RATIO, tol=TOL)
    assert cr.iter[1] == 0 and cr.iter[2] == 1
    inv = inverse(ctx, "lap64")
    inv.set("poly_degree", 4)
    Xg = inv.solve_host(Bm)
    it, rel, flags = inv.columns()
    print("iterations", it, "restatement", cr.iter)
    assert it[1] == 0 and it[2] == 1
    assert it[0] <= 1.5 * cr.iter[0] and it[3] <= 1.5 * cr.iter[3] and it[0] >= 20 and it[3] >= 20
    assert np.all(Xg[:, 1] == 0.0)
    assert np.all(np.isfinite(Xg)) and np.all(flags == 2)
    assert R.true_relres(A, Xg[:, [0, 2, 3]], Bm[:, [0, 2, 3]]).max() <= 10 * TOL


def test_callback_operator_needs_eig_max(ctx):
    import rails_amd

    A, Bm, Xr, cr = C.reference("lap9x8", 3, 4, ratio=RATIO)
    csr_op = rails_amd.HipOperatorWrapper(ctx, A.indptr, A.indices, A.data)

    def action(trans, X, Y):
        csr_op.apply(X, Y)
        return 0

    cb = rails_amd.HipOperatorWrapper.from_callback(ctx, A.shape[0], action)
    inv = rails_amd.IterativeInverse(ctx, cb, method="cg", tol=TOL, diag=A.diagonal(), poly_degree=4, poly_ratio=RATIO)
    with pytest.raises(rails_amd.RailsError, match=r"\(code -1\).*eig_max"):
        inv.solve_host(Bm)
    with pytest.raises(rails_amd.RailsError, match=r"\(code -1\).*eig_max"):
        inv.precondition(rails_amd.HipMultiVectorWrapper(ctx, data=Bm))
    inv.set("eig_max", C.gershgorin(A, C.g_of(A, True)))
    Xg = inv.solve_host(Bm)
    it, rel, flags = inv.columns()
    st = inv.stats()
    assert np.all(flags == 2) and np.all(it <= 1.5 * cr.iter)
    assert R.true_relres(A, Xg, Bm).max() <= 10 * TOL
    assert st["fused_launches"] == 0 and st["poly_applications"] > 0 and st["products"] >= 5 * it.max()
    inv.close()


def test_refusals(ctx):
    import rails_amd

    einval = r"\(code -1\)"
    A = C.problem("lap9x8")
    bi = rails_amd.IterativeInverse(ctx, A, method="bicgstab", tol=TOL)
    with pytest.raises(rails_amd.RailsError, match=einval + ".*BiCGStab"):
        bi.set("poly_degree", 4)
    bi.set("poly_degree", 0)  # off is no request
    Bm = R.rhs(A.shape[0], 2)
    assert R.true_relres(A, bi.solve_host(Bm), Bm).max() <= 10 * TOL
    bi.close()
    with pytest.raises(rails_amd.RailsError, match=einval + ".*BiCGStab"):
        rails_amd.IterativeInverse(ctx, A, method="bicgstab", poly_degree=2)
    inv = inverse(ctx, "lap9x8")
    for bad in (1.0, 0.5, 0.0, -3.0):
        with pytest.raises(rails_amd.RailsError, match=einval + ".*poly_ratio"):
            inv.set("poly_ratio", bad)
    for bad in (-1, 65, 2.5):
        with pytest.raises(rails_amd.RailsError, match=einval + ".*poly_degree"):
            inv.set("poly_degree", bad)
    with pytest.raises(rails_amd.RailsError, match=einval + ".*eig_max"):
        inv.set("eig_max", -1.0)
    inv.set("poly_degree", 64)
    # windows and rows of rails_iter_precondition
    X = rails_amd.HipMultiVectorWrapper(ctx, data=Bm)
    with pytest.raises(rails_amd.RailsError, match=einval + ".*alias"):
        inv.precondition(X, X)
    with pytest.raises(rails_amd.RailsError, match=einval + ".*rows"):
        inv.precondition(rails_amd.HipMultiVectorWrapper(ctx, data=Bm[:-1]))
    # the object still works, at the largest degree
    assert R.true_relres(A, inv.solve_host(Bm), Bm).max() <= 10 * TOL


@pytest.mark.parametrize("K", (2, 3))
def test_a_bound_set_too_low(ctx, K):
    """eig_max a quarter of the Gershgorin bound on the 9 x 8 Laplacian.  Above the bound the residual polynomial T_{K+1} is large with the
    sign (-1)^(K+1): for odd K the preconditioner is indefinite and the ordinary breakdown rule meets it (p.Ap and r.z of different
    signs), for even K it stays definite and the solve is merely slow.  Either way every column converges or is flagged breakdown, the
    call returns RAILS_OK, strict turns flagged columns into RAILS_ENOCONV, and a converged column is finite."""
    import rails_amd

    A = C.problem("lap9x8")
    Bm = R.rhs(A.shape[0], 3)
    low = 0.25 * C.gershgorin(A, C.g_of(A, True))
    _, cr = C.pcg(A, Bm, K, ratio=RATIO, hi=low, tol=TOL)
    inv = inverse(ctx, "lap9x8")
    inv.set("poly_degree", K)
    inv.set("eig_max", low)
    X = rails_amd.HipMultiVectorWrapper(ctx, data=Bm)
    Y = rails_amd.HipMultiVectorWrapper(ctx, A.shape[0], 3)
    rc = ctx.lib.rails_iter_solve(ctx.h, inv.h, 0, X.panel.h, X.c0, X.n, Y.panel.h, Y.c0)
    assert rc == 0
    it, rel, flags = inv.columns()
    print("bound too low, K %d: flags %s iterations %s (restatement %s, %s)" % (K, flags, it, cr.flags, cr.iter))
    assert np.all((flags == 8) | (flags == 2)), flags
    assert np.array_equal(flags, cr.flags)
    assert np.any(flags == 8) == (K == 3)
    Yh = Y.to_host()
    assert np.all(np.isfinite(Yh[:, flags == 2]))
    assert R.true_relres(A, Yh[:, flags == 2], Bm[:, flags == 2]).max(initial=0.0) <= 10 * TOL
    inv.set("strict", 1)
    rc = ctx.lib.rails_iter_solve(ctx.h, inv.h, 0, X.panel.h, X.c0, X.n, Y.panel.h, Y.c0)
    assert rc == (rails_amd.itsolve.ENOCONV if K == 3 else 0)
