"""The iterative A^-1 operator (include/rails_hip.h: rails_iter_*, rails_amd/csrc/itsolve.hip, iter_setup.hip) on the GPU against the numpy restatement of
tests/iter_reference.py: solves through the operator handle (rails_spmm) and through rails_iter_solve on full panels and on windows at odd
columns of wide panels, the transposed solve, determinism and independence of check_every, columns of different speed in one solve, the
iteration cap, the breakdown rule, the refusals, and the work panels.
The passes themselves, iterate by iterate against a longdouble run: tests/test_gpu_iter_steps.py."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import iter_reference as R

pytestmark = pytest.mark.gpu

TOL = 1e-10
WIDTHS = (1, 3, 16, 17, 33, 70)  # one column, an odd width, a full 16, one past it, one past a group of 32, two groups and a tail
PANEL, XC0, YC0 = 200, 37, 91    # windows at odd columns of panels 200 columns wide
SENTINEL = 7.25


@pytest.fixture(scope="module")
def ctx():
    import rails_amd

    c = rails_amd.Context(device=0, seed=3)
    yield c
    c.close()


_inverses = {}


def inverse(ctx, tag, jacobi=True, maxit=1000):
    """one IterativeInverse per problem, shared by the tests of this module"""
    import rails_amd

    if tag not in _inverses:
        A, method = R.problem(tag)
        _inverses[tag] = rails_amd.IterativeInverse(ctx, A, method=method, tol=TOL)
    inv = _inverses[tag]
    inv.set("tolerance", TOL)
    inv.set("jacobi", 1 if jacobi else 0)
    inv.set("max_iterations", maxit)
    inv.set("strict", 0)
    inv.set("check_every", 8)
    return inv


@pytest.fixture(scope="module", autouse=True)
def _close_inverses(ctx):
    yield
    for inv in _inverses.values():
        inv.close()
    _inverses.clear()


def window(mv, c0, nc):
    return mv.view(c0, c0 + nc - 1) if nc > 1 else mv.view(c0)


def solve_all_ways(ctx, inv, Bm, trans=False):
    """the four ways the issue names: handle / rails_iter_solve x full panels / windows.  Returns the four results; checks that X is
    unchanged and that nothing beside Y's window was written"""
    import rails_amd

    n, nc = Bm.shape
    out = []
    op = inv.op.transpose() if trans else inv.op
    for through_handle in (False, True):
        X = rails_amd.HipMultiVectorWrapper(ctx, data=Bm)
        Y = rails_amd.HipMultiVectorWrapper(ctx, n, nc)
        if through_handle:
            op.apply(X, Y)
        else:
            inv.solve(X, Y, trans=trans)
        assert np.array_equal(X.to_host(), Bm)
        out.append(Y.to_host())
        big = np.full((n, PANEL), np.nan)
        big[:, XC0:XC0 + nc] = Bm
        Xp = rails_amd.HipMultiVectorWrapper(ctx, data=big)
        Yp = rails_amd.HipMultiVectorWrapper(ctx, data=np.full((n, PANEL), SENTINEL))
        Xv, Yv = window(Xp, XC0, nc), window(Yp, YC0, nc)
        if through_handle:
            op.apply(Xv, Yv)
        else:
            inv.solve(Xv, Yv, trans=trans)
        assert np.array_equal(Xp.to_host(), big, equal_nan=True)  # X and the NaN beside its window are as they were
        Yh = Yp.to_host()
        assert np.all(Yh[:, :YC0] == SENTINEL) and np.all(Yh[:, YC0 + nc:] == SENTINEL)  # the sentinels survive
        out.append(Yh[:, YC0:YC0 + nc].copy())
    return out


def check_against_restatement(ctx, tag, nc, jacobi):
    A, Bm, Xr, cr = R.reference(tag, nc, jacobi=jacobi)
    inv = inverse(ctx, tag, jacobi=jacobi, maxit=5000)
    results = solve_all_ways(ctx, inv, Bm)
    it, rel, flags = inv.columns()
    print("problem (%s), %d columns, jacobi %d: iterations %d..%d (restatement %d..%d), products on %s" % (
        tag, nc, jacobi, it.min(), it.max(), cr.iter.min(), cr.iter.max(), inv.A.last_kernel()))
    for Xg in results:
        assert np.all(np.isfinite(Xg))
        true_rel = R.true_relres(A, Xg, Bm)
        assert true_rel.max() <= 10 * TOL, true_rel.max()
        assert np.array_equal(Xg, results[0])  # the same bits whichever way the solve was asked for
    assert np.all(flags == 2), flags  # converged
    assert np.all(rel <= TOL)
    assert np.all(it <= 1.5 * cr.iter), (it, cr.iter)
    st = inv.stats()
    assert st["unconverged_columns"] == 0 and st["max_iterations_of_a_column"] == it.max()


@pytest.mark.parametrize("nc", WIDTHS)
@pytest.mark.parametrize("tag", ["a", "b", "c", "c4", "c'", "d", "e"])
def test_solves_match_the_restatement(ctx, tag, nc):
    check_against_restatement(ctx, tag, nc, True)


@pytest.mark.parametrize("nc", (3, 33))
@pytest.mark.parametrize("tag", ["b", "c'"])
def test_scaled_problems_without_jacobi(ctx, tag, nc):
    """(b) and (c') with jacobi 0: several times the iterations, the same answers"""
    check_against_restatement(ctx, tag, nc, False)
    _, _, _, with_j = R.reference(tag, nc, jacobi=True)
    it, _, _ = inverse(ctx, tag).columns()
    assert it.min() > 1.5 * with_j.iter.max()  # the bound of the Jacobi runs does tell the two paths apart


@pytest.mark.parametrize("nc", (16, 17))
def test_kernel_coverage_on_the_grid_stencil(ctx, nc):
    """(d) at 16 columns runs its products on the plane-sweep kernel, at 17 on a row kernel: both must pass (recorded, not asserted)"""
    check_against_restatement(ctx, "d", nc, True)
    print("laplace7(13, 11, 10), %d columns: rails_csr_last_kernel = %s" % (nc, inverse(ctx, "d").A.last_kernel()))


def test_transposed_solve(ctx):
    A, Bm, Xr, cr = R.reference("c", 3, trans=True)
    inv = inverse(ctx, "c")
    Xs = spla.splu(sp.csc_matrix(A.T)).solve(Bm)
    for Xg in solve_all_ways(ctx, inv, Bm, trans=True):
        assert R.true_relres(A, Xg, Bm, trans=True).max() <= 10 * TOL
        # against splu(A.T) without a condition number: A' (X - Xs) is the solve's residual minus splu's own, which is at rounding level
        assert (np.linalg.norm(A.T @ (Xg - Xs), axis=0) / np.linalg.norm(Bm, axis=0)).max() <= 11 * TOL
    it, _, flags = inv.columns()
    assert np.all(flags == 2) and np.all(it <= 1.5 * cr.iter)
    # and it is not the untransposed solve
    assert R.true_relres(A, Xg, Bm, trans=False).max() > 1e-3


@pytest.mark.parametrize("tag", ["a", "c"])
def test_determinism_and_check_every(ctx, tag):
    import rails_amd

    A, Bm, Xr, cr = R.reference(tag, 5)
    inv = inverse(ctx, tag)
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
    A, _ = R.problem("a")
    n = A.shape[0]
    k = int(round(np.sqrt(n)))
    s = np.sin(np.pi * np.arange(1, k + 1) / (k + 1))
    Bm = R.rhs(n, 4)
    Bm[:, 1] = 0.0
    Bm[:, 2] = np.kron(s, s)  # an eigenvector of A
    Xr, cr = R.cg(A, Bm, tol=TOL)
    assert cr.iter[1] == 0 and cr.iter[2] == 1
    inv = inverse(ctx, "a")
    Xg = inv.solve_host(Bm)
    it, rel, flags = inv.columns()
    print("iterations", it, "restatement", cr.iter)
    assert it[1] == 0 and it[2] == 1
    assert it[0] <= 1.5 * cr.iter[0] and it[3] <= 1.5 * cr.iter[3] and it[0] >= 100 and it[3] >= 100
    assert np.all(Xg[:, 1] == 0.0)
    assert np.all(np.isfinite(Xg)) and np.all(flags == 2)
    assert R.true_relres(A, Xg[:, [0, 2, 3]], Bm[:, [0, 2, 3]]).max() <= 10 * TOL


def test_iteration_cap_and_strict(ctx):
    import rails_amd

    A, Bm, _, _ = R.reference("a", 3)
    X5, c5 = R.cg(A, Bm, tol=TOL, maxit=5)
    inv = inverse(ctx, "a", maxit=5)
    X = rails_amd.HipMultiVectorWrapper(ctx, data=Bm)
    Y = rails_amd.HipMultiVectorWrapper(ctx, A.shape[0], 3)
    rc = ctx.lib.rails_iter_solve(ctx.h, inv.h, 0, X.panel.h, X.c0, X.n, Y.panel.h, Y.c0)
    assert rc == 0  # RAILS_OK: the reference allows an approximate inverse
    it, rel, flags = inv.columns()
    assert np.all(flags == 4) and np.all(it == 5)
    Xg = Y.to_host()
    assert np.linalg.norm(Xg - X5) <= 1e-10 * np.linalg.norm(X5)
    assert inv.stats()["unconverged_columns"] == 3
    inv.set("strict", 1)
    rc = ctx.lib.rails_iter_solve(ctx.h, inv.h, 0, X.panel.h, X.c0, X.n, Y.panel.h, Y.c0)
    assert rc == rails_amd.itsolve.ENOCONV == -7
    assert b"did not reach the tolerance" in ctx.lib.rails_last_error()
    assert np.array_equal(Y.to_host(), Xg)  # the last iterates are delivered all the same


def test_cg_breakdown_on_an_indefinite_matrix(ctx):
    import rails_amd

    n = 500
    d = np.array([2.0] * 10 + [-1.0] * (n - 10))
    b = np.ones((n, 1))
    assert (d * b[:, 0] ** 2).sum() < 0  # p.q is negative where rho = r.r is positive
    inv = rails_amd.IterativeInverse(ctx, sp.diags(d).tocsr(), method="cg", tol=TOL, jacobi=False)
    Xg = inv.solve_host(b)
    it, rel, flags = inv.columns()
    assert flags[0] == 8 and it[0] == 1, (flags, it)
    assert np.all(np.isfinite(Xg))
    st = inv.stats()
    assert st["breakdown_columns"] == 1 and st["unconverged_columns"] == 1
    inv.set("jacobi", 1)
    Xg = inv.solve_host(b)
    it, rel, flags = inv.columns()
    assert flags[0] == 2 and it[0] == 1
    assert np.allclose(Xg[:, 0], b[:, 0] / d, rtol=1e-14, atol=0)
    inv.close()


def test_callback_operator_with_a_given_diagonal(ctx):
    """A as an operator given by its action (the Schur complement's form): the preconditioner comes from diag_host"""
    import rails_amd

    A, Bm, Xr, cr = R.reference("b", 3)
    csr_op = rails_amd.HipOperatorWrapper(ctx, A.indptr, A.indices, A.data)

    def action(trans, X, Y):
        (csr_op.transpose() if trans else csr_op).apply(X, Y)
        return 0

    cb = rails_amd.HipOperatorWrapper.from_callback(ctx, A.shape[0], action)
    inv = rails_amd.IterativeInverse(ctx, cb, method="cg", tol=TOL, diag=A.diagonal())
    Xg = inv.solve_host(Bm)
    it, rel, flags = inv.columns()
    assert np.all(flags == 2) and np.all(it <= 1.5 * cr.iter)
    assert R.true_relres(A, Xg, Bm).max() <= 10 * TOL
    with pytest.raises(ValueError):
        rails_amd.IterativeInverse(ctx, cb)  # an operator wrapper needs its method named
    inv.close()


def test_refusals(ctx):
    import rails_amd

    A, Bm, _, _ = R.reference("a", 3)
    n = A.shape[0]
    einval = r"\(code -1\)"
    # a rectangular operator
    rect = rails_amd.HipOperatorWrapper.rect(ctx, 2, 3, np.array([0, 1, 2]), np.array([0, 2]), np.array([1.0, 1.0]))
    with pytest.raises(rails_amd.RailsError, match=einval + ".*rectangular"):
        rails_amd.IterativeInverse(ctx, rect, method="cg")
    inv = inverse(ctx, "a")
    # wrong row counts
    short = rails_amd.HipMultiVectorWrapper(ctx, data=Bm[: n - 1])
    with pytest.raises(rails_amd.RailsError, match=einval + ".*rows"):
        inv.solve(short)
    with pytest.raises(rails_amd.RailsError, match=einval + ".*rows"):
        inv.op.apply(short)
    # aliased X and Y
    X = rails_amd.HipMultiVectorWrapper(ctx, data=Bm)
    with pytest.raises(rails_amd.RailsError, match=einval + ".*alias"):
        inv.solve(X, X)
    with pytest.raises(rails_amd.RailsError, match=einval + ".*alias"):
        inv.solve(X.view(0, 1), X.view(1, 2))
    # a partitioned context
    ctx2 = rails_amd.Context(device=0, seed=1)
    ctx2.set_partition(0, 2, 0, 2 * n)
    op2 = rails_amd.HipOperatorWrapper(ctx2, A.indptr, A.indices, A.data)
    with pytest.raises(rails_amd.RailsError, match=einval + ".*single GPU"):
        rails_amd.IterativeInverse(ctx2, op2, method="cg")
    del op2
    ctx2.close()
    # a NaN right-hand side
    bad = Bm.copy()
    bad[5, 1] = np.nan
    with pytest.raises(rails_amd.RailsError, match=einval + ".*not finite"):
        inv.solve_host(bad)
    # a setting that does not exist, a method that does not exist
    with pytest.raises(rails_amd.RailsError, match=einval):
        inv.set("no_such_setting", 1)
    h = C.c_void_p()
    assert ctx.lib.rails_iter_create(ctx.h, inv.A.h.h, 3, None, C.byref(h)) == -1
    # the object still works
    assert R.true_relres(A, inv.solve_host(Bm), Bm).max() <= 10 * TOL


def test_work_panels_never_shrink(ctx):
    A, B33, _, _ = R.reference("a", 33)
    inv = inverse(ctx, "a")
    inv.solve_host(B33)
    assert inv.stats()["workspace_columns"] == 32  # groups of 32 columns
    inv.solve_host(B33[:, :3])
    st = inv.stats()
    assert st["workspace_columns"] == 32 and len(inv.columns()[0]) == 3
    assert st["total_solves"] >= 2 and st["total_iterations"] > 0
