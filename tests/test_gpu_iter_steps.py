"""The passes of the iterative A^-1 operator (rails_amd/csrc/itsolve.hip: k_cg_init, k_cg_init_poly, k_bi_init, k_iter_dots, k_cg_update,
k_cg_dir, k_bi_dir, k_bi_s, k_bi_update, k_iter_scalars with iter_reduce) step by step on the GPU against the longdouble restatement of
tests/iter_steps_reference.py.  With tolerance 0 and max_iterations k a solve stops every column after exactly k iterations; x_k and the
recurrence's relative residual depend on every inner product, reduction and update up to k, and both must lie within the bounds that
module derives (4 times the float64 restatement's worst error over three orders of summation, at least 64 eps), at the shapes at which
the passes' geometry changes: fewer rows than row classes, every tx_bits, odd last columns, 2, 16, 17, 33 and 1017 slabs, several
groups.  Then the edges: one row, no iteration at all, no trace of an earlier solve in the work panels, windows, determinism."""
import numpy as np
import pytest

import cheb_reference as C
import iter_steps_reference as S

pytestmark = pytest.mark.gpu

PANEL, XC0, YC0 = 200, 37, 91  # windows at odd columns of panels 200 columns wide
SENTINEL = 7.25
MAXIT_FLAG = 4


@pytest.fixture(scope="module")
def ctx():
    import rails_amd

    c = rails_amd.Context(device=0, seed=3)
    yield c
    c.close()


_worst = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for variant in sorted(_worst):
        print("\n%s: largest error / bound over its cases: x %.3f, relative residual %.3f" % ((variant,) + tuple(_worst[variant])), end="")
    print()


def make_inverse(ctx, c, A=None):
    """a new object for the case's matrix, tolerance 0: a column stops only at max_iterations"""
    import rails_amd

    A = c.matrix() if A is None else A
    inv = rails_amd.IterativeInverse(ctx, A, method=c.method, tol=0.0, maxit=1, jacobi=c.jacobi)
    if c.poly:
        inv.set("poly_ratio", S.POLY_RATIO)
        inv.set("eig_max", C.gershgorin(A, C.g_of(A, c.jacobi)))  # the restatement's own number, not the library's sum in another order
        inv.set("poly_fused", 1 if c.fused else 0)
        inv.set("poly_degree", c.poly)
    return inv


def window(mv, c0, nc):
    return mv.view(c0, c0 + nc - 1) if nc > 1 else mv.view(c0)


def solve_k(ctx, inv, B, k, trans=False):
    """(x_k, iterations, relative residuals, flags) of a solve from zero stopped after k iterations"""
    import rails_amd

    inv.set("max_iterations", k)
    X = inv.solve(rails_amd.HipMultiVectorWrapper(ctx, data=B), trans=trans).to_host()
    it, rel, flags = inv.columns()
    return X, it.copy(), rel.copy(), flags.copy()


@pytest.mark.parametrize("case_id", [c.id for c in S.CASES])
def test_steps_against_longdouble(ctx, case_id):
    c = S.case(case_id)
    e = S.expected(c)
    B = c.rhs()
    inv = make_inverse(ctx, c)
    worst_x = worst_r = 0.0
    failures = []
    for k in c.steps:
        X, it, rel, flags = solve_k(ctx, inv, B, k, c.trans)
        assert np.all(it == k) and np.all(flags == MAXIT_FLAG), (case_id, k, it, flags)
        if c.poly:
            st = inv.stats()
            assert (st["fused_launches"] > 0) == c.fused and st["poly_applications"] == (k + 1) * len(S.groups(c.w)), (case_id, st)
        rx, rr = e.ratios(k, X, rel)
        worst_x, worst_r = max(worst_x, rx), max(worst_r, rr)
        if not (rx <= 1.0 and rr <= 1.0):
            failures.append((k, rx, rr))
    inv.close()
    print("%s: largest error / bound: x %.3f, relative residual %.3f" % (case_id, worst_x, worst_r))
    w = _worst.setdefault(c.variant, [0.0, 0.0])
    w[0], w[1] = max(w[0], worst_x), max(w[1], worst_r)
    assert not failures, "%s: (step, x error / bound, residual error / bound) outside: %r" % (case_id, failures)


@pytest.mark.parametrize("case_id", ["cg-jacobi-m72-w17", "bicgstab-jacobi-m72-w17", "bicgstab-plain-m2181-w33"])
def test_windows_give_the_same_bits(ctx, case_id):
    """through windows at odd columns of panels 200 columns wide, NaN beside X and sentinels beside Y: the full-panel result bit for bit"""
    import rails_amd

    c = S.case(case_id)
    B = c.rhs()
    inv = make_inverse(ctx, c)
    full, it, rel, flags = solve_k(ctx, inv, B, 3)
    big = np.full((c.m, PANEL), np.nan)
    big[:, XC0:XC0 + c.w] = B
    Xp = rails_amd.HipMultiVectorWrapper(ctx, data=big)
    Yp = rails_amd.HipMultiVectorWrapper(ctx, data=np.full((c.m, PANEL), SENTINEL))
    inv.solve(window(Xp, XC0, c.w), window(Yp, YC0, c.w))
    it2, rel2, flags2 = inv.columns()
    inv.close()
    assert np.array_equal(Xp.to_host(), big, equal_nan=True)
    Yh = Yp.to_host()
    assert np.all(Yh[:, :YC0] == SENTINEL) and np.all(Yh[:, YC0 + c.w:] == SENTINEL)
    assert np.array_equal(Yh[:, YC0:YC0 + c.w], full)
    assert np.array_equal(it2, it) and np.array_equal(rel2, rel) and np.array_equal(flags2, flags) and np.all(it == 3)


@pytest.mark.parametrize("w", (1, 3))
@pytest.mark.parametrize("method", ("cg", "bicgstab"))
def test_one_row(ctx, method, w):
    """m = 1: one iteration, converged, x = b / d to 4 eps"""
    import rails_amd

    A = S.matrix(method, 1)
    d = A[0, 0]
    B = S.rhs(1, w)
    for jacobi in (True, False):
        inv = rails_amd.IterativeInverse(ctx, A, method=method, tol=1e-10, jacobi=jacobi)
        X = inv.solve_host(B)
        it, rel, flags = inv.columns()
        inv.close()
        assert np.all(it == 1) and np.all(flags == 2), (method, w, jacobi, it, flags)
        assert np.all(np.abs(X - B / d) <= 4 * S.EPS * np.abs(B / d)), (method, w, jacobi)


@pytest.mark.parametrize("method", ("cg", "bicgstab"))
def test_no_iterations_at_all(ctx, method):
    """max_iterations 0: x = 0 exactly over whatever Y held, iter 0, flagged as stopped at the cap, RAILS_OK"""
    import rails_amd

    c = S.case("%s-jacobi-m72-w17" % method)
    inv = make_inverse(ctx, c)
    inv.set("max_iterations", 0)
    X = rails_amd.HipMultiVectorWrapper(ctx, data=c.rhs())
    Y = rails_amd.HipMultiVectorWrapper(ctx, data=np.full((c.m, c.w), SENTINEL))
    rc = ctx.lib.rails_iter_solve(ctx.h, inv.h, 0, X.panel.h, X.c0, X.n, Y.panel.h, Y.c0)
    it, rel, flags = inv.columns()
    inv.close()
    assert rc == 0
    assert np.all(it == 0) and np.all(flags == MAXIT_FLAG) and np.all(rel == 1.0)
    Yh = Y.to_host()
    assert np.all(Yh == 0.0)


@pytest.mark.parametrize("jacobi", (True, False))
@pytest.mark.parametrize("method", ("cg", "bicgstab"))
def test_no_trace_of_an_earlier_solve(ctx, method, jacobi):
    """one object: 32 columns, then a refused solve that leaves a NaN in the work panels' fourth column, then 3, 1 and 31 columns -- each
    the bits of an object that has only ever seen that right-hand side.  The pad column beside an odd last column is read by every ld2
    and must never reach a result."""
    import rails_amd

    m = 2181
    A = S.matrix(method, m)
    B = S.rhs(m, 32)
    used = rails_amd.IterativeInverse(ctx, A, method=method, tol=0.0, maxit=3, jacobi=jacobi)
    used.solve_host(B)
    bad = B[:, :4].copy()
    bad[m // 2, 3] = np.nan
    with pytest.raises(rails_amd.RailsError, match=r"\(code -1\).*not finite"):
        used.solve_host(bad)
    for w in (3, 1, 31):
        Bw = np.ascontiguousarray(B[:, 32 - w:])  # columns the object has seen at other positions
        got = used.solve_host(Bw)
        got_cols = [a.copy() for a in used.columns()]
        fresh = rails_amd.IterativeInverse(ctx, A, method=method, tol=0.0, maxit=3, jacobi=jacobi)
        want = fresh.solve_host(Bw)
        want_cols = fresh.columns()
        fresh.close()
        assert np.all(np.isfinite(got)) and np.all(got_cols[0] == 3) and np.all(got_cols[2] == MAXIT_FLAG), (method, jacobi, w)
        assert np.array_equal(got, want), (method, jacobi, w, np.abs(got - want).max())
        assert all(np.array_equal(a, b) for a, b in zip(got_cols, want_cols))
    used.close()


@pytest.mark.parametrize("method", ("cg", "bicgstab"))
def test_two_runs_give_the_same_bits(ctx, method):
    c = S.case("%s-jacobi-m2181-w32" % method)
    B = c.rhs()
    inv = make_inverse(ctx, c)
    first = solve_k(ctx, inv, B, 8)
    second = solve_k(ctx, inv, B, 8)
    inv.close()
    assert all(np.array_equal(a, b) for a, b in zip(first, second))
    assert np.all(first[1] == 8)
