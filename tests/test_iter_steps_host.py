"""The step-by-step restatement of the CG and BiCGStab recurrences (tests/iter_steps_reference.py) on the CPU: for every case of
tests/test_gpu_iter_steps.py the float64 restatement in every order of summation is within the bounds, the bounds stay under their cap
and no column comes near convergence before the last step; the restated pass geometry gives the table the cases were chosen for; the
restatement agrees with tests/iter_reference.py; and seeded mistakes are rejected by the bounds at the smallest case that can show them."""
import numpy as np
import pytest

import iter_reference as R
import iter_steps_reference as S


@pytest.mark.parametrize("case_id", [c.id for c in S.CASES])
def test_bounds_and_conditions(case_id):
    c = S.case(case_id)
    e = S.expected(c)
    worst_x = worst_r = 0.0
    for k in c.steps:
        for order in S.ORDERS:
            assert np.all(e.err_x[k][order] <= e.bound_x[k]) and np.all(e.err_r[k][order] <= e.bound_r[k]), (case_id, k, order)
            worst_x = max(worst_x, (e.err_x[k][order] / e.xmax[k]).max() / S.EPS)
            worst_r = max(worst_r, e.err_r[k][order].max() / S.EPS)
        assert np.all(e.xmax[k] > 0)
        assert np.all(e.bound_x[k] <= S.CAP * e.xmax[k]), (case_id, k, (e.bound_x[k] / e.xmax[k]).max() / S.EPS)  # condition 1
        assert np.all(e.bound_r[k] <= S.CAP), (case_id, k, e.bound_r[k].max() / S.EPS)
    k = max(c.steps)
    assert np.all(e.decay[k] >= S.RR_FLOOR), (case_id, e.decay[k].min())  # condition 2
    print("%s: the float64 restatement's worst error %.1f eps of |x|_inf, %.1f eps in the relative residual; rr_K / bb >= %.1e" % (
        case_id, worst_x, worst_r, e.decay[k].min()))


def test_the_case_list_is_the_intended_one():
    ids = [c.id for c in S.CASES]
    assert len(set(ids)) == len(ids)
    per_variant = {v[0]: sorted((c.m, c.w) for c in S.CASES if c.variant == v[0]) for v in S.VARIANTS}
    everything = sorted((m, w) for m, (widths, _, _) in S.SHAPES.items() for w in widths)
    for name in ("cg-jacobi", "cg-plain", "bicgstab-jacobi", "bicgstab-plain"):
        assert per_variant[name] == everything
    for name in ("bicgstab-jacobi-trans", "bicgstab-plain-trans"):
        assert per_variant[name] == [mw for mw in everything if mw[0] in (72, 2181)]
    for name in ("cg-negated-jacobi", "cg-negated-plain"):
        assert per_variant[name] == [mw for mw in everything if mw[0] == 72]
    for name in ("cg-poly-fused", "cg-poly-unfused"):
        assert per_variant[name] == [(72, 3), (72, 32), (2181, 3), (2181, 32)]
    for c in S.CASES:
        full = S.SHAPES[c.m][1]
        assert c.steps == full[:len(c.steps)] and len(c.steps) >= 1  # a lowered case keeps the first steps
        assert (c.steps != full) == ((c.variant, c.m, c.w) in S.LOWERED)
    assert all(not S.case("%s-m%d-w%d" % key).poly for key in S.LOWERED)


def test_lowered_cases_miss_the_cap_at_the_first_step_left_out():
    """a case has fewer steps only where condition 1 fails at the next one"""
    for (variant, m, w), steps in S.LOWERED.items():
        k = S.SHAPES[m][1][len(steps)]
        e = S.Expected(S.Case(next(v for v in S.VARIANTS if v[0] == variant), m, w, (k,)))
        over_x, over_r = (e.bound_x[k] / e.xmax[k]).max() / S.CAP, e.bound_r[k].max() / S.CAP
        print("%s-m%d-w%d, step %d: bound / cap %.3g for x, %.3g for the relative residual" % (variant, m, w, k, over_x, over_r))
        assert over_x > 1.0 or over_r > 1.0


def test_geometry_table():
    """every group of every case lands on the geometry it was chosen for"""
    seen = set()
    for c in S.CASES:
        for _, gw in S.groups(c.w):
            assert S.geometry(c.m, gw) == S.GEOMETRY[(c.m, gw)], (c.m, gw, S.geometry(c.m, gw))
            seen.add((c.m, gw))
    assert seen == set(S.GEOMETRY)
    assert S.groups(70) == [(0, 32), (32, 32), (64, 6)] and S.groups(33) == [(0, 32), (32, 1)]
    # what the shapes are for
    assert {S.geometry(72, w)[0] for w in S.SHAPES[72][0] if w <= 32} == {256, 128, 64, 32, 16}          # every tx_bits
    assert all(S.geometry(5, w)[0] > 5 for w in S.SHAPES[5][0])                                          # fewer rows than row classes
    assert S.geometry(2181, 17) == S.geometry(2181, 32) == (16, 17, 129, 117)                            # a strand's second trip, ragged
    assert S.geometry(4231, 16)[1] == 16 and S.geometry(4231, 32)[1] == 33
    assert 131168 // (16 * 8) >= 1024 and S.geometry(131168, 32) == (16, 1017, 129, 104)                 # the cap of 1024 slabs


@pytest.mark.parametrize("method,jacobi,trans", [("cg", True, False), ("cg", False, False), ("bicgstab", True, False), ("bicgstab", False, True)])
def test_agrees_with_the_solve_restatement(method, jacobi, trans):
    """the same recurrences as iter_reference's solves stopped after k iterations (those carry the freeze and the breakdown rules; the
    updates here are written without axpy_sel): the same iterates to rounding"""
    A, B = S.matrix(method, 72), S.rhs(72, 3)
    steps = (S.cg_steps if method == "cg" else S.bicgstab_steps)(A, B, 4, jacobi, trans)
    for k in range(1, 5):
        kw = {"trans": trans} if method == "bicgstab" else {}
        X, c = R.solve(method, A, B, tol=0.0, maxit=k, jacobi=jacobi, **kw)
        assert np.all(c.iter == k) and np.all(c.flags == R.MAXIT)
        assert np.abs(steps[k - 1][0] - X).max() <= 64 * S.EPS * np.abs(X).max()
        assert np.abs(steps.relres(k) - c.relres()).max() <= 64 * S.EPS


def test_negated_operator_gives_the_negated_iterates():
    """CG on (-A, b): x_k = -x_k of (A, b) bit for bit, with the sign rule of iter_scalars.h letting the run without Jacobi through"""
    for jacobi in (True, False):
        pos = S.cg_steps(S.matrix("cg", 72), S.rhs(72, 3), 3, jacobi)
        neg = S.cg_steps(S.matrix("cg", 72, negated=True), S.rhs(72, 3), 3, jacobi)
        for (xp, rp), (xn, rn) in zip(pos, neg):
            assert np.array_equal(xp, -xn) and np.array_equal(rp, rn)


def _rejection(c, bug):
    """(largest error / bound over the case's steps, the step it occurs at, whether in x or in the residual)"""
    e = S.expected(c)
    run = c.run(bug=bug)
    worst = (0.0, 0, "")
    for k in c.steps:
        rx, rr = e.ratios(k, run[k - 1][0], run.relres(k))
        worst = max(worst, (rx, k, "x"), (rr, k, "relres"))
    return worst


@pytest.mark.parametrize("bug", S.MISTAKES)
def test_seeded_mistakes_are_rejected(bug):
    assert S.CAUGHT_BY[bug]
    for case_id in S.CAUGHT_BY[bug]:
        c = S.case(case_id)
        ratio, k, what = _rejection(c, bug)
        print("%s: rejected by %s at step %d, %s error / bound %.3g" % (bug, case_id, k, what, ratio))
        assert ratio > 10.0, (bug, case_id, ratio)
        assert _rejection(c, None)[0] <= 0.25  # the unmutated run is far inside


def test_the_cases_named_are_the_smallest_that_can_show_the_mistake():
    """m = 5, w = 2 is the first case of its variant; the last slab can only be skipped where there are more than 16 of them"""
    for bug, ids in S.CAUGHT_BY.items():
        for case_id in ids:
            c = S.case(case_id)
            smaller = [o for o in S.CASES if o.variant == c.variant and (o.m, o.w) < (c.m, c.w)]
            if bug == "reduce_skips_last_slab":
                assert all(S.geometry(o.m, gw)[1] <= 16 for o in smaller for _, gw in S.groups(o.w))
                assert S.geometry(c.m, c.w)[1] > 16
            else:
                assert not smaller
    c = S.case("cg-jacobi-m4231-w16")  # exactly 16 slabs: nothing is skipped, the same bits
    a, b = c.run(), c.run(bug="reduce_skips_last_slab")
    assert all(np.array_equal(xa, xb) and np.array_equal(ra, rb) for (xa, ra), (xb, rb) in zip(a, b))
