"""The block forms of the passes of the iterative A^-1 operator (rails_amd/csrc/iter_kernels.inc: k_cg_init_bj, k_cg_update_bj, k_bi_dir_bj,
k_bi_s_bj on iter_pass_block, and the point passes of the same solve on the block geometry) step by step on the GPU against the
longdouble restatement of tests/block_jacobi_reference.py.  With tolerance 0 and max_iterations k a solve stops every column after
exactly k iterations; x_k and the recurrence's relative residual depend on every inner product, reduction, block product and update up
to k, and both must lie within iter_steps_reference's bounds (4 times the float64 restatement's worst error over three orders of
summation, at least 64 eps).  The restatement applies the inverse blocks the library itself uploaded (rails_iter_block_jacobi_info).
Shapes: fewer block rows than row classes, every tx_bits, odd last columns, two groups, 1, 2, 17 (ragged) and 34 slabs, every b for
conjugate gradients and for BiCGStab with both `trans` values; one block row at every b and both methods, where one step arrives: x_1
within its bound, the residuals (rounding noise on both sides) not compared, and beside it the converged solve."""
import numpy as np
import pytest

import block_jacobi_reference as BJ
import iter_steps_reference as S

pytestmark = pytest.mark.gpu

MAXIT_FLAG, CONVERGED_FLAG = 4, 2


@pytest.fixture(scope="module")
def ctx():
    import rails_amd

    c = rails_amd.Context(device=0, seed=3)
    yield c
    c.close()


_problems = {}


def problem(c):
    """block_coupled7 of the case, computed once per (grid, b, skew)"""
    key = (c.nx, c.ny, c.nz, c.b, c.skew)
    if key not in _problems:
        _problems.clear()  # the cases of one problem follow each other; the large ones are not kept
        _problems[key] = c.problem()
    return _problems[key]


def solve_k(ctx, inv, B, k, trans=False):
    import rails_amd

    inv.set("max_iterations", k)
    X = inv.solve(rails_amd.HipMultiVectorWrapper(ctx, data=B), trans=trans).to_host()
    it, rel, flags = inv.columns()
    return X, it.copy(), rel.copy(), flags.copy()


@pytest.mark.parametrize("case_id", [c.id for c in BJ.CASES])
def test_steps_against_longdouble(ctx, case_id):
    import rails_amd

    c = BJ.case(case_id)
    bsr, A = problem(c)
    op = rails_amd.HipOperatorWrapper.from_bsr(ctx, *bsr)
    inv = rails_amd.IterativeInverse(ctx, op, method=c.method, tol=0.0, maxit=1, block_jacobi=True)
    info = inv.block_jacobi_info()
    assert info["b"] == c.b and info["blocks"] == c.nb
    G = info["inverse"]
    e = BJ.Expected(c, G)
    B = c.rhs()
    worst_x = worst_r = 0.0
    failures = []
    for k in c.steps:
        # the bounds' own conditions (host arithmetic): none above the cap, no column converged before the last step
        assert np.all(e.bound_x[k] <= S.CAP * e.xmax[k]) and np.all(e.bound_r[k] <= S.CAP), (case_id, k)
        assert c.one_block or np.all(e.decay[k] >= S.RR_FLOOR), (case_id, k)
        X, it, rel, flags = solve_k(ctx, inv, B, k, c.trans)
        assert np.all(it == k) and np.all((flags == MAXIT_FLAG) | (c.one_block & (flags == CONVERGED_FLAG))), (case_id, k, it, flags)
        rx, rr = e.ratios(k, X, rel)
        if c.one_block:
            # the residuals are rounding noise on both sides (block_jacobi_reference.SHAPES): x_1 alone is compared.  Of the device's
            # residual only its size: r_1 = b - alpha D (G b) with alpha = 1 up to rounding is at most about (b + 2) eps |D| |G| |b|, below
            # 10 * 150 * eps of ||b|| for these blocks (condition below 150, b <= 8), itself below the cap of the bounds
            assert np.all(rel <= S.CAP), (case_id, rel)
            rr = 0.0
        worst_x, worst_r = max(worst_x, rx), max(worst_r, rr)
        if not (rx <= 1.0 and rr <= 1.0):
            failures.append((k, rx, rr))
    inv.close()
    print("%s: largest error / bound: x %.3f, relative residual %.3f" % (case_id, worst_x, worst_r))
    assert not failures, "%s: (step, x error / bound, residual error / bound) outside: %r" % (case_id, failures)


@pytest.mark.parametrize("method,trans", (("cg", False), ("bicgstab", False), ("bicgstab", True)))
@pytest.mark.parametrize("b,w", ((2, 1), (3, 3), (8, 2)))
def test_one_block_row(ctx, method, trans, b, w):
    """m = b: the preconditioner is the exact inverse; one iteration, converged, the true residual within 10 x the tolerance"""
    import rails_amd
    from rails_amd import problems as P

    tol = 1e-10
    bsr, csr = P.block_coupled7(1, 1, 1, b, BJ.SPREAD, skew=0.0 if method == "cg" else BJ.SKEW, seed=b)
    A = BJ.csr_of(csr)
    B = S.rhs(b, w)
    op = rails_amd.HipOperatorWrapper.from_bsr(ctx, *bsr)
    inv = rails_amd.IterativeInverse(ctx, op, method=method, tol=tol, block_jacobi=True)
    X = inv.solve_host(B, trans=trans)
    it, rel, flags = inv.columns()
    inv.close()
    Aop = A.T if trans else A
    true_rel = np.linalg.norm(Aop @ X - B, axis=0) / np.linalg.norm(B, axis=0)
    assert np.all(it == 1) and np.all(flags == 2), (it, flags)
    assert true_rel.max() <= 10 * tol, true_rel


@pytest.mark.parametrize("case_id", ["cg-6x5x4-b2-w17", "bicgstab-trans-5x5x4-b6-w3", "cg-13x13x13-b3-w32"])
def test_two_runs_and_check_every_give_the_same_bits(ctx, case_id):
    import rails_amd

    c = BJ.case(case_id)
    bsr, A = problem(c)
    op = rails_amd.HipOperatorWrapper.from_bsr(ctx, *bsr)
    inv = rails_amd.IterativeInverse(ctx, op, method=c.method, tol=0.0, maxit=1, block_jacobi=True)
    B = c.rhs()
    first = solve_k(ctx, inv, B, 5, c.trans)
    inv.set("check_every", 1)
    second = solve_k(ctx, inv, B, 5, c.trans)
    inv.set("check_every", 3)
    third = solve_k(ctx, inv, B, 5, c.trans)
    inv.close()
    assert all(np.array_equal(a, b) for a, b in zip(first, second)) and all(np.array_equal(a, b) for a, b in zip(first, third))
    assert np.all(first[1] == 5)
