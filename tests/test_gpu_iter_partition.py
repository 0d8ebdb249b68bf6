"""Converged solves of the iterative A^-1 operator on a row partition, and its refusals there.  Ranks are threads on one device
(tests/test_gpu_partition.py's emulation).  The bounds are those of tests/test_gpu_iter.py: the true relative residual of the stacked
result at most 10 times the tolerance, iteration counts at most 1.5 times the restatement's (tests/iter_reference.py)."""
import numpy as np
import pytest

import iter_partition_cases as PC
import iter_reference as R

pytestmark = pytest.mark.gpu

TOL = 1e-10
EINVAL = r"\(code -1\)"


@pytest.mark.parametrize("nranks", PC.RANKS)
@pytest.mark.parametrize("nc", (3, 33))
@pytest.mark.parametrize("tag", ["a", "c"])  # conjugate gradients on the 2-D Laplacian, BiCGStab on convection-diffusion
def test_partitioned_solves_converge(tag, nc, nranks):
    import rails_amd

    A, Bm, Xr, cr = R.reference(tag, nc)
    method = R.problem(tag)[1]

    def work(r, ctx, op, plan, r0, r1):
        inv = rails_amd.IterativeInverse(ctx, op, method=method, tol=TOL, maxit=5000)
        Bl = rails_amd.HipMultiVectorWrapper(ctx, data=Bm[r0:r1])
        X = inv.solve(Bl).to_host()
        cols = [a.copy() for a in inv.columns()]
        Xop = inv.op.apply(Bl).to_host()  # the operator handle: what Solver.set_inverse uses
        out = dict(X=X, Xop=Xop, cols=cols, cols_op=[a.copy() for a in inv.columns()], stats=inv.stats())
        inv.close()
        return out

    res = PC.run_ranks(nranks, PC.csr_triple(A), work)
    it, rel, flags = res[0]["cols"]
    for r in range(nranks):
        for a, b, c in zip(res[r]["cols"], res[0]["cols"], res[r]["cols_op"]):
            assert np.array_equal(a, b) and np.array_equal(a, c)  # the same scalars on every rank, the same solve through the handle
        assert np.array_equal(res[r]["X"], res[r]["Xop"])
        assert res[r]["stats"]["unconverged_columns"] == 0
    X = np.vstack([res[r]["X"] for r in range(nranks)])
    true_rel = R.true_relres(A, X, Bm)
    print("problem (%s), %d columns, %d ranks: iterations %d..%d (restatement %d..%d), true relative residual %.2e" % (
        tag, nc, nranks, it.min(), it.max(), cr.iter.min(), cr.iter.max(), true_rel.max()))
    assert np.all(np.isfinite(X)) and true_rel.max() <= 10 * TOL, true_rel.max()
    assert np.all(flags == 2) and np.all(rel <= TOL)
    assert np.all(it <= 1.5 * cr.iter), (it, cr.iter)


@pytest.mark.parametrize("nranks", PC.RANKS)
def test_a_nan_that_one_rank_owns_is_refused_on_every_rank(nranks):
    """the count of non-finite columns comes from all-reduced sums: every rank returns RAILS_EINVAL at the same point, nobody is left at
    a barrier, and the objects go on to solve"""
    import rails_amd
    from rails_amd import partition

    A, Bm, Xr, cr = R.reference("a", 3)
    starts = partition.row_ranges(A.shape[0], nranks)
    bad = Bm.copy()
    bad[int(starts[1]) + 2, 1] = np.nan  # a row of rank 1 alone

    def work(r, ctx, op, plan, r0, r1):
        inv = rails_amd.IterativeInverse(ctx, op, method="cg", tol=TOL, maxit=5000)
        with pytest.raises(rails_amd.RailsError, match=EINVAL + ".*not finite"):
            inv.solve(rails_amd.HipMultiVectorWrapper(ctx, data=bad[r0:r1]))
        X = inv.solve(rails_amd.HipMultiVectorWrapper(ctx, data=Bm[r0:r1])).to_host()
        flags = inv.columns()[2].copy()
        inv.close()
        return X, flags

    res = PC.run_ranks(nranks, PC.csr_triple(A), work)
    X = np.vstack([res[r][0] for r in range(nranks)])
    assert R.true_relres(A, X, Bm).max() <= 10 * TOL and all(np.all(res[r][1] == 2) for r in range(nranks))


def test_transposed_solve_is_refused_before_any_collective():
    import rails_amd

    A, Bm, Xr, cr = R.reference("c", 3)

    def work(r, ctx, op, plan, r0, r1):
        inv = rails_amd.IterativeInverse(ctx, op, method="bicgstab", tol=TOL)
        Bl = rails_amd.HipMultiVectorWrapper(ctx, data=Bm[r0:r1])
        n0 = ctx.stats()["allreduce"]
        with pytest.raises(rails_amd.RailsError, match=EINVAL + ".*transposed"):
            inv.solve(Bl, trans=True)
        moved = ctx.stats()["allreduce"] - n0
        inv.close()
        return moved

    assert PC.run_ranks(2, PC.csr_triple(A), work) == [0, 0]


def test_a_partition_without_hook_or_communicator_is_refused():
    """What tests/test_gpu_iter.py::test_refusals asserts, restated here with its reason: without an all-reduce hook or a communicator the
    first inner product would fail with RAILS_ECOMM, so the object is refused when it is made -- the hook or communicator has to be
    installed first."""
    import rails_amd

    A, Bm, Xr, cr = R.reference("a", 3)
    n = A.shape[0]
    ctx = rails_amd.Context(device=0, seed=1)
    try:
        ctx.set_partition(0, 2, 0, 2 * n)
        op = rails_amd.HipOperatorWrapper(ctx, A.indptr, A.indices, A.data)
        with pytest.raises(rails_amd.RailsError, match=EINVAL + ".*single GPU"):
            rails_amd.IterativeInverse(ctx, op, method="cg")
        del op
    finally:
        ctx.close()


def test_matrix_forms_are_refused_on_a_partitioned_context():
    import rails_amd

    A, Bm, Xr, cr = R.reference("a", 3)
    ctx = rails_amd.Context(device=0, seed=1)
    try:
        ctx.set_partition(0, 2, 0, A.shape[0])
        ctx.set_allreduce(lambda ptr, n, stream: 0)
        with pytest.raises(ValueError, match="operator wrapper"):
            rails_amd.IterativeInverse(ctx, A, method="cg")
        with pytest.raises(ValueError, match="operator wrapper"):
            rails_amd.IterativeInverse(ctx, (A.indptr, A.indices, A.data))
    finally:
        ctx.close()


def test_auto_on_a_wrapper_stays_an_error():
    import rails_amd

    A, Bm, Xr, cr = R.reference("a", 3)

    def work(r, ctx, op, plan, r0, r1):
        with pytest.raises(ValueError, match="name the method"):
            rails_amd.IterativeInverse(ctx, op)
        return True

    assert PC.run_ranks(2, PC.csr_triple(A), work) == [True, True]
