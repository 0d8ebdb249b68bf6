"""The projection methods above 1 on a row partition: "Projection method" 2.2 and 1.2 with a conjugate-gradients inverse at 1e-8, with
and without its Chebyshev polynomial, on 2 and 3 ranks and both back ends, against the single-rank GPU run of the same code with the same
inverse, under the bounds tests/test_gpu_partition.py::test_partitioned_solve_matches_oracle_and_single_rank uses at Tolerance 1e-3.
Ranks are threads on one device (that module's emulation)."""
import numpy as np
import pytest

import iter_partition_cases as PC

pytestmark = pytest.mark.gpu

# laplace7(12, 12, 9): 1296 rows, planes of 144, so every rank of 2 and of 3 has ghost rows; B of 4 columns.  The single-rank runs take
# 5 (method 2.2) and 11 (method 1.2) trips on either back end, with and without the polynomial.
GRID = (12, 12, 9)
PARAMS = {"Restart size": 64, "Reduced size": 32, "Expand size": 4, "Lanczos iterations": 8, "Tolerance": 1e-3}
SEED = 3
INNER_TOL = 1e-8
_single = {}


def problem():
    from rails_amd import problems as P

    A = P.laplace7(*GRID)
    m = A[0].size - 1
    return A, m, P.rhs(m, 4, seed=5)


def solve(ctx, op, Bl, m, method, poly, subspace):
    import rails_amd

    s = rails_amd.Solver(ctx, op, Bl, m_global=m)
    assert s.set_parameters({**PARAMS, "Projection method": method}) == 0
    s.set_option("verbose", 0)
    s.set_option("subspace", subspace)
    inv = rails_amd.IterativeInverse(ctx, op, method="cg", tol=INNER_TOL, poly_degree=poly)
    s.set_inverse(inv)
    code, V, T = s.solve()
    out = dict(code=code, V=V, T=T, hist=np.asarray(s.history()).copy(), trips=s.trips(), rel=s.relative_residual(), inv=inv.stats())
    s.close()
    inv.close()
    return out


def single(method, poly, subspace):
    key = (method, poly, subspace)
    if key not in _single:
        import rails_amd

        A, m, B = problem()
        ctx = rails_amd.Context(device=0, seed=SEED)
        try:
            _single[key] = solve(ctx, rails_amd.HipOperatorWrapper(ctx, *A), B, m, method, poly, subspace)
        finally:
            ctx.close()
    return _single[key]


@pytest.mark.parametrize("subspace", [1, 0])
@pytest.mark.parametrize("nranks", PC.RANKS)
@pytest.mark.parametrize("poly", [0, 4])
@pytest.mark.parametrize("method", [2.2, 1.2])
def test_projection_methods_on_a_partition(method, poly, nranks, subspace):
    A, m, B = problem()
    one = single(method, poly, subspace)
    assert one["code"] == 0 and one["trips"] < 15 and one["inv"]["total_flagged_columns"] == 0

    def work(r, ctx, op, plan, r0, r1):
        return solve(ctx, op, B[r0:r1], m, method, poly, subspace)

    res = PC.run_ranks(nranks, A, work, seed=SEED)
    V = np.vstack([res[r]["V"] for r in range(nranks)])
    T = res[0]["T"]
    for r in range(nranks):
        assert res[r]["code"] == 0
        assert abs(res[r]["trips"] - one["trips"]) <= 1 and res[r]["trips"] == res[0]["trips"]
        assert np.array_equal(res[r]["T"], T) and np.array_equal(res[r]["hist"], res[0]["hist"])  # replicated
        assert res[r]["inv"]["total_flagged_columns"] == 0
        assert res[r]["inv"]["total_iterations"] == res[0]["inv"]["total_iterations"]
    X, X1 = V @ T @ V.T, one["V"] @ one["T"] @ one["V"].T
    diff = np.linalg.norm(X - X1) / np.linalg.norm(X1)
    print("method %g, degree %d, %d ranks, subspace %d: %d trips (one rank: %d), |X - X_1| / |X_1| = %.2e, %d inner iterations" % (
        method, poly, nranks, subspace, res[0]["trips"], one["trips"], diff, res[0]["inv"]["total_iterations"]))
    assert diff <= 1e-2
    assert res[0]["rel"] < 5e-3
    assert np.abs(V.T @ V - np.eye(V.shape[1])).max() < 1e-10
