"""Solver.solution(): the solution object of the last solve (rails_solution_from_solver, a device copy of V and the host T) against the
object built from the downloaded arrays, on both back ends, for the 3-D 7-point Laplacian; and its trace, which is trace(T) for an
orthonormal V and trace(T V'V) for an M-orthonormal one."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PARAMS = {"Expand size": 4, "Lanczos iterations": 10, "Tolerance": 1e-6}


@pytest.mark.parametrize("subspace", [0, 1])
def test_solution_of_the_last_solve(subspace):
    import rails_amd
    from rails_amd import problems as P

    ctx = rails_amd.Context(device=0, seed=5)
    A = P.laplace7(16, 16, 16)
    m = A[0].size - 1
    assert m == 4096
    B = P.rhs(m, 3, seed=2)
    op = rails_amd.HipOperatorWrapper(ctx, *A)
    solver = rails_amd.Solver(ctx, op, B)
    with pytest.raises(rails_amd.RailsError):
        solver.solution()  # nothing solved yet
    assert solver.set_parameters(PARAMS) == 0
    solver.set_option("verbose", 0)
    solver.set_option("subspace", subspace)
    code, V, T = solver.solve()
    assert code == 0
    k = V.shape[1]
    sol = solver.solution()
    ref = rails_amd.Solution(ctx, V, T)
    assert (sol.k, sol.m) == (k, m) == (ref.k, ref.m)
    np.testing.assert_array_equal(sol.U().to_host(), V)  # the same bits: a device copy
    np.testing.assert_array_equal(sol.S(), (T + T.T) / 2)
    np.testing.assert_array_equal(sol.variance(), ref.variance())
    assert sol.trace() == ref.trace()
    assert abs(sol.trace() - np.trace(T)) <= 1e-12 * abs(np.trace(T))  # V orthonormal
    la, Za = sol.eigs(6)
    lb, Zb = ref.eigs(6)
    np.testing.assert_array_equal(la, lb)
    np.testing.assert_array_equal(Za, Zb)
    # the object owns its copy: it outlives the solver and a second solve
    solver.close()
    X = V @ T @ V.T
    assert np.abs(sol.variance() - np.diag(X)).max() <= 1e-13 * np.abs(X).max() * k
    sol.close()
    ref.close()
    ctx.close()


def test_trace_with_mass_orthogonalisation():
    import rails_amd
    from rails_amd import problems as P

    ctx = rails_amd.Context(device=0, seed=5)
    A = P.laplace7(16, 16, 16)
    m = A[0].size - 1
    B = P.rhs(m, 3, seed=2)
    d = 1.0 + 0.5 * np.random.default_rng(0).uniform(size=m)  # diagonal SPD mass matrix
    op = rails_amd.HipOperatorWrapper(ctx, *A)
    Mop = rails_amd.HipOperatorWrapper(ctx, np.arange(m + 1, dtype=np.int64), np.arange(m, dtype=np.int32), d)
    solver = rails_amd.Solver(ctx, op, B, M=Mop)
    assert solver.set_parameters(PARAMS) == 0
    solver.set_option("verbose", 0)
    solver.set_option("mass", 1)
    solver.set_option("mass_orthogonalisation", 1)
    code, V, T = solver.solve()
    assert code == 0
    assert np.abs((V.T * d) @ V - np.eye(V.shape[1])).max() < 1e-10  # M-orthonormal, not orthonormal
    sol = solver.solution()
    want = np.trace(T @ (V.T @ V))
    assert abs(sol.trace() - want) <= 1e-12 * abs(want)
    sol.close()
    solver.close()
    ctx.close()
