"""The projection methods ("Projection method" 1.1 .. 2.3 with Solver.set_inverse) on the GPU with the iterative A^-1 operator
(rails_amd.IterativeInverse) in place of the device sparse LU: the structure of tests/test_gpu_projection.py.  Start spaces after one
trip against the splu inverse, acceptance on the MATLAB tests' Laplace 256 with a diagonal M by the reference's own four bounds
(test_Laplace.m:39-42) with conjugate gradients and BiCGStab and once with a loose inner tolerance, the refusal and the close order."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import generalized_problems as G

pytestmark = pytest.mark.gpu


def projector_residual(V, Y):
    return np.linalg.norm(Y - V @ (V.T @ Y)) / np.linalg.norm(Y)


def make(name="Laplace_256", subspace=1, mass=True, method="cg", tol=1e-10):
    import rails_amd

    A, Md, B, params, bound, seed = G.build(name)
    ctx = rails_amd.Context(device=0, seed=seed)
    op = rails_amd.HipOperatorWrapper(ctx, *G.csr(A))
    mop = rails_amd.HipOperatorWrapper(ctx, *G.diag_csr(Md)) if mass else None
    s = rails_amd.Solver(ctx, op, B, M=mop)
    s.set_option("verbose", 0)
    if mass:
        s.set_option("mass", 1)
    s.set_option("subspace", subspace)
    inv = rails_amd.IterativeInverse(ctx, G.csr(A), method=method, tol=tol) if method else None
    return ctx, A, Md, B, params, bound, s, inv


@pytest.mark.parametrize("subspace", [1, 0])
def test_start_spaces_after_one_trip(subspace):
    ctx, A, Md, B, params, bound, s, inv = make(subspace=subspace, mass=False, tol=1e-12)
    lu = spla.splu(sp.csc_matrix(A))
    Ai = lambda Y: lu.solve(np.asfortranarray(Y))
    s.set_inverse(inv)
    s.set_option("max_trips", 1)
    p = B.shape[1]
    assert s.set_parameters({**params, "Projection method": 1.2}) == 0
    _, V, _ = s.solve()
    assert V.shape[1] == p and projector_residual(V, Ai(B)) <= 1e-8
    assert s.set_parameters({**params, "Projection method": 2.2}) == 0
    _, V, _ = s.solve()
    assert V.shape[1] == 2 * p and projector_residual(V, np.hstack([B, Ai(B)])) <= 1e-8
    V0 = np.linalg.qr(np.random.default_rng(4).standard_normal((A.shape[0], 2)))[0]
    for method, want in ((1.1, Ai(V0)), (2.1, np.hstack([V0, Ai(V0)]))):
        assert s.set_parameters({**params, "Projection method": method, "Restart from solution": 1}) == 0
        _, V, _ = s.solve(V0=V0)
        assert V.shape[1] == want.shape[1] and projector_residual(V, want) <= 1e-8, method
    assert inv.stats()["total_flagged_columns"] == 0
    s.close()
    inv.close()
    ctx.close()


@pytest.mark.parametrize("subspace", [1, 0])
@pytest.mark.parametrize("method,inner", [(1.2, "cg"), (2.2, "cg"), (2.3, "cg"), (2.2, "bicgstab")])
def test_acceptance_laplace_256(method, inner, subspace):
    """the four bounds of test_Laplace.m:39-42 (true residual below 1e-4, trips below n - 10); the trip counts are recorded next to those
    of the LU run, not asserted"""
    import rails_amd

    ctx, A, Md, B, params, bound, s, inv = make(subspace=subspace, method=inner)
    s.set_inverse(inv)
    assert s.set_parameters({**params, "Projection method": method}) == 0
    code, V, T = s.solve()
    assert code == 0
    G.check_acceptance(A, Md, B, V, T, abs(s.history()[-1]), s.trips(), bound)
    trips = s.trips()
    st = inv.stats()
    lu = rails_amd.SparseLU(ctx, G.csr(A))
    s.set_inverse(lu)
    assert s.set_parameters({**params, "Projection method": method}) == 0
    code_lu, _, _ = s.solve()
    print("method %g, %s, subspace %d: %d trips (LU: %d, code %d); %d inner solves, %d inner iterations, %d flagged columns" % (
        method, inner, subspace, trips, s.trips(), code_lu, st["total_solves"], st["total_iterations"], st["total_flagged_columns"]))
    s.close()
    lu.close()
    inv.close()
    ctx.close()


@pytest.mark.parametrize("subspace", [1, 0])
def test_acceptance_with_a_loose_inverse(subspace):
    """method 2.2 with the inverse at 1e-4: the reference allows an approximate inverse (matlab/RAILSsolver.m:19-23); only convergence and
    the reference's bounds are asserted"""
    ctx, A, Md, B, params, bound, s, inv = make(subspace=subspace, tol=1e-4)
    s.set_inverse(inv)
    assert s.set_parameters({**params, "Projection method": 2.2}) == 0
    code, V, T = s.solve()
    assert code == 0
    G.check_acceptance(A, Md, B, V, T, abs(s.history()[-1]), s.trips(), bound)
    print("method 2.2, inverse at 1e-4, subspace %d: %d trips, %d inner iterations" % (subspace, s.trips(), inv.stats()["total_iterations"]))
    s.close()
    inv.close()
    ctx.close()


def test_refusal_of_an_inverse_of_the_wrong_row_count():
    import rails_amd

    ctx, A, Md, B, params, bound, s, inv = make()
    other = rails_amd.IterativeInverse(ctx, G.csr(G.laplacian2(64)), method="cg")
    with pytest.raises(rails_amd.RailsError, match="rows"):
        s.set_inverse(other)
    other.close()
    s.close()
    inv.close()
    ctx.close()


@pytest.mark.parametrize("inverse_first", [True, False])
def test_close_order(inverse_first):
    ctx, A, Md, B, params, bound, s, inv = make(mass=False)
    s.set_inverse(inv)
    s.set_option("max_trips", 2)
    assert s.set_parameters({**params, "Projection method": 2.2}) == 0
    s.solve()
    if inverse_first:
        inv.close()
        s.close()
    else:
        s.close()
        inv.close()
    ctx.close()
