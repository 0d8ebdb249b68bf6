"""The projection methods ("Projection method" 1.1 .. 2.3 with Solver.set_inverse; matlab/RAILSsolver.m:7-24,288-314,520-530) on the
GPU, both back ends, through the C ABI with the device sparse LU as A^-1: the start spaces and expansions, acceptance on the MATLAB
tests' Laplace 256 with a diagonal M, and the refusals."""
import numpy as np
import pytest

import generalized_problems as G

pytestmark = pytest.mark.gpu

METHODS = (1.1, 1.2, 1.3, 2.1, 2.2, 2.3)


def projector_residual(V, Y):
    return np.linalg.norm(Y - V @ (V.T @ Y)) / np.linalg.norm(Y)


def make(name="Laplace_256", subspace=1, mass=True):
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
    lu = rails_amd.SparseLU(ctx, G.csr(A))
    return ctx, A, Md, B, params, bound, s, lu


@pytest.mark.parametrize("subspace", [1, 0])
def test_start_spaces_after_one_trip(subspace):
    ctx, A, Md, B, params, bound, s, lu = make(subspace=subspace, mass=False)
    Ai = lambda Y: lu.lu.solve(np.asfortranarray(Y))
    s.set_inverse(lu)
    s.set_option("max_trips", 1)
    p = B.shape[1]
    assert s.set_parameters({**params, "Projection method": 1.2}) == 0
    _, V, _ = s.solve()
    assert V.shape[1] == p and projector_residual(V, Ai(B)) <= 1e-10
    assert s.set_parameters({**params, "Projection method": 2.2}) == 0
    _, V, _ = s.solve()
    assert V.shape[1] == 2 * p and projector_residual(V, np.hstack([B, Ai(B)])) <= 1e-10
    V0 = np.linalg.qr(np.random.default_rng(4).standard_normal((A.shape[0], 2)))[0]
    for method, want in ((1.1, Ai(V0)), (2.1, np.hstack([V0, Ai(V0)]))):
        assert s.set_parameters({**params, "Projection method": method, "Restart from solution": 1}) == 0
        _, V, _ = s.solve(V0=V0)
        assert V.shape[1] == want.shape[1] and projector_residual(V, want) <= 1e-10, method
    assert s.set_parameters({**params, "Projection method": 2.3, "Restart from solution": 1}) == 0
    _, V, _ = s.solve(V0=V0)
    assert V.shape == V0.shape and np.abs(V - V0).max() <= 1e-10
    assert np.abs(V.T @ V - np.eye(V.shape[1])).max() < 1e-10
    s.close()
    lu.close()
    ctx.close()


@pytest.mark.parametrize("subspace", [1, 0])
@pytest.mark.parametrize("method,per", [(1.2, 1), (2.2, 2), (1.3, 1), (2.3, 2)])
def test_columns_added_per_trip(subspace, method, per):
    ctx, A, Md, B, params, bound, s, lu = make(subspace=subspace, mass=False)
    s.set_inverse(lu.op)
    e = 3
    widths = []
    for trips in (1, 2):
        assert s.set_parameters({**params, "Expand size": e, "Projection method": method}) == 0
        s.set_option("max_trips", trips)
        _, V, _ = s.solve()
        widths.append(V.shape[1])
        assert np.abs(V.T @ V - np.eye(V.shape[1])).max() < 1e-10
    assert widths[1] - widths[0] == per * e, widths  # (nothing is dropped without mass orthogonalisation)
    s.close()
    lu.close()
    ctx.close()


@pytest.mark.parametrize("morth", [0, 1])
@pytest.mark.parametrize("subspace", [1, 0])
@pytest.mark.parametrize("method", METHODS)
def test_acceptance_laplace_256(method, subspace, morth):
    """the four bounds of test_Laplace.m:39-42 (true residual below 1e-4, trips below n - 10) with every method, once more with
    mass_orthogonalisation (opts.ortho = 'M')"""
    ctx, A, Md, B, params, bound, s, lu = make(subspace=subspace)
    s.set_inverse(lu)
    assert s.set_parameters({**params, "Projection method": method}) == 0
    if morth:
        s.set_option("mass_orthogonalisation", 1)
    code, V, T = s.solve()
    assert code == 0
    if morth:
        assert np.abs(V.T @ (Md[:, None] * V) - np.eye(V.shape[1])).max() < 1e-10
    G.check_acceptance(A, Md, B, V, T, abs(s.history()[-1]), s.trips(), bound)
    s.close()
    lu.close()
    ctx.close()


@pytest.mark.parametrize("subspace", [1, 0])
def test_refusals(subspace):
    import rails_amd

    ctx, A, Md, B, params, bound, s, lu = make(subspace=subspace)
    assert s.set_parameters({**params, "Projection method": 1.5}) != 0  # no such method
    assert s.set_parameters({**params, "Projection method": 2.2}) == 0
    with pytest.raises(rails_amd.RailsError, match="needs an inverse"):  # a method above 1 without an inverse
        s.solve()
    other = rails_amd.SparseLU(ctx, G.csr(G.laplacian2(64)))
    with pytest.raises(rails_amd.RailsError, match="rows"):  # an inverse of the wrong row count
        s.set_inverse(other)
    other.close()
    s.set_inverse(lu)
    assert s.set_parameters({**params, "Projection method": 1.0}) == 0
    s.set_option("max_trips", 1)
    code, V, T = s.solve()  # method 1 with an inverse set: the inverse is not used
    assert V.shape[1] == 1
    s.close()
    lu.close()
    ctx.close()
