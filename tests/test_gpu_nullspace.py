"""Nullspace deflation (the reference's opts.nullspace, matlab/RAILSsolver.m:33-34,221-222,311-313,527-529,538-616) on the HIP path, both
back ends, through the C ABI: the reference's acceptance test test_opts.m:197-216, agreement with the dense solution on the complement of
the kernel, warm starts, the projection methods, the M-orthogonal mode and the device work of the coordinate-space back end."""
import numpy as np
import pytest
import scipy.linalg as sl
import scipy.sparse as sp

import generalized_problems as G

pytestmark = pytest.mark.gpu


def neumann2(k):
    """the 2D Laplacian of a k x k grid with Neumann boundaries: negative semidefinite, kernel = the constants"""
    T = 2 * np.eye(k) - np.eye(k, k=1) - np.eye(k, k=-1)
    T[0, 0] = T[-1, -1] = 1.0
    return -(np.kron(np.eye(k), T) + np.kron(T, np.eye(k)))


def solver(ctx, A, B, params, subspace, M=None):
    import rails_amd

    op = rails_amd.HipOperatorWrapper(ctx, *G.csr(sp.csr_matrix(A)))
    mop = rails_amd.HipOperatorWrapper(ctx, *G.csr(sp.csr_matrix(M))) if M is not None else None
    s = rails_amd.Solver(ctx, op, B, M=mop)
    assert s.set_parameters(params) == 0
    s.set_option("verbose", 0)
    s.set_option("subspace", subspace)
    if M is not None:
        s.set_option("mass", 1)
    return s


@pytest.mark.parametrize("subspace", [1, 0])
def test_nullspace_acceptance(subspace):
    """test_opts.m:197-216: A = PAP, B = PB, M = PMP with P = I - QQ' for a random unit Q; opts.nullspace = Q.  The seed follows the
    convention of generalized_problems.CASES: one at which the CPU oracle meets the reference's bounds on the same problem solved without
    the option (at some seeds, 4634 among them, neither the oracle nor this solve converges in the 100 trips of the MATLAB defaults)."""
    import rails_amd

    n = 256
    g = np.random.default_rng(1)
    A = G.laplacian2(n).toarray()
    Md = g.uniform(0.0, 1.0, n)
    B = g.uniform(0.0, 1.0, (n, 1))
    Q = g.uniform(0.0, 1.0, (n, 1))
    Q /= np.linalg.norm(Q)
    P = np.eye(n) - Q @ Q.T
    A, B, M = P @ A @ P, np.asfortranarray(P @ B), P @ np.diag(Md) @ P
    ctx = rails_amd.Context(device=0, seed=1)
    s = solver(ctx, A, B, G.MATLAB_DEFAULTS, subspace, M=M)
    s.set_nullspace(Q)
    code, V, T = s.solve()
    assert s.nullspace_rank == 1
    assert np.linalg.norm(Q.T @ V, 2) < 1e-10
    scale = np.linalg.norm(B.T @ B, 2)
    res = abs(s.history()[-1]) / scale
    assert res * scale < 1e-2 and res < 1e-4, (code, res)
    X = V @ T @ V.T
    true_res = np.linalg.norm(A @ X @ M.T + M @ X @ A.T + B @ B.T, 2) / scale
    assert true_res < 1e-4, true_res
    s.close()
    ctx.close()


def complement_solution(A, B, N):
    """X_ref = Z Y Z' with Z an orthonormal basis of the complement of span(N) and (Z'AZ) Y + Y (Z'AZ)' + Z'BB'Z = 0"""
    Z = sl.null_space(N.T)
    Ar = Z.T @ A @ Z
    Y = sl.solve_continuous_lyapunov(Ar, -(Z.T @ B) @ (Z.T @ B).T)
    return Z @ Y @ Z.T


NEUMANN_PARAMS = {"Expand size": 3, "Lanczos iterations": 10, "Tolerance": 1e-8}


def neumann_problem(q):
    g = np.random.default_rng(10 + q)
    if q == 1:
        A = neumann2(16)
        N = np.ones((A.shape[0], 1))
    else:  # three disconnected Neumann blocks: the kernel is their three indicator vectors
        blocks = [neumann2(k) for k in (8, 10, 12)]
        A = sl.block_diag(*blocks)
        N = sl.block_diag(*[np.ones((b.shape[0], 1)) for b in blocks])
    B = g.uniform(-1, 1, (A.shape[0], 2))
    Nq = np.linalg.qr(N)[0]
    B = np.asfortranarray(B - Nq @ (Nq.T @ B))
    return A, B, N


@pytest.mark.parametrize("subspace", [1, 0])
@pytest.mark.parametrize("q", [1, 3])
def test_matches_the_dense_solution_on_the_complement(subspace, q):
    import rails_amd

    A, B, N = neumann_problem(q)
    ctx = rails_amd.Context(device=0, seed=5)
    s = solver(ctx, A, B, NEUMANN_PARAMS, subspace)
    s.set_nullspace(N)
    code, V, T = s.solve()
    assert code == 0 and s.nullspace_rank == q
    Nq = np.linalg.qr(N)[0]
    assert np.abs(Nq.T @ V).max() < 1e-10
    Xref = complement_solution(A, B, N)
    err = np.linalg.norm(V @ T @ V.T - Xref) / np.linalg.norm(Xref)
    print("q %d subspace %d: %d trips, ||VTV' - X_ref|| / ||X_ref|| = %.3e" % (q, subspace, s.trips(), err))
    assert err < 1e-5, err
    s.close()
    ctx.close()


@pytest.mark.parametrize("subspace", [1, 0])
def test_warm_start_is_deflated(subspace):
    import rails_amd

    A, B, N = neumann_problem(1)
    n = A.shape[0]
    g = np.random.default_rng(3)
    V0 = np.linalg.qr(g.uniform(-1, 1, (n, 4)) + 0.5)[0]  # components along the constants
    assert np.abs(N.T @ V0).max() > 1e-2
    ctx = rails_amd.Context(device=0, seed=6)
    s = solver(ctx, A, B, {**NEUMANN_PARAMS, "Restart from solution": 1}, subspace)
    s.set_nullspace(N)
    code, V, T = s.solve(V0=V0)
    assert code == 0
    assert np.abs(N.T @ V).max() / np.sqrt(n) < 1e-10
    assert np.abs(V.T @ V - np.eye(V.shape[1])).max() < 1e-10
    s.close()
    ctx.close()


@pytest.mark.parametrize("subspace", [1, 0])
@pytest.mark.parametrize("method", [1.2, 2.2])
def test_projection_methods_stay_orthogonal_to_the_nullspace(subspace, method):
    import rails_amd

    n = 256
    A = G.laplacian2(n)
    g = np.random.default_rng(8)
    B = np.asfortranarray(g.uniform(-1, 1, (n, 2)))
    N = g.uniform(-1, 1, (n, 2))
    ctx = rails_amd.Context(device=0, seed=8)
    s = solver(ctx, A.toarray(), B, {**NEUMANN_PARAMS, "Projection method": method}, subspace)
    lu = rails_amd.SparseLU(ctx, G.csr(A))
    s.set_inverse(lu)
    s.set_nullspace(N)
    s.set_option("max_trips", 6)
    code, V, T = s.solve()
    # blocks of A^-1 W are ill-conditioned against V: the block orthogonalisation leaves V'V = I, and N'V = 0 with it, to eps times their
    # condition (about 1e-9 measured); without the option N'V is of the order of the columns' entries
    Nq = np.linalg.qr(N)[0]
    print("method %g subspace %d: max |N'V| %.2e, max |V'V - I| %.2e" % (method, subspace, np.abs(Nq.T @ V).max(), np.abs(V.T @ V - np.eye(V.shape[1])).max()))
    assert V.shape[1] > 2 and np.abs(Nq.T @ V).max() < 1e-8
    assert np.abs(V.T @ V - np.eye(V.shape[1])).max() < 1e-8
    s.close()
    lu.close()
    ctx.close()


@pytest.mark.parametrize("subspace", [1, 0])
def test_mass_orthogonal_mode(subspace):
    """with opts.ortho = 'M' the nullspace is M-orthonormalised (a deliberate deviation): N'MV = 0 and V'MV = I.  A = PAP and B = PB as in
    the acceptance test, M diagonal and definite: the solution lies in the span of the generalized eigenvectors M-orthogonal to Q."""
    import rails_amd

    n = 256
    g = np.random.default_rng(1)
    A = G.laplacian2(n).toarray()
    Md = g.uniform(0.0, 1.0, n)
    B = g.uniform(0.0, 1.0, (n, 1))
    Q = g.uniform(0.0, 1.0, (n, 1))
    Q /= np.linalg.norm(Q)
    P = np.eye(n) - Q @ Q.T
    A, B, N = P @ A @ P, np.asfortranarray(P @ B), Q
    ctx = rails_amd.Context(device=0, seed=1)
    s = solver(ctx, A, B, {**G.MATLAB_DEFAULTS, "Maximum iterations": 300}, subspace, M=np.diag(Md))
    s.set_option("mass_orthogonalisation", 1)
    s.set_nullspace(N)
    code, V, T = s.solve()
    assert code == 0 and s.nullspace_rank == 1
    MV = Md[:, None] * V
    assert np.abs(N.T @ MV).max() <= 1e-10
    assert np.abs(V.T @ MV - np.eye(V.shape[1])).max() <= 1e-10
    s.close()
    ctx.close()


def test_coordinate_space_back_end_adds_no_device_work_per_trip():
    """Apart from the one absorb of N at the start, a trip with a nullspace runs what a trip without one runs (backend statistics): one
    materialise and one absorbed A*W block per trip, no one-by-one absorbs, no compress.  The two runs follow different trajectories, and
    each column that orthogonalize() replaces by a random direction (data-dependent, with or without a nullspace) costs one absorbed
    random column: those are counted by "replaced_columns" and taken out of the comparison."""
    import rails_amd

    n = 256
    A = G.laplacian2(n).toarray()
    g = np.random.default_rng(2)
    B = np.asfortranarray(g.uniform(-1, 1, (n, 2)))
    N = g.uniform(-1, 1, (n, 3))
    stats = []
    for with_n in (False, True):
        ctx = rails_amd.Context(device=0, seed=2)
        s = solver(ctx, A, B, {**NEUMANN_PARAMS, "Restart iterations": -1}, 1)
        if with_n:
            s.set_nullspace(N)
        s.set_option("max_trips", 12)
        code, V, T = s.solve()
        assert code == 2 and s.trips() == 12
        stats.append(s.backend_stats())
        s.close()
        ctx.close()
    without, with_n = stats
    print("without", without)
    print("with", with_n)
    assert with_n["absorb"] - with_n["replaced_columns"] == without["absorb"] - without["replaced_columns"] + 1, (without, with_n)
    assert with_n["absorb_columns"] - with_n["replaced_columns"] == without["absorb_columns"] - without["replaced_columns"] + N.shape[1], (without, with_n)
    for key in ("materialise", "one_by_one", "dropped", "compress"):
        assert with_n[key] == without[key], (key, without, with_n)


@pytest.mark.parametrize("subspace", [1, 0])
def test_refused_nullspace_leaves_the_solver_usable(subspace):
    import rails_amd

    A, B, N = neumann_problem(1)
    n = A.shape[0]
    ctx = rails_amd.Context(device=0, seed=9)
    s = solver(ctx, A, B, NEUMANN_PARAMS, subspace)
    s.set_nullspace(np.zeros((n, 2)))
    code, _, _ = s.solve(fetch=False)
    assert code == -2 and s.nullspace_rank == 0
    s.set_nullspace(None)
    s.set_nullspace(N)
    code, V, T = s.solve()
    assert code == 0 and s.nullspace_rank == 1
    s.close()
    ctx.close()
