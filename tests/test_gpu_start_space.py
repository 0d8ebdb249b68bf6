"""Continuation runs on the GPU, both back ends, through the C ABI (include/rails_solver.h): "Restart upon start"
(opts.restart_upon_start of matlab/RAILSsolver.m:53-57,455) against numpy's prediction of what the shrink keeps, and
rails_solver_set_start_space (opts.space, :25-28): a start space that is neither orthonormal nor independent, given as a device
multivector or as a solution object, with and without a nullspace."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PARAMS = {"Expand size": 2, "Lanczos iterations": 8, "Tolerance": 1e-6, "Restart tolerance": 1e-10}


def banded_problem(n=200, p=2, seed=3):
    """a banded stable A (five diagonals, diagonally dominant) and B = U(-1, 1)^{n x p}"""
    g = np.random.default_rng(seed)
    A = np.zeros((n, n))
    for d in (-2, -1, 1, 2):
        A += np.diag(g.uniform(-1, 1, n - abs(d)), d)
    A -= np.diag(g.uniform(2.5, 6.0, n))
    return A, np.asfortranarray(g.uniform(-1, 1, (n, p)))


def csr(A):
    import scipy.sparse as sp

    S = sp.csr_matrix(A)
    return S.indptr.astype(np.int64), S.indices.astype(np.int32), S.data.astype(np.float64)


@pytest.fixture(scope="module")
def ctx():
    import rails_amd

    c = rails_amd.Context(device=0, seed=1)
    yield c
    c.close()


def make(ctx, A, B, subspace, params=PARAMS, seed=1):
    import rails_amd

    ctx.set_seed(seed, 0)
    s = rails_amd.Solver(ctx, rails_amd.HipOperatorWrapper(ctx, *csr(A)), B)
    assert s.set_parameters(params) == 0
    s.set_option("verbose", 0)
    s.set_option("subspace", subspace)
    return s


@pytest.fixture(scope="module")
def first_solution(ctx):
    """(A, B, V1, T1, trips of the cold solve), computed once on the direct back end and handed out read-only"""
    A, B = banded_problem()
    s = make(ctx, A, B, 0)
    code, V1, T1 = s.solve()
    assert code == 0
    trips = s.trips()
    s.close()
    for a in (A, B, V1, T1):
        a.setflags(write=False)
    return A, B, V1, T1, trips


def gap_tolerance(moduli):
    """the geometric mean of two neighbouring moduli that differ by at least a factor of 10 -- of such gaps the one nearest the middle
    of the spectrum: the count of moduli above it cannot flip on rounding, and the eigenvectors above it span a well separated space"""
    mods = np.sort(np.abs(moduli))[::-1]
    gaps = [i for i in range(mods.size - 1) if mods[i] >= 10.0 * mods[i + 1]]
    assert gaps, mods
    i = min(gaps, key=lambda j: abs(2 * (j + 1) - mods.size))
    return float(np.sqrt(mods[i] * mods[i + 1])), i + 1


def restart_prediction(T0, tol, reduced_size):
    """what compute_restart_vectors keeps: eigenvectors of T0 for the `reduced_size` eigenvalues of largest modulus, those above tol"""
    lam, Z = np.linalg.eigh(T0, UPLO="U")  # the triangle compute_restart_vectors reads
    order = np.argsort(-np.abs(lam), kind="stable")
    if reduced_size > 0:
        order = order[:reduced_size]
    order = [i for i in order if abs(lam[i]) > tol]
    return len(order), Z[:, order]


def warm_solve(s, V1, subspace):
    """a warm start from the orthonormal V1.  On the direct back end the plain one (rails_solver_set_V).  The coordinate-space back end
    takes V1 as a start space: a converged solution holds B to within the tolerance (1e-6 here), and the plain warm start there absorbs
    such a block through the overlapped orthogonalisation, which ends the run when a block does not confirm its prediction (as this one
    does not); the start space is absorbed the waiting way.  V1 is orthonormal, so its range basis is V1 itself."""
    if not subspace:
        return s.solve(V0=V1)
    s.set_start_space(V1)
    return s.solve()


@pytest.mark.parametrize("subspace", [1, 0])
@pytest.mark.parametrize("capped", [False, True])
def test_restart_upon_start_keeps_what_numpy_predicts(ctx, first_solution, subspace, capped):
    A, B, V1, T1, _ = first_solution
    # (a tolerance V1 does not meet: a run that has converged after its first projected solve stops there, before any shrink)
    one = {**PARAMS, "Restart from solution": 1, "Minimize solution space": 0, "Tolerance": 1e-13}
    # (a) one trip from V1: the reduced solution T0 on span(V1)
    s = make(ctx, A, B, subspace, one)
    s.set_option("max_trips", 1)
    code, Va, T0 = warm_solve(s, V1, subspace)
    assert s.trips() == 1 and Va.shape[1] == V1.shape[1]
    tol, above = gap_tolerance(np.linalg.eigvalsh(T0, UPLO="U"))
    reduced = above - 2 if capped else -1
    k1, X = restart_prediction(T0, tol, reduced)
    assert k1 == (above - 2 if capped else above) and 1 < k1 < Va.shape[1]
    # (b) the same with the shrink after the first projected solve, and one more trip
    assert s.set_parameters({**one, "Restart upon start": 1, "Restart tolerance": tol, "Reduced size": reduced}) == 0
    s.set_option("max_trips", 2)
    ctx.set_seed(1, 0)
    code, V, T = warm_solve(s, V1, subspace)
    assert s.trips() == 2
    assert V.shape[1] == k1  # (the parent commit ignores the parameter and returns every column)
    VX = Va @ X
    print("span %.2e" % np.abs(V - VX @ (VX.T @ V)).max())
    assert np.abs(V - VX @ (VX.T @ V)).max() < 1e-10
    proj = V.T @ A @ V @ T + T @ V.T @ A.T @ V + V.T @ B @ B.T @ V
    print("projected equation %.2e of %.2e" % (np.abs(proj).max(), np.linalg.norm(B, 2) ** 2))
    assert np.abs(proj).max() <= 1e-9 * np.linalg.norm(B, 2) ** 2
    s.close()


@pytest.mark.parametrize("subspace", [1, 0])
@pytest.mark.parametrize("form", ["multivector", "solution", "host"])
def test_raw_start_space(ctx, first_solution, subspace, form):
    import rails_amd

    A, B, V1, T1, cold_trips = first_solution
    s = make(ctx, A, B, subspace)
    if form == "solution":
        sol = rails_amd.Solution(ctx, V1, T1)
        s.set_start_space(sol)
        rank = V1.shape[1]
    else:
        G = np.random.default_rng(8).uniform(-1, 1, (3, 3))
        S = np.hstack([V1, B, V1[:, :3] @ G])  # neither orthonormal nor independent
        rank = np.linalg.matrix_rank(S / np.linalg.norm(S, axis=0), tol=1e-8)
        assert rank == V1.shape[1] + B.shape[1]
        s.set_start_space(rails_amd.HipMultiVectorWrapper(ctx, data=S) if form == "multivector" else S)
    code, V, T = s.solve()
    assert code == 0
    assert s.start_rank == rank
    # V'V - I.  Direct back end: V's columns come out of the block orthogonalisations themselves, rounding level.  Coordinate-space back
    # end: V = P c with c orthonormal to rounding, so the defect is that of the device basis P, which holds B's columns first; a start space
    # that is a converged solution contains B up to the first solve's tolerance f = 1e-6, its block keeps that fraction of two directions
    # once B's columns are projected out, and what is left of a direction inherits the rounding of the projection magnified by 1 / f
    # (DESIGN.md section 5 (vi)): eps / f.
    bound = np.finfo(float).eps / PARAMS["Tolerance"] if subspace else 1e-12
    print("orthonormality %.2e (bound %.1e)" % (np.abs(V.T @ V - np.eye(V.shape[1])).max(), bound))
    assert np.abs(V.T @ V - np.eye(V.shape[1])).max() < bound
    assert s.relative_residual() < 1e-3  # the bound of the warm start in tests/test_gpu_solver.py
    assert s.trips() <= cold_trips
    assert bool(s.backend_stats()) == bool(subspace)
    # the space is consumed: the next solve is a cold start
    code, V, T = s.solve()
    assert code == 0 and s.start_rank == 1
    s.close()


def test_solution_of_the_solver_as_start_space_of_a_similar_problem(ctx, first_solution):
    import rails_amd

    A, B, _, _, _ = first_solution
    s = make(ctx, A, B, 1)
    code, V1, T1 = s.solve()
    assert code == 0
    sol = s.solution()
    A2 = A + 0.01 * np.diag(np.diag(A))
    cold = make(ctx, A2, B, 1)
    assert cold.solve(fetch=False)[0] == 0
    warm = make(ctx, A2, B, 1, {**PARAMS, "Restart upon start": 1})
    warm.set_start_space(sol)
    code, V, T = warm.solve()
    assert code == 0 and warm.start_rank == V1.shape[1] and warm.trips() <= cold.trips()
    assert warm.relative_residual() < 1e-3
    for x in (sol, s, cold, warm):
        x.close()


@pytest.mark.parametrize("subspace", [1, 0])
def test_start_space_with_a_nullspace(ctx, subspace):
    """the singular problem of tests/test_gpu_nullspace.py (2D Neumann Laplacian, kernel = the constants) with a start space that
    contains the nullspace vector itself: that column goes; the solve runs on the direct back end whatever the option says"""
    k = 16
    Tm = 2 * np.eye(k) - np.eye(k, k=1) - np.eye(k, k=-1)
    Tm[0, 0] = Tm[-1, -1] = 1.0
    A = -(np.kron(np.eye(k), Tm) + np.kron(Tm, np.eye(k)))
    n = A.shape[0]
    N = np.ones((n, 1)) / np.sqrt(n)
    B = np.random.default_rng(11).uniform(-1, 1, (n, 2))
    B = np.asfortranarray(B - N @ (N.T @ B))
    params = {"Expand size": 3, "Lanczos iterations": 10, "Tolerance": 1e-8}
    s = make(ctx, A, B, subspace, params)
    s.set_nullspace(np.ones((n, 1)))
    code, V1, T1 = s.solve()
    assert code == 0 and s.nullspace_rank == 1
    S = np.hstack([V1[:, :5], np.ones((n, 1)), V1[:, 5:], V1[:, :2] @ np.array([[1.0, 2.0], [-3.0, 0.5]])])
    rank = np.linalg.matrix_rank(S / np.linalg.norm(S, axis=0), tol=1e-8)
    assert rank == V1.shape[1] + 1
    s.set_start_space(S)
    code, V, T = s.solve()
    assert code == 0 and s.start_rank == rank - 1
    assert s.backend_stats() == {}
    assert np.abs(N.T @ V).max() < 1e-12
    assert np.abs(V.T @ V - np.eye(V.shape[1])).max() < 1e-12
    s.close()


def test_refusals(ctx, first_solution):
    import rails_amd

    A, B, V1, _, _ = first_solution
    n = A.shape[0]
    s = make(ctx, A, B, 1)
    with pytest.raises(rails_amd.RailsError, match="rows"):
        s.set_start_space(np.ones((n + 1, 2)))
    with pytest.raises(rails_amd.RailsError):
        s.set_start_space(rails_amd.HipMultiVectorWrapper(ctx, n, 0, capacity=4))
    # a start space of which nothing survives: the solve is refused and V, T stay what they were
    code, V, T = s.solve()
    assert code == 0
    s.set_start_space(np.zeros((n, 2)))
    code, V2, T2 = s.solve()
    assert code == -2 and np.array_equal(V, V2) and np.array_equal(T, T2)
    s.close()
