"""Solves with a sparse right-hand side (rails_amd.SparseRHS, rails_solver_create_sparse) on the GPU, checked in dense numpy on a
256-row problem: laplace7(16, 16, 1) with B "selection" (p = 40) and the same A minus 2 I with B "mixed" (p = 130, more columns than the
dense fused Lanczos takes).  All cases: Tolerance 1e-4, Expand size 16, Lanczos iterations 40, no Restart size.  Both solves pass 128
basis columns (NCH = 2 of the pass kernel) and shrink on first convergence, so the rotation of the p-row B'V is exercised.  Also the
variants (mass matrix, warm start, nullspace, projection method 2.3), the refusals, and the driver's --sparse-B."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import lanczos_steps_device as D
import sparse_rhs_reference as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4
PARAMS = {"Tolerance": TOL, "Expand size": 16, "Lanczos iterations": 40}
M_ROWS = 256


def problem(which):
    from rails_amd import problems as P

    rowptr, col, val = P.laplace7(16, 16, 1)
    A = sp.csr_matrix((val, col, rowptr), shape=(M_ROWS, M_ROWS))
    if which == "mixed":
        return sp.csr_matrix(A - 2.0 * sp.identity(M_ROWS)), S.make_B("mixed", M_ROWS, 130)
    return A, S.make_B("selection", M_ROWS, 40)


def csr(A):
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data.astype(np.float64)


@pytest.fixture(scope="module")
def ctx():
    import rails_amd

    c = rails_amd.Context(device=0, seed=1)
    yield c
    c.close()


def residual(Ad, Bd, V, T, Md=None):
    X = V @ T @ V.T
    if Md is None:
        return Ad @ X + X @ Ad.T + Bd @ Bd.T
    return Ad @ X @ Md.T + Md @ X @ Ad.T + Bd @ Bd.T


def check_solution(s, code, V, T, Ad, Bd, Md=None, what=""):
    """return code 0, V'V = I to 1e-10, T = T', ||R||_2 <= 2 tol ||B||_2^2 in dense numpy (the factor of tests/test_gpu_configs.py),
    relative_residual() within 1e-6 of numpy's, the solver's scale within 1e-4 relative of ||B||_2^2 and not above it"""
    assert code == 0, (what, code)
    k = V.shape[1]
    assert np.abs(V.T @ V - np.eye(k)).max() <= 1e-10
    assert np.abs(T - T.T).max() <= 1e-12 * np.abs(T).max()
    nb2 = float(np.linalg.norm(Bd, 2) ** 2)
    R = residual(Ad, Bd, V, T, Md)
    r2 = float(np.linalg.norm(R, 2))
    rel_np = float(np.linalg.norm(R, "fro") / np.linalg.norm(Bd.T @ Bd, "fro"))
    rel = s.relative_residual()
    scale = s.scale()
    print("%s: %d trips, %d columns, ||R||_2 / (tol ||B||^2) = %.3g, relative residual %.4e (numpy %.4e), scale / ||B||^2 - 1 = %.3g" % (
        what, s.trips(), k, r2 / (TOL * nb2), rel, rel_np, scale / nb2 - 1.0))
    assert r2 <= 2.0 * TOL * nb2, (what, r2 / (TOL * nb2))
    assert abs(rel - rel_np) <= 1e-6, (what, rel, rel_np)
    assert abs(scale - nb2) <= 1e-4 * nb2 and scale <= nb2 * (1.0 + 1e-12), (what, scale, nb2)
    assert s.backend_stats() == {}  # the direct back end ran
    return r2


def make_solver(ctx, A, B, params=PARAMS, M=None, **options):
    import rails_amd

    op = rails_amd.HipOperatorWrapper(ctx, *csr(A))
    mop = rails_amd.HipOperatorWrapper(ctx, *csr(M)) if M is not None else None
    ctx.set_seed(1, 0)
    s = rails_amd.Solver(ctx, op, B, M=mop)
    assert s.set_parameters(params) == 0
    s.set_option("verbose", 0)
    if M is not None:
        s.set_option("mass", 1)
    for name, value in options.items():
        s.set_option(name, value)
    return s


_first = {}


@pytest.mark.parametrize("which", ["selection", "mixed"])
def test_solve_against_dense_numpy_and_the_oracle(ctx, oracle, which):
    import rails_amd

    A, Bs = problem(which)
    Ad, Bd = A.toarray(), Bs.toarray()
    s = make_solver(ctx, A, rails_amd.SparseRHS.from_scipy(ctx, Bs))
    code, V, T = s.solve()
    check_solution(s, code, V, T, Ad, Bd, what=which)
    ref = oracle.solve(csr(A), np.asfortranarray(Bd), oracle.params({**PARAMS, "rng_mode": 1, "seed": 1}))
    print("%s: oracle (densified B) %d trips, %d columns" % (which, ref["trips"], ref["V"].shape[1]))
    assert ref["ret"] == 0
    assert abs(s.trips() - ref["trips"]) <= max(3, ref["trips"] // 5), (s.trips(), ref["trips"])  # the allowance of test_gpu_generalized_acceptance.py
    assert D.last_launch(ctx)[0] == 2  # the last estimate ran on more than 128 basis columns: NCH = 2 of the pass kernel
    _first[which] = (V, T)
    if which == "selection":  # the dense panel on the direct back end solves the same equation
        d = make_solver(ctx, A, np.asfortranarray(Bd), subspace=0)
        dcode, Vd, Td = d.solve()
        assert dcode == 0
        Xs, Xd = V @ T @ V.T, Vd @ Td @ Vd.T
        diff = np.linalg.norm(Xs - Xd, "fro") / np.linalg.norm(Xd, "fro")
        print("selection: ||X_sparse - X_dense||_F / ||X_dense||_F = %.3g (bound %.3g)" % (diff, 50 * TOL))
        assert diff <= 50 * TOL
        d.close()
    s.close()


def test_scipy_matrix_goes_in_as_it_is_and_subspace_is_ignored(ctx):
    A, Bs = problem("selection")
    s = make_solver(ctx, A, Bs, subspace=1, projected_lanczos=1)  # anything with .tocsr(); both options accepted and ignored
    code, V, T = s.solve()
    check_solution(s, code, V, T, A.toarray(), Bs.toarray(), what="scipy B, subspace = 1")
    s.close()


def test_mass_matrix(ctx):
    from rails_amd import problems as P

    A, Bs = problem("selection")
    mrowptr, mcol, mval = P.mass_diag(M_ROWS)
    M = sp.csr_matrix((mval, mcol, mrowptr), shape=(M_ROWS, M_ROWS))
    s = make_solver(ctx, A, Bs, M=M)
    code, V, T = s.solve()
    check_solution(s, code, V, T, A.toarray(), Bs.toarray(), Md=M.toarray(), what="mass")
    s.close()


def test_warm_start(ctx):
    A, Bs = problem("selection")
    if "selection" not in _first:
        s0 = make_solver(ctx, A, Bs)
        _, V0, T0 = s0.solve()
        _first["selection"] = (V0, T0)
        s0.close()
    V0 = _first["selection"][0]
    s = make_solver(ctx, A, Bs, params={**PARAMS, "Restart from solution": 1})
    code, V, T = s.solve(V0=V0)
    check_solution(s, code, V, T, A.toarray(), Bs.toarray(), what="warm start")
    s.close()


def test_nullspace_of_one_column(ctx):
    """row and column 7 of A and row 7 of B removed (P A P, P B with P = I - e e'): A is singular with kernel e, which is handed over"""
    A, Bs = problem("selection")
    j = 7
    assert Bs[j].nnz == 1
    keep = sp.identity(M_ROWS, format="csr").tolil()
    keep[j, j] = 0.0
    keep = sp.csr_matrix(keep)
    A2, B2 = sp.csr_matrix(keep @ A @ keep), sp.csr_matrix(keep @ Bs)
    B2.eliminate_zeros()
    s = make_solver(ctx, A2, B2)
    e = np.zeros((M_ROWS, 1))
    e[j] = 1.0
    s.set_nullspace(e)
    code, V, T = s.solve()
    assert s.nullspace_rank == 1 and np.abs(V[j]).max() <= 1e-10
    check_solution(s, code, V, T, A2.toarray(), B2.toarray(), what="nullspace")
    s.close()


def test_projection_method_2_3_with_a_sparse_lu_and_refusal_of_x_2(ctx):
    import rails_amd

    A, Bs = problem("selection")
    lu = rails_amd.SparseLU(ctx, csr(A))
    s = make_solver(ctx, A, Bs, params={**PARAMS, "Projection method": 2.3})
    s.set_inverse(lu)
    code, V, T = s.solve()
    check_solution(s, code, V, T, A.toarray(), Bs.toarray(), what="projection method 2.3")
    for method in (1.2, 2.2):  # they start from B, which is an operator
        assert s.set_parameters({**PARAMS, "Projection method": method}) == 0
        code, _, _ = s.solve()
        assert code == -2, (method, code)
    s.close()
    lu.close()


def test_two_ranks_are_refused():
    import rails_amd

    A, Bs = problem("selection")
    two = rails_amd.Context(device=0, seed=1)
    try:
        two.set_partition(0, 2, 0, 2 * M_ROWS)
        op = rails_amd.HipOperatorWrapper(two, *csr(A))
        with pytest.raises(rails_amd.RailsError, match=r"code -1\).*single GPU only"):
            rails_amd.Solver(two, op, Bs)
    finally:
        two.close()


def test_driver_sparse_B(tmp_path):
    from rails_amd import mmio

    A, Bs = problem("selection")
    mmio.write_csr(str(tmp_path / "A.mtx"), M_ROWS, M_ROWS, *csr(A))
    mmio.write_csr(str(tmp_path / "B.mtx"), M_ROWS, 40, *csr(Bs))  # a coordinate file
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    args = [sys.executable, "-m", "rails_amd.main", "--dir", str(tmp_path), "--sparse-B"] + [x for k, v in PARAMS.items() for x in ("--set", "%s=%r" % (k, v))]
    p = subprocess.run(args, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(p.stdout[-1500:])
    assert p.returncode == 0, p.stdout[-3000:]
    V, T = mmio.read_dense(str(tmp_path / "V.mtx")), mmio.read_dense(str(tmp_path / "T.mtx"))
    Ad, Bd = A.toarray(), Bs.toarray()
    R = residual(Ad, Bd, V, T)
    nb2 = float(np.linalg.norm(Bd, 2) ** 2)
    assert np.linalg.norm(R, 2) <= 2.0 * TOL * nb2
    rel_np = float(np.linalg.norm(R, "fro") / np.linalg.norm(Bd.T @ Bd, "fro"))
    (line,) = [ln for ln in p.stdout.splitlines() if "relative residual" in ln and ln.startswith("solve returned")]
    printed = float(line.rsplit("relative residual", 1)[1])
    assert abs(printed - rel_np) <= 1e-6 + 5e-4 * rel_np, (printed, rel_np)  # printed with four significant digits
