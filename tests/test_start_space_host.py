"""Continuation runs of the solver template without a GPU (rails_amd/include/rails/LyapunovSolver.hpp on the plain CPU backend of
tests/cpu_backend): "Restart upon start" against numpy's prediction of what the shrink keeps, and the raw start space
(Solver::set_raw_start_space) through the contract-only orthonormalisation rails::orthogonalize_range against a longdouble
Gram-Schmidt."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compile(tmp_path_factory, name):
    import rails_amd

    rails_amd.load()
    out = tmp_path_factory.mktemp(name) / name
    cmd = ["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "rails_amd", "include"),
           "-I" + os.path.join(ROOT, "tests", "cpu_backend"), os.path.join(ROOT, "tests", "cpu_backend", name + ".cpp"),
           "-o", str(out), "-L" + os.path.join(ROOT, "rails_amd", "lib"), "-lrails_hip", "-L/opt/rocm/lib",
           "-Wl,-rpath," + os.path.join(ROOT, "rails_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return str(out)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _compile(tmp_path_factory, "solver_cpu_driver")


@pytest.fixture(scope="module")
def start_driver(tmp_path_factory):
    return _compile(tmp_path_factory, "start_space_cpu_driver")


def _dump(path, X):
    np.asfortranarray(X).T.copy().tofile(path)  # column-major on disk


def _load(path, rows, cols):
    return np.fromfile(str(path)).reshape(cols, rows).T


def run_driver(driver, tmp_path, A, B, params, seed=1, V0=None):
    n, p = B.shape
    _dump(tmp_path / "A.bin", A)
    _dump(tmp_path / "B.bin", B)
    args = [driver, str(tmp_path / "A.bin"), str(tmp_path / "B.bin"), str(n), str(p), str(seed), str(tmp_path / "out")]
    args += ["%s=%r" % (k, float(v)) for k, v in params.items()]
    if V0 is not None:
        _dump(tmp_path / "V0.bin", V0)
        args += ["V0=%s" % (tmp_path / "V0.bin"), "V0cols=%d" % V0.shape[1]]
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    lines = open(str(tmp_path / "out.txt")).read().split()
    rc, trips, k = int(lines[0]), int(lines[1]), int(lines[2])
    return rc, trips, _load(tmp_path / "out.V", n, k), _load(tmp_path / "out.T", k, k)


def run_start_solve(start_driver, tmp_path, A, B, V0, params, seed=1):
    n, p = B.shape
    for name, X in (("A", A), ("B", B), ("V0", V0)):
        _dump(tmp_path / (name + ".bin"), X)
    args = [start_driver, "solve"] + [str(tmp_path / (x + ".bin")) for x in ("A", "B", "V0")]
    args += [str(n), str(p), str(V0.shape[1]), str(seed), str(tmp_path / "out")] + ["%s=%r" % (k, float(v)) for k, v in params.items()]
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    rc, trips, k, start_rank = (int(x) for x in open(str(tmp_path / "out.txt")).read().split())
    V = _load(tmp_path / "out.V", n, k)
    T = _load(tmp_path / "out.T", k, k) if os.path.exists(str(tmp_path / "out.T")) else None
    return rc, trips, start_rank, V, T


def banded_problem(n=200, p=2, seed=3):
    """a banded stable A (five diagonals, diagonally dominant) and B = U(-1, 1)^{n x p}"""
    g = np.random.default_rng(seed)
    A = np.zeros((n, n))
    for d in (-2, -1, 1, 2):
        A += np.diag(g.uniform(-1, 1, n - abs(d)), d)
    A -= np.diag(g.uniform(2.5, 6.0, n))
    return A, g.uniform(-1, 1, (n, p))


PARAMS = {"Expand size": 2, "Lanczos iterations": 8, "Tolerance": 1e-6, "Restart tolerance": 1e-10}


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


@pytest.mark.parametrize("capped", [False, True])
def test_restart_upon_start_keeps_what_numpy_predicts(driver, tmp_path, capped):
    A, B = banded_problem()
    rc, _, V1, T1 = run_driver(driver, tmp_path, A, B, PARAMS)
    assert rc == 0
    # (a tolerance V1 does not meet: a run that has converged after its first projected solve stops there, before any shrink)
    one = {**PARAMS, "Restart from solution": 1, "Minimize solution space": 0, "Tolerance": 1e-13}
    # (a) one trip from V1: the reduced solution T0 on span(V1)
    rc, trips, Va, T0 = run_driver(driver, tmp_path, A, B, {**one, "Maximum iterations": 1}, V0=V1)
    assert trips == 1 and Va.shape[1] == V1.shape[1]
    tol, above = gap_tolerance(np.linalg.eigvalsh(T0, UPLO="U"))
    reduced = above - 2 if capped else -1
    k1, X = restart_prediction(T0, tol, reduced)
    assert k1 == (above - 2 if capped else above) and 1 < k1 < Va.shape[1]
    # (b) the same with the shrink after the first projected solve, and one more trip
    prm = {**one, "Restart upon start": 1, "Maximum iterations": 2, "Restart tolerance": tol, "Reduced size": reduced}
    rc, trips, V, T = run_driver(driver, tmp_path, A, B, prm, V0=V1)
    assert trips == 2
    assert V.shape[1] == k1
    VX = Va @ X
    assert np.abs(V - VX @ (VX.T @ V)).max() < 1e-10
    proj = V.T @ A @ V @ T + T @ V.T @ A.T @ V + V.T @ B @ B.T @ V
    assert np.abs(proj).max() <= 1e-9 * np.linalg.norm(B, 2) ** 2
    # without the parameter the same run keeps every column
    rc, trips, V, T = run_driver(driver, tmp_path, A, B, {**prm, "Restart upon start": 0}, V0=V1)
    assert V.shape[1] > k1


def test_restart_upon_start_leaves_a_cold_start_alone(driver, tmp_path):
    A, B = banded_problem()
    rc0, trips0, V0, T0 = run_driver(driver, tmp_path, A, B, PARAMS)
    rc1, trips1, V1, T1 = run_driver(driver, tmp_path, A, B, {**PARAMS, "Restart upon start": 1})
    assert (rc0, trips0) == (rc1, trips1) and np.array_equal(V0, V1) and np.array_equal(T0, T1)


# ---- the contract-only range basis against a longdouble Gram-Schmidt (the inputs of tests/test_gpu_range_basis.py at m = 400) ----------

def build(m, w, k_old, q, seed):
    r = np.random.default_rng(seed)
    P = np.linalg.qr(r.standard_normal((m, q + k_old)))[0]
    W = r.standard_normal((m, w)) * np.exp(r.uniform(-3, 3, w))
    dep = []

    def setdep(j, vec):
        if j < w:
            W[:, j] = vec
            dep.append(j)

    if w > 1:
        setdep(1, 3.0 * W[:, 0])
    if w > 4:
        setdep(4, np.zeros(m))
    if w > 20 and q:
        setdep(20, P[:, :q] @ r.standard_normal(q))
    if w > 21 and k_old:
        setdep(21, P[:, q:] @ r.standard_normal(k_old))
    if w > 130:
        setdep(130, W[:, 2] - 2 * W[:, 100] + (P @ r.standard_normal(q + k_old) if q + k_old else 0))
    if w > 260:
        setdep(260, W[:, 129] + W[:, 7])
    if w > 299:
        setdep(w - 1, W[:, w - 2] * -1e-3)
    return P, W, sorted(set(dep))


def mgs_ref(P, W, tol=1e-8):
    Q = P.astype(np.longdouble).copy()
    kept, res = [], []
    for j in range(W.shape[1]):
        v = W[:, j].astype(np.longdouble)
        n0 = np.sqrt(v @ v)
        if n0 == 0:
            res.append(0.0)
            continue
        v = v / n0
        for _ in range(2):
            v = v - Q @ (Q.T @ v)
        n1 = float(np.sqrt(v @ v))
        res.append(n1)
        if n1 < tol:
            continue
        Q = np.hstack([Q, (v / n1)[:, None]])
        kept.append(j)
    return kept, np.array(res)


@pytest.mark.parametrize("case", [(33, 7, 0), (300, 0, 0), (129, 0, 3)], ids=lambda c: "w%d-k%d-q%d" % c)
def test_contract_range_basis_matches_longdouble_gram_schmidt(start_driver, tmp_path, case):
    """the generic orthogonalize_range starts at column 0: the old columns lead the input (orthonormal, so all of them stay)"""
    w, k_old, q = case
    m = 400
    P, W, dep = build(m, w, k_old, q, 5)
    N, X = P[:, :q], np.hstack([P[:, q:], W])
    kept_ref, res = mgs_ref(N, X)
    dropped = [j for j in range(k_old + w) if j not in kept_ref]
    assert dropped == [k_old + j for j in dep]
    assert all(res[j] <= 1e-15 for j in dropped) and all(res[j] >= 0.1 for j in kept_ref)
    _dump(tmp_path / "W.bin", X)
    _dump(tmp_path / "N.bin", N if q else np.zeros((m, 1)))
    subprocess.check_call([start_driver, "orth", str(tmp_path / "W.bin"), str(tmp_path / "N.bin"), str(m), str(k_old + w), str(q),
                           str(tmp_path / "out")])
    kept, cols = (int(x) for x in open(str(tmp_path / "out.txt")).read().split())
    assert kept == cols == len(kept_ref)
    Q = _load(tmp_path / "out.V", m, kept)
    assert np.abs(Q.T @ Q - np.eye(kept)).max() < 1e-13
    if q:
        assert np.abs(N.T @ Q).max() < 1e-13
    Xp = X - N @ (N.T @ X)
    assert np.abs(Xp - Q @ (Q.T @ Xp)).max() <= 1e-10 * np.abs(X).max()
    R = Q.T @ Xp[:, kept_ref]  # in-order semantics: upper triangular with a positive diagonal pins WHICH columns were kept
    norms = np.linalg.norm(Xp[:, kept_ref], axis=0)
    assert np.all(np.diag(R) > 0) and (np.abs(np.tril(R, -1)) / norms).max() <= 1e-10


def test_raw_start_space_solve(start_driver, driver, tmp_path):
    A, B = banded_problem()
    rc, cold_trips, V1, T1 = run_driver(driver, tmp_path, A, B, PARAMS)
    assert rc == 0
    G = np.random.default_rng(8).uniform(-1, 1, (3, 3))
    S = np.hstack([V1, B, V1[:, :3] @ G])  # neither orthonormal nor independent
    rank = np.linalg.matrix_rank(S / np.linalg.norm(S, axis=0), tol=1e-8)
    assert rank == V1.shape[1] + B.shape[1]
    A2 = A + 0.01 * np.diag(np.diag(A))  # a similar problem
    rc, trips, start_rank, V, T = run_start_solve(start_driver, tmp_path, A2, B, S, {**PARAMS, "Restart from solution": 1})
    assert rc == 0 and start_rank == rank
    assert np.abs(V.T @ V - np.eye(V.shape[1])).max() < 1e-12
    X = V @ T @ V.T
    R = A2 @ X + X @ A2.T + B @ B.T
    assert np.linalg.norm(R, 2) <= 10 * PARAMS["Tolerance"] * np.linalg.norm(B, 2) ** 2
    rc, trips2, _, _ = run_driver(driver, tmp_path, A2, B, PARAMS)
    assert rc == 0 and trips <= trips2
    # without "Restart from solution" the extension does nothing: a cold start
    rc, trips3, start_rank, _, _ = run_start_solve(start_driver, tmp_path, A2, B, S, PARAMS)
    assert rc == 0 and start_rank == 1 and trips3 == trips2


def test_raw_start_space_without_a_surviving_column_is_refused(start_driver, tmp_path):
    A, B = banded_problem(n=50)
    S = np.zeros((50, 2))
    rc, trips, start_rank, V, T = run_start_solve(start_driver, tmp_path, A, B, S, {**PARAMS, "Restart from solution": 1})
    assert rc == -2 and trips == 0 and start_rank == 0
    assert V.shape == (50, 2) and np.all(V == 0.0) and T is None
