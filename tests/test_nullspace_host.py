"""Nullspace deflation of the solver template (Solver::set_nullspace, the reference's opts.nullspace, matlab/RAILSsolver.m:33-34,
221-222,311-313,527-529,538-616) on the plain CPU backend (tests/cpu_backend, test scaffolding), which has no orthogonalize(N) member and
so runs the template's generic path: a singular A with a known kernel, the refusals, and what happens without the option."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    import rails_amd

    rails_amd.load()
    out = tmp_path_factory.mktemp("cpu_nullspace") / "nullspace_cpu_driver"
    cmd = ["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "rails_amd", "include"),
           "-I" + os.path.join(ROOT, "tests", "cpu_backend"), os.path.join(ROOT, "tests", "cpu_backend", "nullspace_cpu_driver.cpp"),
           "-o", str(out), "-L" + os.path.join(ROOT, "rails_amd", "lib"), "-lrails_hip", "-L/opt/rocm/lib",
           "-Wl,-rpath," + os.path.join(ROOT, "rails_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return str(out)


def neumann2(k):
    """the 2D Laplacian of a k x k grid with Neumann boundaries (negative semidefinite; its kernel is the constants)"""
    T = 2 * np.eye(k) - np.eye(k, k=1) - np.eye(k, k=-1)
    T[0, 0] = T[-1, -1] = 1.0
    return -(np.kron(np.eye(k), T) + np.kron(T, np.eye(k)))


def run(driver, tmp_path, A, B, N, params, max_trips=0, nrows=None):
    n, p = B.shape
    q = 0 if N is None else N.shape[1]
    for name, M in (("A", A), ("B", B), ("N", N if N is not None else np.zeros((1, 1)))):
        np.asfortranarray(M).T.copy().tofile(tmp_path / (name + ".bin"))
    args = [driver, str(tmp_path / "A.bin"), str(tmp_path / "B.bin"), str(tmp_path / "N.bin"), str(n), str(p), str(q), "5", str(tmp_path / "out")]
    args += ["%s=%r" % (k, float(v)) for k, v in params.items()]
    args += ["max_trips=%d" % max_trips, "nrows=%d" % (N.shape[0] if N is not None else n)]
    subprocess.check_call(args, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    rc, trips, k, rank = (int(x) for x in open(str(tmp_path / "out.txt")).read().split()[:4])
    V = np.fromfile(str(tmp_path / "out.V")).reshape(k, n).T
    T = np.fromfile(str(tmp_path / "out.T")).reshape(k, k).T if os.path.exists(str(tmp_path / "out.T")) else None
    return rc, trips, V, T, rank


PARAMS = {"Expand size": 3, "Lanczos iterations": 10, "Tolerance": 1e-6}


@pytest.fixture(scope="module")
def problem():
    A = neumann2(24)
    B = np.random.default_rng(3).uniform(-1, 1, (A.shape[0], 2))
    B -= B.mean(axis=0)  # B in the complement of the kernel
    return A, B


def true_residual(A, B, V, T):
    X = V @ T @ V.T
    return np.linalg.norm(A @ X + X @ A.T + B @ B.T, 2) / np.linalg.norm(B, 2) ** 2


def test_nullspace_deflation_converges_orthogonal_to_the_kernel(driver, tmp_path, problem):
    A, B = problem
    N = np.ones((A.shape[0], 1))  # not normalised: the solver orthonormalises it
    rc, trips, V, T, rank = run(driver, tmp_path, A, B, N, PARAMS)
    u = N / np.linalg.norm(N)
    assert rc == 0 and rank == 1, (rc, rank)
    assert np.abs(u.T @ V).max() <= 1e-12
    assert np.abs(V.T @ V - np.eye(V.shape[1])).max() < 1e-10
    assert true_residual(A, B, V, T) < PARAMS["Tolerance"], (true_residual(A, B, V, T), trips)


def test_without_the_nullspace_the_kernel_stays_in_v(driver, tmp_path, problem):
    """Without the option the random start vector has a part of about 1/sqrt(n) along the constants, and nothing removes it.  (Run to
    the end, this solve still converges here -- 76 trips against 73 with the nullspace, true residual 9e-7 -- but its V keeps a column
    that is the constant vector to 1e-3: a direction the solution does not need.  Only the part along N is asserted.)"""
    A, B = problem
    rc, trips, V, T, rank = run(driver, tmp_path, A, B, None, PARAMS, max_trips=30)
    u = np.ones((A.shape[0], 1)) / np.sqrt(A.shape[0])
    assert rank == 0
    assert np.abs(u.T @ V).max() > 1e-6


def test_dependent_columns_are_dropped(driver, tmp_path, problem):
    A, B = problem
    n = A.shape[0]
    one = np.ones((n, 1))
    x = np.linspace(-1, 1, n)[:, None]
    N = np.hstack([one, 2 * one, x, one - 3 * x])  # rank 2
    rc, _, V, _, rank = run(driver, tmp_path, A, B, N, PARAMS, max_trips=3)
    Q = np.linalg.qr(np.hstack([one, x]))[0]
    assert rank == 2 and rc in (0, -1, 1, 2)
    assert np.abs(Q.T @ V).max() <= 1e-12


def test_refusals_leave_v_untouched(driver, tmp_path, problem):
    A, B = problem
    n = A.shape[0]
    cases = {
        "wrong row count": np.ones((n - 1, 1)),
        "no independent column": np.zeros((n, 2)),
        "rank reaches the dimension": np.random.default_rng(1).standard_normal((n, n)),
    }
    for what, N in cases.items():
        rc, trips, V, T, rank = run(driver, tmp_path, A, B, N, PARAMS)
        assert rc == -2 and trips == 0 and rank == 0, (what, rc, trips, rank)
        assert V.shape == (n, 1) and not V.any() and T is None, what
