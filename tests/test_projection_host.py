"""The projection methods of the solver template ("Projection method" with Solver::set_inverse, matlab/RAILSsolver.m:7-24) on the plain
CPU backend (tests/cpu_backend, test scaffolding): parameter checks, the start spaces and expansions of every method, and convergence."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = (1.1, 1.2, 1.3, 2.1, 2.2, 2.3)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    import rails_amd

    rails_amd.load()
    out = tmp_path_factory.mktemp("cpu_projection") / "projection_cpu_driver"
    cmd = ["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "rails_amd", "include"),
           "-I" + os.path.join(ROOT, "tests", "cpu_backend"), os.path.join(ROOT, "tests", "cpu_backend", "projection_cpu_driver.cpp"),
           "-o", str(out), "-L" + os.path.join(ROOT, "rails_amd", "lib"), "-lrails_hip", "-L/opt/rocm/lib",
           "-Wl,-rpath," + os.path.join(ROOT, "rails_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return str(out)


def laplace2(k):
    """the 2D Laplacian of a k x k grid (negative definite: a stable A)"""
    T = 2 * np.eye(k) - np.eye(k, k=1) - np.eye(k, k=-1)
    return -(np.kron(np.eye(k), T) + np.kron(T, np.eye(k)))


def run(driver, tmp_path, A, B, params, V0=None, inverse=True, max_trips=0):
    n, p = B.shape
    for name, M in (("A", A), ("Ainv", np.linalg.inv(A)), ("B", B)):
        np.asfortranarray(M).T.copy().tofile(tmp_path / (name + ".bin"))
    args = [driver, str(tmp_path / "A.bin"), str(tmp_path / "Ainv.bin"), str(tmp_path / "B.bin"), str(n), str(p), "5", str(tmp_path / "out")]
    args += ["%s=%r" % (k, float(v)) for k, v in params.items()]
    args += ["inverse=%d" % int(inverse), "max_trips=%d" % max_trips]
    if V0 is not None:
        np.asfortranarray(V0).T.copy().tofile(tmp_path / "V0.bin")
        args += ["V0=%s" % (tmp_path / "V0.bin"), "V0cols=%d" % V0.shape[1], "Restart from solution=1"]
    subprocess.check_call(args, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    rc, trips, k = (int(x) for x in open(str(tmp_path / "out.txt")).read().split()[:3])
    V = np.fromfile(str(tmp_path / "out.V")).reshape(k, n).T
    T = np.fromfile(str(tmp_path / "out.T")).reshape(k, k).T if os.path.exists(str(tmp_path / "out.T")) else None
    return rc, trips, V, T


def projector_residual(V, Y):
    return np.linalg.norm(Y - V @ (V.T @ Y)) / np.linalg.norm(Y)


@pytest.fixture(scope="module")
def problem():
    A = laplace2(10)
    B = np.random.default_rng(3).uniform(-1, 1, (A.shape[0], 2))
    return A, B


PARAMS = {"Expand size": 3, "Lanczos iterations": 10, "Tolerance": 1e-8}


def test_projection_method_values(driver, tmp_path, problem):
    A, B = problem
    for bad in (1.5, 3.0, 0.0, 2.0):
        assert run(driver, tmp_path, A, B, {**PARAMS, "Projection method": bad})[0] == 2, bad
    assert run(driver, tmp_path, A, B, {**PARAMS, "Projection method": 1.2}, inverse=False)[0] == -2


def test_start_spaces(driver, tmp_path, problem):
    A, B = problem
    Ai = np.linalg.inv(A)
    _, _, V, _ = run(driver, tmp_path, A, B, {**PARAMS, "Projection method": 1.2}, max_trips=1)
    assert V.shape[1] == B.shape[1] and projector_residual(V, Ai @ B) <= 1e-10
    _, _, V, _ = run(driver, tmp_path, A, B, {**PARAMS, "Projection method": 2.2}, max_trips=1)
    assert V.shape[1] == 2 * B.shape[1] and projector_residual(V, np.hstack([B, Ai @ B])) <= 1e-10
    V0 = np.linalg.qr(np.random.default_rng(4).standard_normal((A.shape[0], 2)))[0]
    _, _, V, _ = run(driver, tmp_path, A, B, {**PARAMS, "Projection method": 1.1}, V0=V0, max_trips=1)
    assert V.shape[1] == 2 and projector_residual(V, Ai @ V0) <= 1e-10
    _, _, V, _ = run(driver, tmp_path, A, B, {**PARAMS, "Projection method": 2.1}, V0=V0, max_trips=1)
    assert V.shape[1] == 4 and projector_residual(V, np.hstack([V0, Ai @ V0])) <= 1e-10
    _, _, V, _ = run(driver, tmp_path, A, B, {**PARAMS, "Projection method": 2.3}, V0=V0, max_trips=1)
    assert np.abs(V - V0).max() < 1e-12  # the driver marks V0 orthonormal by orthogonalising it once
    assert np.allclose(V.T @ V, np.eye(V.shape[1]), atol=1e-12)


@pytest.mark.parametrize("method,per", [(1.2, 1), (2.2, 2), (1.3, 1), (2.3, 2)])
def test_expansion_width(driver, tmp_path, problem, method, per):
    A, B = problem
    _, _, V1, _ = run(driver, tmp_path, A, B, {**PARAMS, "Projection method": method}, max_trips=1)
    _, _, V2, _ = run(driver, tmp_path, A, B, {**PARAMS, "Projection method": method}, max_trips=2)
    assert V2.shape[1] - V1.shape[1] == per * PARAMS["Expand size"]
    assert np.allclose(V2.T @ V2, np.eye(V2.shape[1]), atol=1e-10)


@pytest.mark.parametrize("method", (1.0,) + METHODS)
def test_every_method_converges(driver, tmp_path, problem, method):
    A, B = problem
    rc, trips, V, T = run(driver, tmp_path, A, B, {**PARAMS, "Projection method": method})
    X = V @ T @ V.T
    res = np.linalg.norm(A @ X + X @ A.T + B @ B.T) / np.linalg.norm(B @ B.T)
    assert rc == 0 and res < 1e-6 and trips < A.shape[0] - 10, (rc, res, trips)
