"""rails::Solution (rails_amd/include/rails/Solution.hpp), the object for X = U S U', on the plain CPU backend (tests/cpu_backend, test
scaffolding; it has no rowquad member, so the variance takes the template's contract path): trace, variance, products and eigenpairs
against dense algebra, for a non-orthonormal U and for a rank-deficient one.

Bounds.  eps = 2^-52.  Trace, variance and products are sums of at most m k^2 products of entries: |error| <= m k^2 eps max|U|^2 max|S|
is a (crude, certain) forward bound; it is 2e-9 relative to nothing here, the checks use it as it stands.  The eigenpairs go through an
orthonormalisation of U (two rounds of Gram-Schmidt: orthonormal to a few eps whatever the condition of U), a k x k symmetric
eigensolve (backward stable) and two products with Q: residual and orthonormality are bounded by c k eps |X|_2 with a modest c; tol_e =
1e-11 |X|_2 (1e-11 for Z'Z - I), the bound this project uses for device orthogonalisation against the oracle (tests/test_gpu_kernels.py),
leaves c k <= 4.5e4."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    import rails_amd

    rails_amd.load()
    out = tmp_path_factory.mktemp("cpu_solution") / "solution_cpu_driver"
    cmd = ["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "rails_amd", "include"),
           "-I" + os.path.join(ROOT, "tests", "cpu_backend"), os.path.join(ROOT, "tests", "cpu_backend", "solution_cpu_driver.cpp"),
           "-o", str(out), "-L" + os.path.join(ROOT, "rails_amd", "lib"), "-lrails_hip", "-L/opt/rocm/lib",
           "-Wl,-rpath," + os.path.join(ROOT, "rails_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return str(out)


def run(driver, tmp_path, U, S, W, want, tol):
    m, k = U.shape
    for name, M in (("U", U), ("S", S), ("W", W)):
        np.ascontiguousarray(M, dtype=np.float64).tofile(tmp_path / (name + ".bin"))
    subprocess.check_call([driver, str(tmp_path / "U.bin"), str(tmp_path / "S.bin"), str(tmp_path / "W.bin"), str(m), str(k), str(W.shape[1]), str(want),
                           repr(float(tol)), str(tmp_path / "out")])
    rank, found, trace = open(str(tmp_path / "out.txt")).read().split()
    rank, found = int(rank), int(found)
    get = lambda ext, shape: np.fromfile(str(tmp_path / ("out." + ext))).reshape(shape)
    return dict(rank=rank, found=found, trace=float(trace), var=get("var", (m,)), apply=get("apply", (m, W.shape[1])), values=get("values", (found,)),
                vectors=get("vectors", (m, found)))


def problem(deficient):
    g = np.random.default_rng(20)
    m, k = 200, 12
    U = g.standard_normal((m, k)) @ (np.eye(k) + 0.5 * g.standard_normal((k, k)))  # not orthonormal
    if deficient:
        U[:, 7] = U[:, 3]  # two equal columns
    S = g.standard_normal((k, k))
    S = S + S.T  # symmetric indefinite
    W = g.standard_normal((m, 3))
    return U, S, W


def check_eigs(X, out, want_values):
    nX = np.linalg.norm(X, 2)
    lam, Z = out["values"], out["vectors"]
    assert np.all(np.abs(lam[:-1]) >= np.abs(lam[1:]))
    assert np.abs(lam - want_values).max() <= 1e-11 * nX, np.abs(lam - want_values).max() / nX
    resid = np.linalg.norm(X @ Z - Z * lam, axis=0).max()
    orth = np.abs(Z.T @ Z - np.eye(Z.shape[1])).max()
    print("eigenvalue error %.2e, residual %.2e (relative to |X|), |Z'Z - I| %.2e" % (np.abs(lam - want_values).max() / nX, resid / nX, orth))
    assert resid <= 1e-11 * nX and orth <= 1e-11


@pytest.mark.parametrize("deficient", [False, True])
def test_solution_on_the_cpu_backend_matches_dense_algebra(driver, tmp_path, deficient):
    U, S, W = problem(deficient)
    m, k = U.shape
    X = U @ S @ U.T
    bound = m * k * k * EPS * np.abs(U).max() ** 2 * np.abs(S).max()
    out = run(driver, tmp_path, U, S, W, 0, 0.0 if not deficient else 1e-8)
    assert out["rank"] == k
    assert abs(out["trace"] - np.trace(X)) <= bound
    assert np.abs(out["var"] - np.diag(X)).max() <= bound
    assert np.abs(out["apply"] - X @ W).max() <= bound * np.abs(W).max() * m
    w = np.linalg.eigvalsh(X)
    w = w[np.argsort(-np.abs(w))]
    if not deficient:
        assert out["found"] == k
    else:  # the numerical rank, and X reproduced to the tolerance
        assert out["found"] == np.linalg.matrix_rank(U) == k - 1
        Z, lam = out["vectors"], out["values"]
        assert np.linalg.norm(Z @ np.diag(lam) @ Z.T - X, 2) <= 1e-8 * np.linalg.norm(X, 2)
    check_eigs(X, out, w[:out["found"]])


def test_leading_pairs_only(driver, tmp_path):
    U, S, W = problem(False)
    X = U @ S @ U.T
    out = run(driver, tmp_path, U, S, W, 4, 0.0)
    w = np.linalg.eigvalsh(X)
    w = w[np.argsort(-np.abs(w))]
    assert out["found"] == 4
    check_eigs(X, out, w[:4])
