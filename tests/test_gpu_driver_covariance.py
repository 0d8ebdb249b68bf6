"""The driver's --pairs / --pairs-out and --maps / --correlation / --maps-out options (python -m rails_amd.main) on a small Laplacian: the
files it writes are what Solution.covariance and Solution.maps give for the V and T it wrote, the indices being 1-based as in
MatrixMarket; the options go together with --variance, a bad index file is refused before the solve, and on a descriptor system the
indices (--correlation included) refer to the lifted solution in the original row order."""
import os
import subprocess
import sys

import numpy as np
import pytest

import covariance_reference as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def driver(tmp_path, *extra):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "rails_amd.main", "--dir", str(tmp_path), "--set", "Tolerance=1e-8", "--set", "Expand size=3", "--quiet"] + list(extra),
                          env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)


def test_driver_writes_pairs_and_maps(tmp_path):
    import rails_amd
    from rails_amd import mmio, problems as P

    rowptr, col, val = P.laplace7(8, 8, 6)
    m = rowptr.size - 1
    mmio.write_csr(str(tmp_path / "A.mtx"), m, m, rowptr.astype(np.int64), col.astype(np.int64), val)
    mmio.write_array(str(tmp_path / "B.mtx"), P.rhs(m, 2, seed=4))
    g = np.random.default_rng(5)
    ia = np.concatenate([[1, m, 1], g.integers(1, m + 1, 60)])  # 1-based
    ib = np.concatenate([[1, m, m], g.integers(1, m + 1, 60)])
    with open(tmp_path / "pairs.txt", "w") as f:
        f.write("% i j\n")
        for a, b in zip(ia, ib):
            f.write("%d %d\n" % (a, b))
    ref = [1, 17, m]
    p = driver(tmp_path, "--pairs", "pairs.txt", "--pairs-out", "cov.mtx", "--maps", ",".join(map(str, ref)), "--maps-out", "maps.mtx", "--variance", "var.mtx")
    assert p.returncode == 0, p.stdout[-3000:]
    assert sorted(os.listdir(tmp_path)) == ["A.mtx", "B.mtx", "T.mtx", "V.mtx", "cov.mtx", "maps.mtx", "pairs.txt", "var.mtx"]
    V, T = mmio.read_dense(str(tmp_path / "V.mtx")), mmio.read_dense(str(tmp_path / "T.mtx"))
    cov, maps, var = (mmio.read_dense(str(tmp_path / f)) for f in ("cov.mtx", "maps.mtx", "var.mtx"))
    assert cov.shape == (ia.size, 1) and maps.shape == (m, 3) and var.shape == (m, 1)
    # Solution called directly on what the driver wrote (V and T went through a text file with 17 digits: the same doubles)
    ctx = rails_amd.Context(device=0, seed=1)
    sol = rails_amd.Solution(ctx, V, T)
    rows = np.array(ref, dtype=np.int32) - 1
    assert np.array_equal(cov[:, 0], sol.covariance((ia - 1).astype(np.int32), (ib - 1).astype(np.int32)))
    assert np.array_equal(maps, sol.maps(rows))
    assert np.array_equal(var[:, 0], sol.variance())
    # ... and the dense X, within the kernels' bounds
    S = sol.S()
    assert np.all(np.abs(np.asarray(cov[:, 0] - CR.pairs(V, S, ia - 1, ib - 1), dtype=np.float64)) <= CR.pairs_bound(V, S, ia - 1, ib - 1))
    assert np.all(np.abs(np.asarray(maps - CR.maps(V, S, rows), dtype=np.float64)) <= CR.maps_bound(V, S, rows))

    sol.close()
    ctx.close()

    with open(tmp_path / "bad.txt", "w") as f:
        f.write("0 1\n")
    p = driver(tmp_path, "--pairs", "bad.txt")  # refused before the solve (the other refusals: tests/test_covariance_host.py)
    assert p.returncode != 0 and "1-based" in p.stdout and "Creating solver" not in p.stdout, p.stdout[-2000:]


def test_driver_on_a_lifted_schur_solution(tmp_path):
    """a descriptor system: the indices of --pairs and --maps are those of the original row order, over both row sets"""
    import scipy.sparse as sp

    from rails_amd import mmio

    g = np.random.default_rng(0)
    n1, n2 = 30, 120
    n = n1 + n2
    mask1 = np.zeros(n, dtype=bool)
    mask1[np.sort(g.permutation(n)[:n1])] = True
    A = (0.3 * sp.random(n, n, density=0.04, random_state=np.random.RandomState(0), format="lil")).tolil()
    A.setdiag(np.where(mask1, 2.0 + g.uniform(0, 1, n), -4.0 - g.uniform(0, 1, n)))
    A = A.tocsr()
    A.sort_indices()
    B = g.uniform(-1, 1, (n, 2))
    B[mask1] = 0.0
    mmio.write_csr(str(tmp_path / "A.mtx"), n, n, A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data)
    mmio.write_array(str(tmp_path / "B.mtx"), B)
    mmio.write_csr(str(tmp_path / "M.mtx"), n, n, np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int64), np.where(mask1, 0.0, 1.0))
    i1, i2 = np.flatnonzero(mask1), np.flatnonzero(~mask1)
    ia, ib = np.concatenate([i1, i2[:n1]]), np.concatenate([i2[:n1], i1])  # across the two row sets, both orders
    np.savetxt(tmp_path / "pairs.txt", np.column_stack([ia, ib]) + 1, fmt="%d")
    ref = np.array([i1[0], i2[0], i1[-1]])
    p = driver(tmp_path, "--pairs", "pairs.txt", "--maps", ",".join(str(r + 1) for r in ref), "--correlation", "--variance", "var.mtx")
    assert p.returncode == 0, p.stdout[-3000:]
    V, T = mmio.read_dense(str(tmp_path / "V.mtx")), mmio.read_dense(str(tmp_path / "T.mtx"))
    Ad = A.toarray()
    Vf = np.zeros((n, V.shape[1]))
    Vf[i2] = V
    Vf[i1] = -np.linalg.solve(Ad[np.ix_(i1, i1)], Ad[np.ix_(i1, i2)] @ V)
    X = Vf @ T @ Vf.T
    cov, corr, var = (mmio.read_dense(str(tmp_path / f)) for f in ("pairs.mtx", "maps.mtx", "var.mtx"))  # the default output names
    assert cov.shape == (2 * n1, 1) and corr.shape == (n, 3) and var.shape == (n, 1)
    assert np.abs(cov[:, 0] - X[ia, ib]).max() <= 1e-11 * np.abs(X).max()  # the bound tests/test_gpu_solution_driver.py uses for the variance
    # --correlation (with --variance in the same run): scaled back with the written variances the maps are the dense covariances, at the
    # bound of the pairs; where a computed variance is not > 0 (X is positive semidefinite only up to rounding) the entry is 0
    v = var[:, 0]
    assert np.abs(v - np.diag(X)).max() <= 1e-11 * np.abs(X).max()
    live = (v[:, None] > 0) & (v[ref][None, :] > 0)
    assert live.mean() > 0.9 and np.all(corr[~live] == 0.0)
    back = corr * np.sqrt(np.where(live, np.outer(v, v[ref]), 0.0))
    assert np.abs(back - X[:, ref])[live].max() <= 1e-11 * np.abs(X).max()
    solid = v > 1e-8 * v.max()  # rows whose variance is more than rounding of the solve
    assert solid.mean() > 0.5 and solid[ref].any() and np.abs(corr[solid][:, solid[ref]]).max() <= 1.0 + 1e-6
    assert all(corr[r, j] == 1.0 for j, r in enumerate(ref) if v[r] > 0)
