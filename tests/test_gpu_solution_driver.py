"""The driver's --eigs and --variance options (python -m rails_amd.main; the second half of the reference's driver, src/main.cpp:140-170) on
a small written-out problem, with and without a Schur reduction; without the options the driver writes exactly the files it always wrote."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def driver(tmp_path, *extra):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "rails_amd.main", "--dir", str(tmp_path), "--set", "Tolerance=1e-8", "--set", "Expand size=3", "--quiet"] + list(extra),
                          env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)


def shares(stdout):
    """the lines `eigenvalue  eigenvalue/trace` the driver prints"""
    out = []
    for line in stdout.splitlines():
        mt = re.fullmatch(r"\s*(-?[0-9.]+(?:e[-+]?\d+)?)\s+(-?[0-9.]+(?:e[-+]?\d+)?)\s*", line)
        if mt:
            out.append((float(mt.group(1)), float(mt.group(2))))
    return out


@pytest.mark.gpu
def test_driver_eigs_and_variance(tmp_path):
    from rails_amd import mmio, problems as P

    rowptr, col, val = P.laplace7(8, 8, 6)
    m = rowptr.size - 1
    mmio.write_csr(str(tmp_path / "A.mtx"), m, m, rowptr.astype(np.int64), col.astype(np.int64), val)
    mmio.write_array(str(tmp_path / "B.mtx"), P.rhs(m, 2, seed=4))
    p = driver(tmp_path)
    assert p.returncode == 0, p.stdout[-3000:]
    assert sorted(os.listdir(tmp_path)) == ["A.mtx", "B.mtx", "T.mtx", "V.mtx"]  # what it always wrote
    assert not shares(p.stdout)
    V0, T0 = mmio.read_dense(str(tmp_path / "V.mtx")), mmio.read_dense(str(tmp_path / "T.mtx"))

    p = driver(tmp_path, "--eigs", "5", "--variance", "var.mtx")
    assert p.returncode == 0, p.stdout[-3000:]
    assert sorted(os.listdir(tmp_path)) == ["A.mtx", "B.mtx", "T.mtx", "V.mtx", "eigenvalues.mtx", "eigenvectors.mtx", "var.mtx"]
    V, T = mmio.read_dense(str(tmp_path / "V.mtx")), mmio.read_dense(str(tmp_path / "T.mtx"))
    assert V.shape == V0.shape and T.shape == T0.shape
    X = V @ T @ V.T
    var, lam, Z = (mmio.read_dense(str(tmp_path / f)) for f in ("var.mtx", "eigenvalues.mtx", "eigenvectors.mtx"))
    assert var.shape == (m, 1) and lam.shape == (5, 1) and Z.shape == (m, 5)
    scale = np.abs(X).max()
    assert np.abs(var[:, 0] - np.diag(X)).max() <= 1e-12 * scale
    w = np.linalg.eigvalsh(X)
    w = w[np.argsort(-np.abs(w))][:5]
    assert np.abs(lam[:, 0] - w).max() <= 1e-11 * abs(w[0])
    assert np.linalg.norm(X @ Z - Z * lam[:, 0], axis=0).max() <= 1e-11 * abs(w[0])
    printed = shares(p.stdout)
    assert len(printed) == 5
    assert np.allclose([a for a, _ in printed], lam[:, 0], rtol=1e-5)
    assert sum(b for _, b in printed) <= 1.0
    assert np.allclose([b for _, b in printed], lam[:, 0] / np.trace(X), rtol=1e-4)


@pytest.mark.gpu
def test_driver_eigs_and_variance_after_a_schur_reduction(tmp_path):
    """a descriptor system: the files refer to the lifted solution on all unknowns, in the original row order"""
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
    p = driver(tmp_path, "--eigs", "4", "--variance", "var.mtx")
    assert p.returncode == 0, p.stdout[-3000:]
    V, T = mmio.read_dense(str(tmp_path / "V.mtx")), mmio.read_dense(str(tmp_path / "T.mtx"))
    assert V.shape[0] == n2
    Ad = A.toarray()
    i1, i2 = np.flatnonzero(mask1), np.flatnonzero(~mask1)
    Vf = np.zeros((n, V.shape[1]))
    Vf[i2] = V
    Vf[i1] = -np.linalg.solve(Ad[np.ix_(i1, i1)], Ad[np.ix_(i1, i2)] @ V)
    X = Vf @ T @ Vf.T
    var, lam, Z = (mmio.read_dense(str(tmp_path / f)) for f in ("var.mtx", "eigenvalues.mtx", "eigenvectors.mtx"))
    assert var.shape == (n, 1) and lam.shape == (4, 1) and Z.shape == (n, 4)
    assert np.abs(var[:, 0] - np.diag(X)).max() <= 1e-11 * np.abs(X).max()
    w = np.linalg.eigvalsh(X)
    w = w[np.argsort(-np.abs(w))][:4]
    assert np.abs(lam[:, 0] - w).max() <= 1e-11 * abs(w[0])
    printed = shares(p.stdout)
    assert len(printed) == 4 and sum(b for _, b in printed) <= 1.0
