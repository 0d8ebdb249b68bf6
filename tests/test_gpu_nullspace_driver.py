"""The driver's --nullspace option (python -m rails_amd.main): a small pure Neumann problem in MatrixMarket files, and the refusal of a
nullspace file whose row count is not that of the equation."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def neumann2(k):
    T = 2 * np.eye(k) - np.eye(k, k=1) - np.eye(k, k=-1)
    T[0, 0] = T[-1, -1] = 1.0
    return -(np.kron(np.eye(k), T) + np.kron(T, np.eye(k)))


def driver(tmp_path, *extra):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "rails_amd.main", "--dir", str(tmp_path), "--set", "Tolerance=1e-8", "--set", "Expand size=3"] + list(extra),
                          env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)


@pytest.mark.gpu
def test_driver_nullspace(tmp_path):
    import scipy.sparse as sp

    from rails_amd import mmio

    A = sp.csr_matrix(neumann2(12))
    m = A.shape[0]
    mmio.write_csr(str(tmp_path / "A.mtx"), m, m, A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data)
    B = np.random.default_rng(2).uniform(-1, 1, (m, 2))
    B -= B.mean(axis=0)
    mmio.write_array(str(tmp_path / "B.mtx"), B)
    mmio.write_array(str(tmp_path / "N.mtx"), np.ones((m, 1)))
    for backend in ([], ["--direct"]):
        p = driver(tmp_path, "--nullspace", "N.mtx", *backend)
        assert p.returncode == 0, p.stdout[-3000:]
        assert "nullspace: 1 of 1 columns kept" in p.stdout
        V = mmio.read_dense(str(tmp_path / "V.mtx"))
        assert np.abs(V.sum(axis=0)).max() / np.sqrt(m) < 1e-10
    mmio.write_array(str(tmp_path / "N2.mtx"), np.ones((m - 1, 1)))
    p = driver(tmp_path, "--nullspace", "N2.mtx")
    assert p.returncode != 0 and "--nullspace: N has %d rows, the equation solved has %d" % (m - 1, m) in p.stdout, p.stdout[-3000:]
