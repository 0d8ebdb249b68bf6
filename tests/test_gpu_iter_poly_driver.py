"""The driver's --inverse-poly option (python -m rails_amd.main): a small Laplace problem in MatrixMarket files solved with "Projection
method" 2.2 and polynomially preconditioned conjugate gradients on the device as A^-1, and the refusal with BiCGStab."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import generalized_problems as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def drive(tmp_path, inverse):
    from rails_amd import mmio

    A = G.laplacian2(144)
    m = A.shape[0]
    mmio.write_csr(str(tmp_path / "A.mtx"), m, m, A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data)
    mmio.write_array(str(tmp_path / "B.mtx"), np.random.default_rng(2).uniform(-1, 1, (m, 2)))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "rails_amd.main", "--dir", str(tmp_path), "--set", "Tolerance=1e-8", "--set", "Expand size=2", "--set",
                        "Projection method=2.2", "--inverse", inverse, "--inverse-tol", "1e-10", "--inverse-poly", "4"], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    print(p.stdout)
    return A, p


@pytest.mark.gpu
def test_driver_inverse_poly(tmp_path):
    from rails_amd import mmio

    A, p = drive(tmp_path, "cg")
    assert p.returncode == 0, p.stdout[-3000:]
    assert "solve returned 0" in p.stdout
    assert "A^-1 is an iterative solve on the device, method cg" in p.stdout
    assert "a Chebyshev polynomial of degree 4" in p.stdout
    found = re.search(r"iterative inverse \(cg\): (\d+) solves of (\d+) columns, (\d+) inner iterations in all, (\d+) flagged columns", p.stdout)
    assert found, p.stdout[-3000:]
    solves, columns, iterations, flagged = map(int, found.groups())
    assert solves >= 1 and columns >= 2 and iterations >= columns and flagged == 0
    V = mmio.read_dense(str(tmp_path / "V.mtx"))
    T = mmio.read_dense(str(tmp_path / "T.mtx"))
    Ad, B = A.toarray(), mmio.read_dense(str(tmp_path / "B.mtx"))
    X = V @ T @ V.T
    # the solver stops on a Lanczos estimate of ||R||_2 / ||B'B||_2 <= 1e-8; two orders of room for the estimate
    assert np.linalg.norm(Ad @ X + X @ Ad.T + B @ B.T, 2) <= 1e-6 * np.linalg.norm(B.T @ B, 2)


@pytest.mark.gpu
def test_driver_refuses_the_polynomial_with_bicgstab(tmp_path):
    A, p = drive(tmp_path, "bicgstab")
    assert p.returncode != 0
    assert "--inverse-poly 4: the polynomial preconditioner is for conjugate gradients, and the inverse chosen is bicgstab" in p.stdout
    assert "solve returned" not in p.stdout
