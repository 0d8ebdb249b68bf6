"""The driver's --inverse-amg option (python -m rails_amd.main): a small Laplace problem in MatrixMarket files solved with "Projection
method" 2.2 and conjugate gradients preconditioned by the multigrid V-cycle as A^-1, and the combinations the driver refuses."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import generalized_problems as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def drive(tmp_path, *extra):
    from rails_amd import mmio

    A = G.laplacian2(144)
    m = A.shape[0]
    mmio.write_csr(str(tmp_path / "A.mtx"), m, m, A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data)
    mmio.write_array(str(tmp_path / "B.mtx"), np.random.default_rng(2).uniform(-1, 1, (m, 2)))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "rails_amd.main", "--dir", str(tmp_path), "--set", "Tolerance=1e-8", "--set", "Expand size=2", "--set",
                        "Projection method=2.2", "--inverse-tol", "1e-10", "--inverse-amg", *extra], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    print(p.stdout)
    return A, p


@pytest.mark.gpu
def test_driver_inverse_amg(tmp_path):
    from rails_amd import mmio

    A, p = drive(tmp_path, "--inverse", "cg")
    assert p.returncode == 0, p.stdout[-3000:]
    assert "solve returned 0" in p.stdout
    assert "A^-1 is an iterative solve on the device, method cg" in p.stdout
    found = re.search(r"a smoothed-aggregation multigrid V-cycle, (\d+) levels of ([\d /]+) rows, operator complexity ([\d.]+)", p.stdout)
    assert found, p.stdout[-3000:]
    assert int(found.group(1)) >= 1 and found.group(2).split(" / ")[0] == str(A.shape[0])
    found = re.search(r"iterative inverse \(cg\): (\d+) solves of (\d+) columns, (\d+) inner iterations in all, (\d+) flagged columns", p.stdout)
    assert found, p.stdout[-3000:]
    solves, columns, iterations, flagged = map(int, found.groups())
    assert solves >= 1 and columns >= 2 and iterations >= columns and flagged == 0
    found = re.search(r"its last solve: (\d+) inner iterations at most, (\d+) multigrid cycles, (\d+) products and (\d+) launches inside them", p.stdout)
    assert found and int(found.group(2)) > int(found.group(1)) >= 1, p.stdout[-3000:]
    V = mmio.read_dense(str(tmp_path / "V.mtx"))
    T = mmio.read_dense(str(tmp_path / "T.mtx"))
    Ad, B = A.toarray(), mmio.read_dense(str(tmp_path / "B.mtx"))
    X = V @ T @ V.T
    # the solver stops on a Lanczos estimate of ||R||_2 / ||B'B||_2 <= 1e-8; two orders of room for the estimate
    assert np.linalg.norm(Ad @ X + X @ Ad.T + B @ B.T, 2) <= 1e-6 * np.linalg.norm(B.T @ B, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("extra,message", [
    (("--inverse", "bicgstab"), "--inverse-amg: the multigrid preconditioner is for conjugate gradients, and the inverse chosen is bicgstab"),
    (("--inverse", "cg", "--inverse-poly", "4"), "--inverse-amg together with --inverse-poly 4: one preconditioner at a time"),
    (("--inverse", "lu"), "--inverse-amg: the multigrid preconditioner is for a conjugate-gradients inverse"),
])
def test_driver_refuses(tmp_path, extra, message):
    A, p = drive(tmp_path, *extra)
    assert p.returncode != 0
    assert message in p.stdout
    assert "solve returned" not in p.stdout


@pytest.mark.gpu
def test_driver_refuses_on_two_ranks(tmp_path):
    """`--inverse cg --inverse-amg` on two ranks (both on device 0, collectives through gloo, as tests/test_gpu_iter_partition_driver.py
    starts them): every rank refuses before an inverse is built or anything is solved"""
    from rails_amd import mmio

    A = G.laplacian2(144)
    m = A.shape[0]
    mmio.write_csr(str(tmp_path / "A.mtx"), m, m, A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data)
    mmio.write_array(str(tmp_path / "B.mtx"), np.random.default_rng(2).uniform(-1, 1, (m, 2)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29653",
                        "-m", "rails_amd.main", "--dir", str(tmp_path), "--no-mass", "--set", "Tolerance=1e-8", "--set", "Expand size=2", "--set",
                        "Projection method=2.2", "--inverse", "cg", "--inverse-tol", "1e-10", "--inverse-amg", "--backend", "gloo", "--one-device"],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(p.stdout[-3000:])
    assert p.returncode != 0
    assert "--inverse-amg on 2 ranks: the multigrid preconditioner is single GPU" in p.stdout
    assert "A^-1 is" not in p.stdout and "Performing solve" not in p.stdout and "solve returned" not in p.stdout
    assert not (tmp_path / "V.mtx").exists() and not (tmp_path / "T.mtx").exists()
