"""The command-line driver on two ranks with an iterative inverse: `python -m torch.distributed.run --nproc-per-node 2 -m rails_amd.main
... --backend gloo --one-device --inverse cg --set "Projection method=2.2"` on MatrixMarket files of a small Laplacian, both ranks on
device 0 and the collectives through gloo, staged through host memory (the rehearsal tests/test_gpu_multiprocess.py makes of the
benchmark): everything of a run on two GPUs except RCCL itself.  The result is compared with the one-process run of the same command
line, without and with `--inverse-poly 4` (which must really precondition: the object's own counters and the inner iteration count say
so); `--inverse lu` on two ranks keeps its refusal, and so does the polynomial on a BiCGStab inverse."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = (12, 12, 9)  # the grid of tests/test_gpu_iter_partition_solver.py


def _driver(directory, nranks, port, inverse, poly=0):
    cmd = [sys.executable]
    if nranks > 1:
        cmd += ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nranks), "--master-addr", "127.0.0.1", "--master-port", str(port)]
    cmd += ["-m", "rails_amd.main", "--dir", str(directory), "--no-mass", "--inverse", inverse, "--inverse-tol", "1e-8", "--seed", "3",
            "--set", "Projection method=2.2", "--set", "Tolerance=1e-3", "--set", "Restart size=64", "--set", "Reduced size=32", "--set", "Expand size=4",
            "--set", "Lanczos iterations=8"]
    if poly:
        cmd += ["--inverse-poly", str(poly)]
    if nranks > 1:
        cmd += ["--backend", "gloo", "--one-device"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from rails_amd import mmio
    from rails_amd import problems as P

    d = tmp_path_factory.mktemp("driver")
    rowptr, col, val = P.laplace7(*GRID)
    m = rowptr.size - 1
    mmio.write_csr(str(d / "A.mtx"), m, m, rowptr, col, val)
    mmio.write_array(str(d / "B.mtx"), P.rhs(m, 4, seed=5))
    return d


def _run(files, nranks, port, poly=0):
    """one driver run with a conjugate-gradients inverse: (X = V T V' from the files it wrote, inner iterations, stdout)"""
    from rails_amd import mmio

    p = _driver(files, nranks, port, "cg", poly)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    assert "A^-1 is an iterative solve on the device, method cg" in p.stdout, p.stdout[-2000:]
    found = re.search(r"(\d+) inner iterations in all, (\d+) flagged columns", p.stdout)
    assert found and int(found.group(2)) == 0, p.stdout[-2000:]
    V, T = mmio.read_dense(str(files / "V.mtx")), mmio.read_dense(str(files / "T.mtx"))
    return V @ T @ V.T, int(found.group(1)), p.stdout


@pytest.fixture(scope="module")
def plain_runs(files):
    """the one-process and the two-process run without the polynomial"""
    return {nranks: _run(files, nranks, 29641) for nranks in (1, 2)}


def test_two_rank_driver_run_with_an_iterative_inverse(plain_runs):
    X1, it1, _ = plain_runs[1]
    X2, it2, out2 = plain_runs[2]
    assert np.linalg.norm(X2 - X1) / np.linalg.norm(X1) <= 1e-2
    assert "a Chebyshev polynomial" not in out2 and it2 > 0


def test_inverse_poly_works_on_two_ranks(files, plain_runs):
    """--inverse-poly 4 on two ranks: the object itself reports applications of the polynomial and launches of the fused step (its
    ghost-row form: every rank's block has ghost rows), the inner iterations drop to well under half of those without it (at solver
    level 779 to 197, tests/test_gpu_iter_partition_solver.py), and X is the one-process X of the same command line"""
    X1, _, out1 = _run(files, 1, 29645, poly=4)
    X2, inner, out2 = _run(files, 2, 29645, poly=4)
    for out in (out1, out2):
        assert "its preconditioner: a Chebyshev polynomial of degree 4" in out, out[-2000:]
        found = re.search(r"its last solve: (\d+) applications of the polynomial, (\d+) products with A, (\d+) of them in fused steps", out)
        assert found, out[-2000:]
        applications, products, fused = (int(g) for g in found.groups())
        assert applications > 0 and fused == 4 * applications and products > fused
    assert 0 < inner < 0.5 * plain_runs[2][1], (inner, plain_runs[2][1])
    assert np.linalg.norm(X2 - X1) / np.linalg.norm(X1) <= 1e-2
    assert np.linalg.norm(X2 - plain_runs[2][0]) / np.linalg.norm(X1) <= 1e-2


def test_inverse_poly_on_a_bicgstab_inverse_is_refused_on_two_ranks(files):
    p = _driver(files, 2, 29647, "bicgstab", poly=4)
    assert p.returncode != 0
    assert "--inverse-poly 4: the polynomial preconditioner is for conjugate gradients, and the inverse chosen is bicgstab" in p.stderr, p.stderr[-3000:]
    assert "solve returned" not in p.stdout


def test_lu_on_two_ranks_points_at_the_iterative_inverse(files):
    p = _driver(files, 2, 29643, "lu")
    assert p.returncode != 0
    assert "--inverse iterative" in p.stderr and "sparse LU inverse runs on one rank" in p.stderr, p.stderr[-3000:]
