"""python -m rails_amd.main --block-size 3 --inverse cg --inverse-block-amg on a small written .mtx: the inverse of "Projection method"
2.2 iterates on the block-CSR operator with the block multigrid cycle, the driver prints b, the levels and the cycles, the solution agrees
with the run whose inverse is the sparse LU, the inverse needs fewer inner iterations than with block Jacobi; and each of the flag's
refusals."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env):
    p = subprocess.run(args, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(p.stdout[-2500:])
    return p


@pytest.mark.gpu
def test_driver_inverse_block_amg(tmp_path):
    from rails_amd import mmio
    from rails_amd import problems as P

    nx, ny, nz, b = 7, 7, 6, 3  # 882 rows: two matrices at the default "amg_coarse"
    _, (rowptr, col, val) = P.block_diffusion7(nx, ny, nz, b, 100.0, 0.01, seed=1)
    m = rowptr.size - 1
    mmio.write_csr(str(tmp_path / "A.mtx"), m, m, rowptr, col.astype(np.int64), val)
    mmio.write_array(str(tmp_path / "B.mtx"), P.rhs(m, 3, seed=1))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    tol = 1e-6
    base = [sys.executable, "-m", "rails_amd.main", "--dir", str(tmp_path), "--no-mass", "--set", "Tolerance=%r" % tol, "--set", "Expand size=3",
            "--set", "Lanczos iterations=5", "--set", "Projection method=2.2"]
    flag = ["--block-size", "3", "--inverse", "cg", "--inverse-block-amg"]
    X = []
    for extra in (["--block-size", "3"], flag + ["--V", "Vb.mtx", "--T", "Tb.mtx"]):
        p = _run(base + extra, env)
        assert p.returncode == 0, p.stdout[-3000:]
        V, T = mmio.read_dense(str(tmp_path / ("Vb.mtx" if "--V" in extra else "V.mtx"))), mmio.read_dense(str(tmp_path / ("Tb.mtx" if "--T" in extra else "T.mtx")))
        X.append(V @ T @ V.T)
    assert np.linalg.norm(X[1] - X[0]) <= 10 * tol * np.linalg.norm(X[0])
    found = re.search(r"its preconditioner: a block multigrid V-cycle on the block-CSR operator, b = 3, (\d+) levels of 882 / (\d+)", p.stdout)
    assert found and int(found.group(1)) >= 2 and int(found.group(2)) % 3 == 0, p.stdout[-1500:]
    assert "A^-1 is an iterative solve on the device, method cg, block multigrid" in p.stdout and "0 flagged columns" in p.stdout
    assert re.search(r"its last solve: \d+ inner iterations at most, [1-9]\d* block multigrid cycles", p.stdout)
    # the same inverse with block Jacobi needs more inner iterations
    q = _run(base + ["--block-size", "3", "--inverse", "cg", "--inverse-block-jacobi"], env)
    assert q.returncode == 0
    inner = lambda out: int(re.search(r"(\d+) inner iterations in all", out).group(1))
    solves = lambda out: int(re.search(r"(\d+) solves of", out).group(1))
    assert inner(q.stdout) / solves(q.stdout) > inner(p.stdout) / solves(p.stdout), (inner(q.stdout), solves(q.stdout), inner(p.stdout), solves(p.stdout))
    # without a projection method above 1 there is no inverse: the flag is accepted and the driver says that it does nothing
    r = _run([a for a in base if a != "Projection method=2.2"][:-1] + flag, env)
    assert "Traceback" not in r.stdout and "--inverse-block-amg has no effect: 'Projection method' 1 applies no inverse" in r.stdout
    # refusals
    for extra, message in (
            (["--inverse", "cg", "--inverse-block-amg"], "--inverse-block-amg needs --block-size b"),
            (flag + ["--inverse-poly", "2"], "--inverse-block-amg together with --inverse-poly 2: one preconditioner at a time"),
            (flag + ["--inverse-amg"], "one preconditioner at a time"),
            (flag + ["--inverse-block-jacobi"], "one preconditioner at a time"),
            (["--block-size", "3", "--inverse-block-amg"], "the inverse chosen is a sparse LU"),
            (["--block-size", "3", "--inverse", "lu", "--inverse-block-amg"], "the inverse chosen is a sparse LU"),
            (["--block-size", "3", "--inverse", "bicgstab", "--inverse-block-amg"], "the inverse chosen is bicgstab")):
        r = _run(base + extra, env)
        assert r.returncode != 0 and message in r.stdout, (extra, r.stdout[-1500:])
    r = subprocess.run(base + flag, env=dict(env, WORLD_SIZE="2", RANK="0"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode != 0 and "single GPU" in r.stdout
