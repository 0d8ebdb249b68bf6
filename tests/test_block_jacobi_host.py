"""The host part of the block-Jacobi preconditioner (rails_amd/csrc/block_jacobi_host.h: where the blocks come from and every refusal
that needs no device, their extraction from block-CSR and CSR arrays, their inverses in long double) and the block geometry of the passes
(rails_amd/csrc/iter_geom.h: rails_iter_pass_geom_block), checked on the CPU by a stand-alone program (tests/cpp/block_jacobi_host.cpp,
built by rails_amd/csrc/Makefile into rails_amd/lib/block_jacobi_host: no HIP, no library), once more built with the address and
undefined-behaviour sanitizers; the program's geometry against the Python restatement, its inverses against longdouble inverses within
the bound tests/block_jacobi_reference.py derives; and that module's own conditions: the generator, the case table's geometry, the two
conditions of the step bounds."""
import os
import subprocess

import numpy as np
import pytest

import block_jacobi_reference as BJ
import iter_steps_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rails_amd", "lib", "block_jacobi_host")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def exe():
    if not os.path.exists(EXE):
        import rails_amd.build

        rails_amd.build.build()
    return EXE


def run(path):
    p = subprocess.run([path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0 and "ALL PASSED" in p.stdout, p.stdout[-4000:]
    assert " 0 failed" in p.stdout


def test_the_program_on_the_host():
    run(exe())


def test_the_same_program_under_the_sanitizers(tmp_path):
    out = str(tmp_path / "block_jacobi_host_san")
    csrc = os.path.join(ROOT, "rails_amd", "csrc")
    # host code only: the program has no device part, and -fno-gpu-sanitize says so to the compiler driver as well
    cmd = [HIPCC, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=all", "-I" + csrc, "-x", "c++",
           os.path.join(ROOT, "tests", "cpp", "block_jacobi_host.cpp"), os.path.join(csrc, "block_jacobi_host.cpp"), "-o", out]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:]
    run(out)


def test_geometry_against_the_restatement():
    """every (m / b, w, b) with m / b in 1 .. 600 and a few large values, w in 1 .. 32, b in 2 .. 8: the header and the Python restatement
    agree, and the restatement's slabs are whole block rows, none empty, at most 1024, covering the rows"""
    p = subprocess.run([exe(), "geom", "600"], stdout=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0
    table = np.array([[int(v) for v in line.split()] for line in p.stdout.splitlines()], dtype=np.int64)
    assert table.shape == ((600 + 6) * 32 * 7, 6)
    bad = []
    for nb, w, b, TY, slabs, rps in table:
        g = BJ.geometry(int(nb), int(w), int(b))
        ok = g[0] == TY and g[1] == slabs and g[2] * b == rps
        ok = ok and 1 <= g[1] <= 1024 and g[3] >= 1 and (g[1] - 1) * g[2] + g[3] == nb and g[3] <= g[2]
        ok = ok and (nb < 8 * TY or g[2] >= 8 * TY)
        if not ok:
            bad.append((nb, w, b, TY, slabs, rps, g))
    assert not bad, bad[:10]
    for (nb, w, b), want in BJ.GEOMETRY.items():
        assert BJ.geometry(nb, w, b) == want, (nb, w, b, BJ.geometry(nb, w, b), want)
    used = {(c.nb, min(gw, 32), c.b) for c in BJ.CASES for _, gw in S.groups(c.w)}
    assert used <= set(BJ.GEOMETRY), used - set(BJ.GEOMETRY)
    slabs = {BJ.GEOMETRY[k][1] for k in used}
    assert {1, 2, 17} <= slabs and any(nb % BJ.GEOMETRY[(nb, w, b)][1] for nb, w, b in used)


@pytest.mark.parametrize("b", BJ.BS)
def test_host_inverse_against_longdouble(tmp_path, b):
    """blocks of condition 1, 30 and 1e3, and the diagonal blocks of block_coupled7: the library's inverse within inverse_bound of the
    longdouble inverse, componentwise; the bound itself stays small (below 1e3 eps of the largest entry: a wrong entry cannot hide)"""
    from rails_amd import problems as P

    _, csr = P.block_coupled7(3, 3, 2, b, 1e3, skew=0.4, seed=b)
    blocks = np.concatenate([BJ.conditioned_blocks(40, b, cond, seed=10 * b + k) for k, cond in enumerate((1.0, 30.0, 1e3))]
                            + [BJ.diagonal_blocks(BJ.csr_of(csr), b)])
    conds = np.linalg.cond(blocks)
    assert conds.max() >= 900 and conds.max() <= 1.2e3
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        np.array([blocks.shape[0], b], dtype=np.int64).tofile(f)
        blocks.tofile(f)
    p = subprocess.run([exe(), "invert", fin, fout], stdout=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0, p.stdout
    got = np.fromfile(fout).reshape(blocks.shape)
    X, W, V = BJ.inverse_ld(blocks)
    bound = BJ.inverse_bound(X, W, V)
    err = np.abs(got.astype(BJ.LD) - X).astype(np.float64)
    ratio = err / bound
    rel = bound.max((1, 2)) / (BJ.EPS * np.abs(X).max((1, 2)).astype(np.float64))
    print("b = %d: largest error / bound %.3f; largest bound of a block / (eps max|X|): %.1f at condition 1, %.1f overall" % (
        b, ratio.max(), rel[:40].max(), rel.max()))
    assert np.all(err <= bound), ratio.max()
    assert rel[:40].max() <= 1.0 and rel.max() <= S.CAP / BJ.EPS  # orthogonal blocks: one rounding; nowhere above the step bounds' cap
    # the reference itself: X A = I to longdouble rounding
    res = np.abs(np.einsum("kij,kjl->kil", X, blocks.astype(BJ.LD)) - np.eye(b)).max()
    assert res <= 1e5 * BJ.EPS_LD, res


def test_refused_block_is_named(tmp_path):
    blocks = BJ.conditioned_blocks(5, 3, 10.0, seed=1)
    blocks[3] = [[1.0, 2.0, 4.0], [1.0, 2.0, 4.0], [0.0, 1.0, 1.0]]  # two equal rows of small integers: every step is exact, the last pivot is 0
    fin = str(tmp_path / "in.bin")
    with open(fin, "wb") as f:
        np.array([5, 3], dtype=np.int64).tofile(f)
        blocks.tofile(f)
    p = subprocess.run([exe(), "invert", fin, str(tmp_path / "out.bin")], stdout=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 2 and "diagonal block 3 (rows 9 .. 11)" in p.stdout and "pivot 0" in p.stdout
    blocks[3] = 0.0
    with open(fin, "wb") as f:
        np.array([5, 3], dtype=np.int64).tofile(f)
        blocks.tofile(f)
    p = subprocess.run([exe(), "invert", fin, str(tmp_path / "out.bin")], stdout=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 2 and "diagonal block 3 (rows 9 .. 11)" in p.stdout and "pivot 0" in p.stdout


def test_generator():
    """block_coupled7: the layout of block_stencil7, symmetric negative definite at skew 0, the stated formula at skew 0.4"""
    import scipy.sparse as sp

    from rails_amd import problems as P

    nx, ny, nz, b, spread = 4, 3, 2, 3, 1e3
    for skew in (0.0, 0.4):
        (indptr, indices, data), csr = P.block_coupled7(nx, ny, nz, b, spread, skew=skew, seed=5)
        A = BJ.csr_of(csr)
        mb = nx * ny * nz
        assert A.shape == (mb * b, mb * b) and indptr.size == mb + 1 and data.shape == (indices.size, b, b)
        assert (sp.bsr_matrix((data, indices, indptr), shape=A.shape).tocsr() != A).nnz == 0
        g = np.random.default_rng(5)
        Q = np.linalg.qr(g.standard_normal((mb, b, b)))[0]
        lam = 10.0 ** g.uniform(0.0, np.log10(spread), (mb, b))
        K = g.uniform(-1.0, 1.0, (b, b))
        ex, ey, ez = np.ones(nx), np.ones(ny), np.ones(nz)
        T = lambda e: sp.diags([-e[:-1], 2 * e, -e[:-1]], [-1, 0, 1])
        L = sp.kron(sp.eye(nz), sp.kron(sp.eye(ny), T(ex))) + sp.kron(sp.eye(nz), sp.kron(T(ey), sp.eye(nx))) + sp.kron(T(ez), sp.eye(nx * ny))
        Cd = sp.block_diag([(Q[i] * lam[i]) @ Q[i].T for i in range(mb)])
        want = -(Cd + sp.kron(L, sp.eye(b)) + skew * sp.kron(sp.triu(L, 1) - sp.tril(L, -1), K))
        assert abs(A - want).max() <= 1e-12 * spread
        if skew == 0.0:
            assert (A != A.T).nnz == 0
            ev = np.linalg.eigvalsh(A.toarray())
            assert ev.max() < 0 and ev.min() >= -(spread + 12.0) * (1 + 1e-12)
            blocks = BJ.diagonal_blocks(A, b)
            assert np.linalg.cond(blocks).max() > 20  # the cells are stiff: the scalar diagonal says little about them


@pytest.mark.parametrize("case_id", [c.id for c in BJ.CASES if c.nb <= 120])
def test_step_bounds_hold_their_conditions(case_id):
    """iter_steps_reference's two conditions for the cases of the step test (the larger cases are checked on the GPU test's way in): no
    bound above CAP, no column converged before the last step asked for; and block Jacobi is a different computation from point Jacobi
    there (the first iterate differs by far more than the bound)"""
    c = BJ.case(case_id)
    A = c.problem()[1]
    G = BJ.reference_inverse(A, c.b)
    e = BJ.Expected(c, G)
    for k in c.steps:
        assert np.all(e.bound_x[k] <= S.CAP * e.xmax[k]) and np.all(e.bound_r[k] <= S.CAP), (case_id, k)
        if c.one_block:  # x_1 is the solution: its bound is the floor, and the residual has decayed to rounding size (not compared)
            assert np.all(e.decay[k] < S.RR_FLOOR) and np.all(e.bound_x[k] <= 4 * S.FLOOR * e.xmax[k]), (case_id, k)
        else:
            assert np.all(e.decay[k] >= S.RR_FLOOR), (case_id, k)
    if c.method == "cg" and c.nb > 1:
        point = S.cg_steps(A, c.rhs(), 1, jacobi=True)
        assert np.all(np.abs(point[0][0] - e.x[1]).max(0) > 100 * e.bound_x[1])
