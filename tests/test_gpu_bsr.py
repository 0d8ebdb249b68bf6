"""Block-CSR operators (include/rails_hip.h: rails_csr_create_bsr, rails_amd/csrc/spmm_bsr.hip, bsr_choice.h) on the GPU.

The reference everywhere is the expanded CSR matrix -- every entry of every block, zeros included, in stored order -- on a handle forced to
the row-gather kernel (set_variant(3)), and the comparison is np.array_equal on the bits: the block-CSR product makes the same fused
multiply-adds in the same order.  Only the magnitude test uses a bound, the one tests/test_gpu_kernels.py has for the row kernels
(1e-14 * sqrt(entries per row) * 4, there on the largest entry, here also on the Frobenius norms).

Every shape here is small enough for one round of block rows per lane group (rpg == 1, asserted below where it matters).  The launches with
2 and 4 rounds need thousands of block rows; tests/test_gpu_bsr_rounds.py has them, against an int64 host product instead of a kernel."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "rails_amd", "lib")
WIDTHS = (1, 2, 3, 15, 16, 17, 32, 33, 64, 128, 130)


@pytest.fixture(scope="module")
def ctx():
    import rails_amd

    c = rails_amd.Context(device=0, seed=1234)
    yield c
    c.close()


def random_bsr(mb, b, counts, seed):
    """block rows of counts[i] blocks at random ascending block columns, entries U(-1, 1)"""
    g = np.random.default_rng(seed)
    counts = np.minimum(np.asarray(counts, dtype=np.int64), mb)
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    indices = np.concatenate([np.sort(g.choice(mb, int(n), replace=False)) for n in counts] + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    return indptr, indices, g.uniform(-1.0, 1.0, (indices.size, b, b))


def expand(indptr, indices, data):
    """the CSR matrix of every stored entry, zeros included, in stored order: scalar row i * b + r holds row r of each block of block row i"""
    b = data.shape[1]
    counts = np.diff(indptr)
    rowptr = np.concatenate([[0], np.cumsum(np.repeat(counts, b) * b)]).astype(np.int64)
    # block q contributes to its b scalar rows; the rows of block row i list its blocks in order
    order = np.concatenate([np.tile(np.arange(indptr[i], indptr[i + 1]), b) for i in range(counts.size)] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    r = np.concatenate([np.repeat(np.arange(b), counts[i]) for i in range(counts.size)] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    col = (indices[order].astype(np.int64)[:, None] * b + np.arange(b)[None, :]).ravel().astype(np.int32)
    val = data[order, r, :].ravel()
    return rowptr, col, val


def window(mv, off, nc):
    return mv.view(off, off + nc - 1) if nc > 1 else mv.view(off)


def product(ctx, op, Xh, xoff=0, yoff=0, xtail=0, ytail=0):
    """op * Xh between windows of panels that hold NaN everywhere else; returns the window of Y and checks that nothing else was written"""
    import rails_amd

    m, nc = Xh.shape
    big = rails_amd.HipMultiVectorWrapper(ctx, m=m, n=xoff + nc + xtail, capacity=xoff + nc + xtail)
    big.from_host(np.full((m, xoff + nc + xtail), np.nan))
    window(big, xoff, nc).from_host(Xh)
    out = rails_amd.HipMultiVectorWrapper(ctx, m=m, n=yoff + nc + ytail, capacity=yoff + nc + ytail)
    out.from_host(np.full((m, yoff + nc + ytail), np.nan))
    op.apply(window(big, xoff, nc), window(out, yoff, nc))
    Y = out.to_host()
    assert np.all(np.isnan(Y[:, :yoff])) and np.all(np.isnan(Y[:, yoff + nc:])), "written outside the window of Y"
    return Y[:, yoff:yoff + nc]


class Pair:
    """a block-CSR handle and the row-gather handle of its expanded matrix"""

    def __init__(self, ctx, arrays):
        import rails_amd

        self.ctx, self.arrays = ctx, arrays
        self.b = arrays[2].shape[1]
        self.m = (arrays[0].size - 1) * self.b
        self.bsr = rails_amd.HipOperatorWrapper.from_bsr(ctx, *arrays)
        self.csr_arrays = expand(*arrays)
        self.csr = rails_amd.HipOperatorWrapper(ctx, *self.csr_arrays)
        self.csr.set_variant(3)

    def check(self, nc, seed=0, trans=False, **where):
        Xh = np.random.default_rng(seed).uniform(-1.0, 1.0, (self.m, nc))
        a, r = (self.bsr.transpose(), self.csr.transpose()) if trans else (self.bsr, self.csr)
        got = product(self.ctx, a, Xh, **where)
        assert a.last_kernel().startswith("k_spmm_bsr")
        want = product(self.ctx, r, Xh)
        assert r.last_kernel() == "k_spmm_rowgather"
        assert np.array_equal(got, want), "b %d, %d columns, %s: %d entries differ" % (self.b, nc, where, int((got != want).sum()))
        return got


def table():
    exe = os.path.join(LIBDIR, "bsr_host")
    if not os.path.exists(exe):
        import rails_amd.build

        rails_amd.build.build()
    p = subprocess.run([exe, "--table"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:]
    return [json.loads(line) for line in p.stdout.splitlines()]


def test_every_instantiation_at_its_smallest_shape_and_one_block_row_past_a_workgroup(ctx):
    rows = table()
    assert len(rows) == 21
    for r in rows:
        b, lpr = r["inst"]
        for mb in (r["mb"], 3 * r["rows"] + 1):
            pair = Pair(ctx, random_bsr(mb, b, np.random.default_rng(mb).integers(1, 4, mb), seed=10 * b + lpr))
            pair.check(r["nc"], seed=mb)
            st = pair.bsr.bsr_stats()
            assert (st["B"], st["LPR"], st["threads"], st["rpg"]) == (b, lpr, r["threads"], 1), (r, st)
            workgroups = -(-mb // r["rows"])
            assert st["grid"] == 8 * -(-workgroups // 8) and st["all_staged"]


@pytest.mark.parametrize("b", range(2, 9))
def test_widths(ctx, b):
    mb = 301  # a few thousand rows at b = 8, more than one workgroup at every width
    pair = Pair(ctx, random_bsr(mb, b, np.random.default_rng(b).integers(0, 9, mb), seed=b))
    for nc in WIDTHS:
        pair.check(nc, seed=nc)
        assert pair.bsr.bsr_stats()["LPR"] == (8 if nc <= 16 else 16 if nc <= 32 else 32)
    assert pair.bsr.block_size == b and pair.csr.block_size == 1
    assert pair.bsr.M() == mb * b and pair.bsr.nnz() == pair.arrays[1].size * b * b
    st = pair.bsr.bsr_stats()
    assert st["nnzb"] == pair.arrays[1].size and st["b"] == b and st["max_block_row"] == int(np.diff(pair.arrays[0]).max())
    assert st["device_bytes"] == st["nnzb"] * (b * b * 8 + 4) + (mb + 1) * 8  # no transposed copy yet


@pytest.mark.parametrize("b", [3, 4, 7])
def test_windows_on_even_and_odd_columns_in_poisoned_panels(ctx, b):
    pair = Pair(ctx, random_bsr(130, b, np.random.default_rng(1).integers(1, 8, 130), seed=40 + b))
    for nc in (1, 5, 16, 33):
        for xoff, yoff in ((0, 0), (1, 0), (0, 1), (1, 1), (2, 3), (3, 2)):
            # tails of no columns: both windows end at the last column of their panels
            pair.check(nc, seed=nc + xoff, xoff=xoff, yoff=yoff)
            pair.check(nc, seed=nc + yoff, xoff=xoff, yoff=yoff, xtail=3, ytail=2)


def test_one_block_row(ctx):
    for b in (2, 5, 8):
        pair = Pair(ctx, (np.array([0, 1], dtype=np.int64), np.array([0], dtype=np.int32), np.random.default_rng(b).uniform(-1, 1, (1, b, b))))
        for nc in (1, 4, 17, 70):
            pair.check(nc)


def test_empty_block_rows_at_the_ends_of_a_workgroups_range(ctx):
    b, mb = 4, 200
    counts = np.random.default_rng(3).integers(1, 8, mb)
    rows_per_wg = 256 // 8  # k_spmm_bsr<4, 8> at 16 columns: 32 lane groups, one round
    for i in (0, rows_per_wg - 1, rows_per_wg, 2 * rows_per_wg - 1, 77, 78, mb - 1):
        counts[i] = 0
    counts[3 * rows_per_wg:4 * rows_per_wg] = 0  # a workgroup without any block
    pair = Pair(ctx, random_bsr(mb, b, counts, seed=9))
    for nc in (16, 7, 40):
        got = pair.check(nc)
        assert np.all(got[(counts == 0).repeat(b)] == 0.0) and not np.any(np.signbit(got[(counts == 0).repeat(b)]))
    assert pair.bsr.bsr_stats()["rpg"] == 1


def test_a_block_row_longer_than_the_lds_buffer_beside_short_ones(ctx):
    """b = 8: the buffer holds 64 blocks; a block row of 70 sends its workgroup to the unstaged form.  The short rows of that workgroup
    come out with the bits the staged form gives them (the same matrix with the long row cut to one block)."""
    b, mb, long_row = 8, 90, 5
    counts = np.random.default_rng(4).integers(0, 4, mb)
    counts[long_row] = 70
    arrays = random_bsr(mb, b, counts, seed=12)
    pair = Pair(ctx, arrays)
    indptr, indices, data = arrays
    keep = np.ones(indices.size, dtype=bool)
    keep[indptr[long_row] + 1:indptr[long_row + 1]] = False
    cut_counts = counts.copy()
    cut_counts[long_row] = 1
    cut = Pair(ctx, (np.concatenate([[0], np.cumsum(cut_counts)]).astype(np.int64), indices[keep], data[keep]))
    other = np.ones(mb * b, dtype=bool)
    other[long_row * b:(long_row + 1) * b] = False
    for nc in (16, 3, 33):
        got = pair.check(nc, seed=nc)
        assert not pair.bsr.bsr_stats()["all_staged"]
        short = cut.check(nc, seed=nc)
        assert cut.bsr.bsr_stats()["all_staged"]
        assert np.array_equal(got[other], short[other])


def test_a_block_of_zeros(ctx):
    for b in (2, 6):
        arrays = random_bsr(40, b, np.full(40, 3), seed=b)
        arrays[2][::4] = 0.0
        pair = Pair(ctx, arrays)
        pair.check(16)
        pair.check(5)


@pytest.mark.parametrize("b", [2, 5, 8])
def test_transposed_product(ctx, b):
    pair = Pair(ctx, random_bsr(150, b, np.random.default_rng(b).integers(0, 7, 150), seed=70 + b))
    before = pair.bsr.bsr_stats()["device_bytes"]
    for nc in (1, 16, 33, 130):
        pair.check(nc, seed=nc, trans=True, xoff=1, yoff=1)
        assert pair.bsr.last_kernel() == "k_spmm_bsr (transposed copy)"
    assert pair.bsr.bsr_stats()["device_bytes"] == 2 * before
    pair.check(16)
    assert pair.bsr.last_kernel() == "k_spmm_bsr"


def test_magnitude_against_longdouble(ctx):
    """the bound of tests/test_gpu_kernels.py for the row kernels: 1e-14 * sqrt(entries per row) * 4"""
    for b, nc in ((3, 16), (6, 32), (8, 130)):
        arrays = random_bsr(120, b, np.random.default_rng(b).integers(1, 9, 120), seed=b)
        pair = Pair(ctx, arrays)
        Xh = np.random.default_rng(1).uniform(-1.0, 1.0, (pair.m, nc))
        got = product(ctx, pair.bsr, Xh)
        rowptr, col, val = pair.csr_arrays
        ref = np.zeros((pair.m, nc), dtype=np.longdouble)
        np.add.at(ref, np.repeat(np.arange(pair.m), np.diff(rowptr)), val.astype(np.longdouble)[:, None] * Xh.astype(np.longdouble)[col])
        nnz_row = max(1, val.size // pair.m)
        err = got.astype(np.longdouble) - ref
        print("b %d, %d columns: relative Frobenius error %.3e, largest error %.3e" % (b, nc, float(np.linalg.norm(err) / np.linalg.norm(ref)), float(np.abs(err).max())))
        assert np.linalg.norm(err) <= 1e-14 * np.sqrt(nnz_row) * 4 * np.linalg.norm(ref)
        assert np.abs(err).max() <= 1e-14 * np.sqrt(nnz_row) * 4 * np.abs(ref).max()


@pytest.mark.parametrize("b", [2, 3, 6])
def test_conversion_of_a_csr_matrix_keeps_the_bits(ctx, b):
    """zero fill adds nothing to a finite sum: the converted operator's product is the row-gather product of the original CSR matrix"""
    import scipy.sparse as sp

    import rails_amd

    m = 150 * b
    A = sp.random(m, m, density=4.0 / m, random_state=np.random.RandomState(b), format="csr") + sp.eye(m, format="csr")
    A.sort_indices()
    A.sum_duplicates()
    op = rails_amd.HipOperatorWrapper.from_scipy(ctx, A, block_size=b)
    assert op.block_size == b
    S = sp.bsr_matrix(A, blocksize=(b, b))
    S.sort_indices()  # a bsr_matrix goes in as it is stored: with its block columns ascending it is the conversion's own result
    same = rails_amd.HipOperatorWrapper.from_scipy(ctx, S)
    ref = rails_amd.HipOperatorWrapper.from_scipy(ctx, A)
    assert same.block_size == b and ref.block_size == 1
    ref.set_variant(3)
    for nc in (16, 5, 33):
        Xh = np.random.default_rng(nc).uniform(-1.0, 1.0, (m, nc))
        want = product(ctx, ref, Xh)
        assert ref.last_kernel() == "k_spmm_rowgather"
        assert np.array_equal(product(ctx, op, Xh, xoff=1), want)
        assert np.array_equal(product(ctx, same, Xh, yoff=1), want)


def test_errors(ctx):
    import rails_amd
    from rails_amd import _lib

    g = np.random.default_rng(0)
    ip, ix = np.array([0, 1, 2], dtype=np.int64), np.array([0, 1], dtype=np.int32)
    for b in (1, 9):
        with pytest.raises(rails_amd.RailsError, match=r"code -1\).*block size %d outside 2 \.\. 8" % b):
            rails_amd.HipOperatorWrapper.from_bsr(ctx, ip, ix, g.uniform(-1, 1, (2, b, b)))
    data = g.uniform(-1, 1, (2, 2, 2))
    h = C.c_void_p()
    rc = ctx.lib.rails_csr_create_bsr(ctx.h, 2, 3, 2, ip.ctypes.data_as(C.POINTER(C.c_int64)), ix.ctypes.data_as(C.POINTER(C.c_int32)), data.ctypes.data_as(C.POINTER(C.c_double)),
                                      C.byref(h))
    assert rc == -1 and b"2 block rows but 3 block columns" in ctx.lib.rails_last_error() and not h.value
    with pytest.raises(rails_amd.RailsError, match=r"code -1\).*block column 2 out of range"):
        rails_amd.HipOperatorWrapper.from_bsr(ctx, ip, np.array([0, 2], dtype=np.int32), data)
    two = rails_amd.Context(device=0, seed=1)
    try:
        two.set_partition(0, 2, 0, 8)
        with pytest.raises(rails_amd.RailsError, match=r"code -1\).*single GPU only"):
            rails_amd.HipOperatorWrapper.from_bsr(two, ip, ix, data)
    finally:
        two.close()
    op = rails_amd.HipOperatorWrapper.from_bsr(ctx, ip, ix, data)
    rc = ctx.lib.rails_csr_set_halo(op.h.h, 0, None, 0, _lib.HALO_FN(0), None)
    assert rc == -1 and b"a block-CSR operator is single GPU only" in ctx.lib.rails_last_error()
    # accepted and without effect
    op.set_variant(3)
    assert op.prepare(16) is False
    X = rails_amd.HipMultiVectorWrapper(ctx, data=g.uniform(-1, 1, (4, 6)))
    with pytest.raises(rails_amd.RailsError, match=r"code -1\).*X and Y windows alias"):
        op.apply(X.view(0, 3), X.view(2, 5))
    with pytest.raises(rails_amd.RailsError, match=r"code -1\).*X has 5 rows"):
        op.apply(rails_amd.HipMultiVectorWrapper(ctx, data=g.uniform(-1, 1, (5, 2))))
    rc = ctx.lib.rails_csr_bsr_stats(rails_amd.HipOperatorWrapper(ctx, np.array([0, 1], dtype=np.int64), np.array([0], dtype=np.int32), np.ones(1)).h.h,
                                     (C.c_int64 * 10)(), 10)
    assert rc == -1 and b"not a block-CSR operator" in ctx.lib.rails_last_error()
    # an iterative solve over the handle: as over a callback operator, and what reads scalar CSR arrays is refused
    from rails_amd import problems as P

    spd = P.block_stencil7(3, 3, 2, 2, seed=1)[0]
    big = rails_amd.HipOperatorWrapper.from_bsr(ctx, *spd)
    with pytest.raises(rails_amd.RailsError, match=r"code -1\).*\"amg\" needs the entries of the matrix as scalar CSR arrays: the operator is block-CSR"):
        rails_amd.IterativeInverse(ctx, big, method="cg", amg=True)
    inv = rails_amd.IterativeInverse(ctx, big, method="cg", poly_degree=2)
    R = rails_amd.HipMultiVectorWrapper(ctx, data=g.uniform(-1, 1, (36, 2)))
    with pytest.raises(rails_amd.RailsError, match=r"code -1\).*poly_degree 2 needs an upper bound on the spectrum: a block-CSR operator keeps no scalar CSR arrays"):
        inv.solve(R)
    inv.close()


PARAMS = {"Restart size": 60, "Reduced size": 30, "Expand size": 4, "Lanczos iterations": 6, "Tolerance": 1e-6}


def solve_with(ctx, op, B, subspace, M=None):
    import rails_amd

    ctx.set_seed(5, 0)
    s = rails_amd.Solver(ctx, op, B, M=M)
    assert s.set_parameters(PARAMS) == 0
    s.set_option("verbose", 0)
    s.set_option("subspace", subspace)
    if M is not None:
        s.set_option("mass", 1)
    kernels = []
    s.set_trip_callback(lambda trip: kernels.append(op.last_kernel()))
    code, V, T = s.solve()
    # (the first call comes before the solve's first product: the handle then names no kernel yet)
    assert kernels and all(kernels[1:]), kernels
    out = dict(code=code, trips=s.trips(), history=s.history().copy(), V=V, T=T, kernels=set(kernels[1:]) | {op.last_kernel()})
    s.close()
    return out


@pytest.mark.parametrize("grid,b,subspace,mass", [((6, 6, 6), 4, 1, False), ((6, 6, 6), 4, 0, False), ((5, 5, 4), 6, 1, False), ((5, 5, 4), 6, 0, False), ((5, 5, 4), 6, 1, True),
                                                   ((6, 6, 6), 4, 0, True)])
def test_solve_is_the_row_gather_solve_bit_for_bit(ctx, grid, b, subspace, mass):
    import rails_amd
    from rails_amd import problems as P

    bsr_arrays, csr_arrays = P.block_stencil7(*grid, b)
    m = csr_arrays[0].size - 1
    B = P.rhs(m, 4, seed=3)
    M = rails_amd.HipOperatorWrapper(ctx, *P.mass_diag(m)) if mass else None
    blocked = rails_amd.HipOperatorWrapper.from_bsr(ctx, *bsr_arrays)
    plain = rails_amd.HipOperatorWrapper(ctx, *csr_arrays)
    plain.set_variant(3)
    want = solve_with(ctx, plain, B, subspace, M)
    # first: the forced handle ran the row-gather kernel in every product the solve looked at
    assert want["kernels"] == {"k_spmm_rowgather"}, want["kernels"]
    got = solve_with(ctx, blocked, B, subspace, M)
    assert got["kernels"] == {"k_spmm_bsr"}, got["kernels"]
    assert want["code"] == 0 and 2 <= want["trips"] <= 60
    assert got["code"] == want["code"] and got["trips"] == want["trips"]
    assert np.array_equal(got["history"], want["history"])
    assert np.array_equal(got["V"], want["V"]) and np.array_equal(got["T"], want["T"])


def test_cpp_program_solves_on_both_back_ends():
    exe = os.path.join(LIBDIR, "bsr_solve")
    if not os.path.exists(exe):
        import rails_amd.build

        rails_amd.build.build()
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("OK"), p.stdout[-4000:]
    assert p.stdout.count("the same bits") == 2 and "direct back end: block-CSR returned 0" in p.stdout and "coordinate-space back end: block-CSR returned 0" in p.stdout


def test_driver_block_size(tmp_path):
    """python -m rails_amd.main --block-size 3 against the run without the flag, at the tolerance of the oracle parity tests
    (tests/test_gpu_solver.py: ||X - X'||_F <= 10 * tol * ||X'||_F)"""
    from rails_amd import mmio
    from rails_amd import problems as P

    _, (rowptr, col, val) = P.block_stencil7(5, 4, 3, 3, seed=4)
    m = rowptr.size - 1
    mmio.write_csr(str(tmp_path / "A.mtx"), m, m, rowptr, col.astype(np.int64), val)
    mmio.write_array(str(tmp_path / "B.mtx"), P.rhs(m, 3, seed=1))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    tol = 1e-6
    base = [sys.executable, "-m", "rails_amd.main", "--dir", str(tmp_path), "--no-mass", "--set", "Tolerance=%r" % tol, "--set", "Expand size=3", "--set", "Lanczos iterations=5"]
    X = []
    for extra in ([], ["--block-size", "3", "--V", "Vb.mtx", "--T", "Tb.mtx"]):
        p = subprocess.run(base + extra, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        print(p.stdout[-1500:])
        assert p.returncode == 0, p.stdout[-3000:]
        V, T = mmio.read_dense(str(tmp_path / (extra[3] if extra else "V.mtx"))), mmio.read_dense(str(tmp_path / (extra[5] if extra else "T.mtx")))
        X.append(V @ T @ V.T)
    (line,) = [ln for ln in p.stdout.splitlines() if "as block-CSR" in ln]
    nnzb = 7 * 60 - 2 * (5 * 4 + 4 * 3 + 5 * 3)
    assert "A as block-CSR: %d blocks of 3 x 3, fill ratio 1.000" % nnzb in line and "%d bytes on the device" % (nnzb * 76 + 61 * 8) in line
    assert np.linalg.norm(X[1] - X[0]) <= 10 * tol * np.linalg.norm(X[0])
    # refusals: rows that are no multiple of the block size, more than one rank
    p = subprocess.run(base + ["--block-size", "7"], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode != 0 and "A has 180 rows, no multiple of 7" in p.stdout
    p = subprocess.run(base + ["--block-size", "3"], env=dict(env, WORLD_SIZE="2", RANK="0"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode != 0 and "--block-size on 2 ranks: a block-CSR operator is single GPU" in p.stdout
