"""The block-Jacobi preconditioner of the iterative A^-1 operator (include/rails_hip.h: rails_iter_block_jacobi, "block_jacobi";
rails_amd/csrc/iter_hierarchy.hip for the install, itsolve.hip, iter_kernels.inc) on the GPU: the preconditioner on its own against the library's own
inverse blocks within b eps (|Ginv| |X|), through windows bit for bit; converged solves on rails_amd.problems.block_coupled7 asked for
four ways, against the float64 restatement's iteration counts and against point Jacobi on the same handle; the three sources of the
blocks; the block-CSR handle against the CSR handle forced to row-gather; the toggle; every refusal that needs a device, each leaving
the object usable; and one Lyapunov solve with the inverse Krylov projection."""
import numpy as np
import pytest

import block_jacobi_reference as BJ
import iter_reference as R
import iter_steps_reference as S

pytestmark = pytest.mark.gpu

TOL = 1e-10
PANEL, XC0, YC0 = 120, 37, 51  # windows at odd columns of panels 120 columns wide
SENTINEL = 7.25
SPREAD, SKEW = 1e3, 0.4


@pytest.fixture(scope="module")
def ctx():
    import rails_amd

    c = rails_amd.Context(device=0, seed=3)
    yield c
    c.close()


_problems = {}


def problem(nx, ny, nz, b, skew):
    """(block-CSR arrays, CSR triple, scipy matrix) of block_coupled7 at spread 1e3, computed once"""
    from rails_amd import problems as P

    key = (nx, ny, nz, b, skew)
    if key not in _problems:
        bsr, csr = P.block_coupled7(nx, ny, nz, b, SPREAD, skew=skew, seed=0)
        _problems[key] = (bsr, csr, BJ.csr_of(csr))
    return _problems[key]


def window(mv, c0, nc):
    return mv.view(c0, c0 + nc - 1) if nc > 1 else mv.view(c0)


def through_windows(ctx, call, Bm):
    """call(X, Y) through windows at odd columns of a NaN-filled X panel and a sentinel-filled Y panel: the window of Y; checks that X
    and everything beside Y's window are as they were"""
    import rails_amd

    n, nc = Bm.shape
    big = np.full((n, PANEL), np.nan)
    big[:, XC0:XC0 + nc] = Bm
    Xp = rails_amd.HipMultiVectorWrapper(ctx, data=big)
    Yp = rails_amd.HipMultiVectorWrapper(ctx, data=np.full((n, PANEL), SENTINEL))
    call(window(Xp, XC0, nc), window(Yp, YC0, nc))
    assert np.array_equal(Xp.to_host(), big, equal_nan=True)
    Yh = Yp.to_host()
    assert np.all(Yh[:, :YC0] == SENTINEL) and np.all(Yh[:, YC0 + nc:] == SENTINEL)
    return Yh[:, YC0:YC0 + nc].copy()


def solve_all_ways(ctx, inv, Bm, trans=False):
    """the four ways of tests/test_gpu_iter.py: handle / rails_iter_solve x full panels / windows"""
    import rails_amd

    n, nc = Bm.shape
    out = []
    op = inv.op.transpose() if trans else inv.op
    for through_handle in (False, True):
        call = (lambda X, Y: op.apply(X, Y)) if through_handle else (lambda X, Y: inv.solve(X, Y, trans=trans))
        X = rails_amd.HipMultiVectorWrapper(ctx, data=Bm)
        Y = rails_amd.HipMultiVectorWrapper(ctx, n, nc)
        call(X, Y)
        assert np.array_equal(X.to_host(), Bm)
        out.append(Y.to_host())
        out.append(through_windows(ctx, call, Bm))
    return out


# ---------------------------------------------------------------------------------------------------------------- the preconditioner
@pytest.mark.parametrize("b,w", list(zip(BJ.BS, (33, 1, 17, 2, 9, 3, 5))))
def test_precondition_is_the_block_product(ctx, b, w):
    """rails_iter_precondition with block Jacobi on: blockdiag(the library's own inverse blocks) X within b eps (|Ginv| |X|), on 301 block
    rows (two slabs at the narrow widths would need more: the step test has them), full panels and windows bit for bit"""
    import rails_amd

    bsr, csr, A = problem(7, 43, 1, b, SKEW)
    op = rails_amd.HipOperatorWrapper.from_bsr(ctx, *bsr)
    inv = rails_amd.IterativeInverse(ctx, op, method="bicgstab", block_jacobi=True)
    info = inv.block_jacobi_info()
    G = info["inverse"]
    assert info["b"] == b and info["blocks"] == 301 and G.shape == (301, b, b)
    # the library's inverse against the longdouble one (the host test has the componentwise bound; here: they are the same blocks)
    Xld, W, V = BJ.inverse_ld(BJ.diagonal_blocks(A, b))
    assert np.all(np.abs(G.astype(BJ.LD) - Xld) <= BJ.inverse_bound(Xld, W, V))
    Xh = np.random.default_rng(b).uniform(-1.0, 1.0, (A.shape[0], w))
    full = inv.precondition(rails_amd.HipMultiVectorWrapper(ctx, data=Xh)).to_host()
    want = BJ.apply_blocks(G, Xh.astype(BJ.LD))
    err = np.abs(full.astype(BJ.LD) - want).astype(np.float64)
    bound = BJ.apply_bound(G, Xh)
    print("b = %d, %d columns: largest error / bound %.3f" % (b, w, (err / bound).max()))
    assert np.all(err <= bound)
    assert inv.stats()["products"] == 0 and inv.stats()["launches"] == len(S.groups(w))  # one kernel per group, no product with A
    win = through_windows(ctx, lambda X, Y: inv.precondition(X, Y), Xh)
    assert np.array_equal(win, full)
    inv.close()


@pytest.mark.parametrize("b", BJ.BS)
def test_precondition_on_one_block_row(ctx, b):
    """m = b, one block row and one slab in which every thread but those of row class 0 loads block row 0 again and stores nothing:
    G X within b eps (|Ginv| |X|) at 1, 2, 3 and 33 columns, windows bit for bit"""
    import rails_amd

    bsr, csr, A = problem(1, 1, 1, b, SKEW)
    inv = rails_amd.IterativeInverse(ctx, rails_amd.HipOperatorWrapper.from_bsr(ctx, *bsr), method="bicgstab", block_jacobi=True)
    G = inv.block_jacobi_info()["inverse"]
    assert G.shape == (1, b, b)
    for w in (1, 2, 3, 33):
        Xh = np.random.default_rng(10 * b + w).uniform(-1.0, 1.0, (b, w))
        full = inv.precondition(rails_amd.HipMultiVectorWrapper(ctx, data=Xh)).to_host()
        err = np.abs(full.astype(BJ.LD) - BJ.apply_blocks(G, Xh.astype(BJ.LD))).astype(np.float64)
        assert np.all(err <= BJ.apply_bound(G, Xh)), (b, w, (err / BJ.apply_bound(G, Xh)).max())
        assert np.array_equal(through_windows(ctx, lambda X, Y: inv.precondition(X, Y), Xh), full)
    inv.close()


def test_block_jacobi_true_needs_a_block_size(ctx):
    """block_jacobi=True on a CSR operator without block_size would be the clearing call: the constructor refuses it"""
    import rails_amd

    bsr, csr, A = problem(1, 1, 1, 4, SKEW)
    with pytest.raises(ValueError, match="needs block_size"):
        rails_amd.IterativeInverse(ctx, A, method="bicgstab", block_jacobi=True)
    inv = rails_amd.IterativeInverse(ctx, A, method="bicgstab", block_jacobi=True, block_size=4)
    assert inv.block_jacobi_info()["blocks"] == 1
    inv.close()


# ---------------------------------------------------------------------------------------------------------------- converged solves
GRIDS = ((6, 6, 6, 4), (5, 5, 4, 6), (8, 8, 8, 3))
METHODS = (("cg", False, 0.0), ("bicgstab", False, SKEW), ("bicgstab", True, SKEW))
_counts = {}


@pytest.mark.parametrize("nc", (3, 17))
@pytest.mark.parametrize("method,trans,skew", METHODS)
@pytest.mark.parametrize("grid", GRIDS)
def test_converged_solves(ctx, grid, method, trans, skew, nc):
    import rails_amd

    nx, ny, nz, b = grid
    bsr, csr, A = problem(nx, ny, nz, b, skew)
    m = A.shape[0]
    Bm = R.rhs(m, nc)
    op = rails_amd.HipOperatorWrapper.from_bsr(ctx, *bsr)
    inv = rails_amd.IterativeInverse(ctx, op, method=method, tol=TOL, maxit=5000, block_jacobi=True)
    G = inv.block_jacobi_info()["inverse"]
    results = solve_all_ways(ctx, inv, Bm, trans)
    it, rel, flags = inv.columns()
    for Xg in results:
        assert np.all(np.isfinite(Xg))
        assert R.true_relres(A, Xg, Bm, trans=trans).max() <= 10 * TOL
        assert np.array_equal(Xg, results[0])  # the same bits whichever way the solve was asked for
    assert np.all(flags == 2) and np.all(rel <= TOL)
    want = BJ.iterations(method, A, Bm, TOL, "block", G, trans)
    assert np.all(it <= 1.5 * want), (it, want)
    # point Jacobi on the same handle (the diagonal given: a block-CSR handle keeps no scalar diagonal)
    point = rails_amd.IterativeInverse(ctx, op, method=method, tol=TOL, maxit=5000, diag=A.diagonal())
    point.solve(rails_amd.HipMultiVectorWrapper(ctx, data=Bm), trans=trans)
    pit, _, pflags = point.columns()
    point.close()
    inv.close()
    print("%s %s trans %d, %d columns: block Jacobi %d..%d iterations (restatement %d..%d), point Jacobi %d..%d" % (
        grid, method, trans, nc, it.min(), it.max(), want.min(), want.max(), pit.min(), pit.max()))
    assert np.all(pflags == 2)
    assert pit.min() >= 2 * it.max(), (pit, it)


# ---------------------------------------------------------------------------------------------------------------- sources, handles, toggle
@pytest.mark.parametrize("method,trans,skew", METHODS)
def test_sources_of_the_blocks_and_the_two_handles(ctx, method, trans, skew):
    """blocks from the block-CSR handle, from the CSR handle with b, and passed explicitly: the same inverse bits; iterating on the
    block-CSR handle and on the CSR handle forced to row-gather: the same solve bits (the block-CSR product makes the CSR product's fused
    multiply-adds in the same order, tests/test_gpu_bsr.py)"""
    import rails_amd

    nx, ny, nz, b = 5, 5, 4, 6
    bsr, csr, A = problem(nx, ny, nz, b, skew)
    Bm = R.rhs(A.shape[0], 5)
    blocked = rails_amd.HipOperatorWrapper.from_bsr(ctx, *bsr)
    plain = rails_amd.HipOperatorWrapper(ctx, csr[0], csr[1].astype(np.int32), csr[2])
    plain.set_variant(3)
    made = {
        "bsr": rails_amd.IterativeInverse(ctx, blocked, method=method, tol=TOL, block_jacobi=True),
        "bsr, b named": rails_amd.IterativeInverse(ctx, blocked, method=method, tol=TOL, block_jacobi=True, block_size=b),
        "csr": rails_amd.IterativeInverse(ctx, plain, method=method, tol=TOL, block_jacobi=True, block_size=b),
        "explicit on bsr": rails_amd.IterativeInverse(ctx, blocked, method=method, tol=TOL, block_jacobi=BJ.diagonal_blocks(A, b)),
        "explicit on csr": rails_amd.IterativeInverse(ctx, plain, method=method, tol=TOL, block_jacobi=BJ.diagonal_blocks(A, b)),
        "matrix": rails_amd.IterativeInverse(ctx, A, method=method, tol=TOL, block_jacobi=True, block_size=b),
    }
    made["matrix"].A.set_variant(3)
    infos = {k: v.block_jacobi_info() for k, v in made.items()}
    sols = {k: (v.solve_host(Bm, trans=trans), v.columns()) for k, v in made.items()}
    assert plain.last_kernel() == "k_spmm_rowgather" and blocked.last_kernel().startswith("k_spmm_bsr")
    first = "bsr"
    for k in made:
        assert infos[k]["b"] == b and infos[k]["blocks"] == nx * ny * nz and np.array_equal(infos[k]["inverse"], infos[first]["inverse"]), k
        assert np.array_equal(sols[k][0], sols[first][0]), k
        assert all(np.array_equal(x, y) for x, y in zip(sols[k][1], sols[first][1])), k
    assert np.all(sols[first][1][2] == 2)
    for v in made.values():
        v.close()


@pytest.mark.parametrize("method", ("cg", "bicgstab"))
def test_toggle_gives_the_bits_of_an_object_without_blocks(ctx, method):
    import rails_amd

    bsr, csr, A = problem(5, 5, 4, 6, 0.0 if method == "cg" else SKEW)
    Bm = R.rhs(A.shape[0], 4)
    plain = rails_amd.HipOperatorWrapper(ctx, csr[0], csr[1].astype(np.int32), csr[2])
    never = rails_amd.IterativeInverse(ctx, plain, method=method, tol=TOL, maxit=5000)
    want, want_cols, want_stats = never.solve_host(Bm), never.columns(), never.stats()
    inv = rails_amd.IterativeInverse(ctx, plain, method=method, tol=TOL, maxit=5000, block_jacobi=True, block_size=6)
    on, on_cols = inv.solve_host(Bm), inv.columns()
    assert on_cols[0].max() * 2 <= want_cols[0].min()
    inv.set("block_jacobi", 0)
    off, off_cols, off_stats = inv.solve_host(Bm), inv.columns(), inv.stats()
    assert np.array_equal(off, want) and all(np.array_equal(x, y) for x, y in zip(off_cols, want_cols))
    assert off_stats["launches"] == want_stats["launches"] and off_stats["products"] == want_stats["products"]
    inv.set("block_jacobi", 1)
    again = inv.solve_host(Bm)
    assert np.array_equal(again, on)
    # clearing: no blocks, the setting off, point Jacobi again
    info = inv.block_jacobi()
    assert info["blocks"] == 0 and info["b"] == 0 and info["inverse"].shape[0] == 0
    assert np.array_equal(inv.solve_host(Bm), want)
    never.close()
    inv.close()


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_object_usable(ctx):
    import rails_amd

    b = 4
    bsr, csr, A = problem(6, 6, 6, b, 0.0)
    m = A.shape[0]
    Bm = R.rhs(m, 3)
    blocked = rails_amd.HipOperatorWrapper.from_bsr(ctx, *bsr)
    plain = rails_amd.HipOperatorWrapper(ctx, csr[0], csr[1].astype(np.int32), csr[2])
    inv = rails_amd.IterativeInverse(ctx, blocked, method="cg", tol=TOL, block_jacobi=True)
    want = inv.solve_host(Bm)
    refused = lambda pattern: pytest.raises(rails_amd.RailsError, match=r"\(code -1\).*" + pattern)
    blocks = BJ.diagonal_blocks(A, b)

    def still_fine(obj=inv, expect=want):
        assert np.array_equal(obj.solve_host(Bm), expect)

    with refused("block size 2 on a block-CSR operator of block size 4"):
        inv.block_jacobi(b=2)
    still_fine()
    with refused("block size 2 on a block-CSR operator of block size 4"):
        inv.block_jacobi(BJ.diagonal_blocks(A, 2))
    still_fine()
    bad = blocks.copy()
    bad[17] = 0.0
    with refused(r"diagonal block 17 \(rows 68 \.\. 71\).*pivot"):
        inv.block_jacobi(bad)
    still_fine()
    bad[17] = blocks[17]
    bad[5, 2, 1] = np.nan
    with refused("diagonal block 5 "):
        inv.block_jacobi(bad)
    still_fine()
    bad[5] = blocks[5]
    bad[9] = np.diag([1e-320, 1.0, 1.0, 1.0])
    with refused("inverse of diagonal block 9 .*not finite"):
        inv.block_jacobi(bad)
    still_fine()
    with refused(r"poly_degree 2 together with \"block_jacobi\""):
        inv.set("poly_degree", 2)
    still_fine()
    # "amg" is refused on a block-CSR handle for its own reason; the pair is refused on a CSR handle, in either order
    on_csr = rails_amd.IterativeInverse(ctx, plain, method="cg", tol=TOL, block_jacobi=True, block_size=b)
    want_csr = on_csr.solve_host(Bm)
    with refused(r"\"amg\" together with \"block_jacobi\""):
        on_csr.set("amg", 1)
    with refused(r"poly_degree 3 together with \"block_jacobi\""):
        on_csr.set("poly_degree", 3)
    with refused("block size 9 is not in 2 .. 8"):
        on_csr.block_jacobi(b=9)
    with refused("block size 5 does not divide the operator's 864 rows"):
        on_csr.block_jacobi(b=5)
    still_fine(on_csr, want_csr)
    on_csr.set("block_jacobi", 0)
    on_csr.set("poly_degree", 2)
    with refused(r"\"block_jacobi\" together with poly_degree 2"):
        on_csr.set("block_jacobi", 1)
    with refused("together with poly_degree 2"):
        on_csr.block_jacobi(b=b)
    on_csr.set("poly_degree", 0)
    on_csr.set("amg", 1)
    with refused(r"\"block_jacobi\" together with \"amg\""):
        on_csr.set("block_jacobi", 1)
    with refused(r"together with \"amg\""):
        on_csr.block_jacobi(b=b)
    on_csr.set("amg", 0)
    on_csr.set("block_jacobi", 1)
    still_fine(on_csr, want_csr)
    on_csr.close()
    # "block_jacobi" 1 without blocks; no blocks given on a callback, an LU and an iterative-solve handle
    none = rails_amd.IterativeInverse(ctx, plain, method="cg", tol=TOL)
    with refused(r"\"block_jacobi\" 1 without blocks"):
        none.set("block_jacobi", 1)
    assert none.block_jacobi_info()["blocks"] == 0
    def action(trans, X, Y):
        blocked.apply(X, Y)
        return 0

    cb = rails_amd.HipOperatorWrapper.from_callback(ctx, m, action)
    on_cb = rails_amd.IterativeInverse(ctx, cb, method="cg", tol=TOL)
    with refused("the operator is a callback"):
        on_cb.block_jacobi(b=b)
    on_cb.block_jacobi(blocks)  # given explicitly: any square operator
    assert np.array_equal(on_cb.block_jacobi_info()["inverse"], inv.block_jacobi_info()["inverse"])
    assert np.array_equal(on_cb.solve_host(Bm), want)
    on_cb.close()
    on_iter = rails_amd.IterativeInverse(ctx, none.op, method="cg", tol=TOL)
    with refused("the operator is an iterative solve"):
        on_iter.block_jacobi(b=b)
    on_iter.close()
    lu = rails_amd.SparseLU(ctx, (csr[0], csr[1].astype(np.int32), csr[2]))
    on_lu = rails_amd.IterativeInverse(ctx, lu.op, method="bicgstab", tol=TOL)
    with refused("the operator is an LU handle"):
        on_lu.block_jacobi(b=b)
    on_lu.close()
    lu.close()
    none.close()
    # a context that reduces (an all-reduce hook on one rank)
    from rails_amd import _lib

    c2 = rails_amd.Context(device=0, seed=3)
    hook = _lib.ALLREDUCE_FN(lambda buf, dev, n, user: 0)
    assert c2.lib.rails_ctx_set_allreduce(c2.h, hook, None) == 0
    op2 = rails_amd.HipOperatorWrapper(c2, csr[0], csr[1].astype(np.int32), csr[2])
    red = rails_amd.IterativeInverse(c2, op2, method="cg", tol=TOL)
    with refused("a context that reduces"):
        red.block_jacobi(b=b)
    with refused("a context that reduces"):
        red.block_jacobi(blocks)
    red.block_jacobi()  # clearing is no use of the preconditioner
    red.close()
    c2.close()
    still_fine()
    inv.close()


# ---------------------------------------------------------------------------------------------------------------- a whole solve
def test_lyapunov_solve_with_the_inverse_krylov_projection(ctx):
    """"Projection method" 1.1 on block_coupled7(6, 6, 6, 4, 1e3), B of 4 columns: with the inverse on the block-CSR handle and block
    Jacobi the solve converges, its relative residual is within 10 x what the same solve reaches with the sparse LU as the inverse, and the
    inverse needs fewer than half of the inner iterations of the same solve with point Jacobi"""
    import rails_amd
    from rails_amd import problems as P

    b = 4
    bsr, csr, A = problem(6, 6, 6, b, 0.0)
    m = A.shape[0]
    B = P.rhs(m, 4, seed=2)
    params = {"Restart size": 80, "Reduced size": 40, "Expand size": 4, "Lanczos iterations": 8, "Tolerance": 1e-6, "Projection method": 1.1}
    op = rails_amd.HipOperatorWrapper.from_bsr(ctx, *bsr)

    def solve_with(inverse):
        s = rails_amd.Solver(ctx, op, B)
        assert s.set_parameters(params) == 0
        s.set_option("verbose", 0)
        s.set_inverse(inverse)
        code, V, T = s.solve()
        out = (code, s.relative_residual(), s.trips())
        s.close()
        return out

    def run(inverse):
        # In a thread of its own: the projected Lyapunov solve keeps what it learned per thread from call to call (lyap_dense.cpp:
        # resting routes, inherited shifts), whichever solver object calls.  The three solves here start alike that way, and the tests
        # elsewhere in the suite that compare two solves bit for bit find the main thread as this test found it.
        import threading

        box = {}

        def work():
            try:
                box["out"] = solve_with(inverse)
            except BaseException as e:  # handed to the main thread below
                box["error"] = e

        t = threading.Thread(target=work)
        t.start()
        t.join()
        if "error" in box:
            raise box["error"]
        return box["out"]

    lu = rails_amd.SparseLU(ctx, (csr[0], csr[1].astype(np.int32), csr[2]))
    code_lu, rel_lu, trips_lu = run(lu)
    lu.close()
    block = rails_amd.IterativeInverse(ctx, op, method="cg", tol=TOL, block_jacobi=True)
    code_b, rel_b, trips_b = run(block)
    total_b = block.stats()["total_iterations"]
    assert block.stats()["total_flagged_columns"] == 0
    block.close()
    point = rails_amd.IterativeInverse(ctx, op, method="cg", tol=TOL, diag=A.diagonal())
    code_p, rel_p, trips_p = run(point)
    total_p = point.stats()["total_iterations"]
    point.close()
    print("LU: code %d, %d trips, relative residual %.2e; block Jacobi: code %d, %d trips, %.2e, %d inner iterations; point Jacobi: code %d, %d trips, %.2e, %d" % (
        code_lu, trips_lu, rel_lu, code_b, trips_b, rel_b, total_b, code_p, trips_p, rel_p, total_p))
    assert code_lu == 0 and code_b == 0 and code_p == 0
    # (rails_solver_relative_residual is the true residual against ||B B'||, not the estimate the solve stops on: the LU solve's own
    # value is the yardstick, as for the smoke run)
    assert rel_lu <= 1e-4 and rel_b <= 10 * rel_lu
    assert total_b > 0 and 2 * total_b < total_p
