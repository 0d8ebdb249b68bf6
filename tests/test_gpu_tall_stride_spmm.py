"""The SpMM kernels on windows of panels whose byte extent crosses 2^31 and 2^32 (shapes, operators and the case table:
tests/tall_stride_cases.py, pinned on the CPU by test_tall_stride_cases_host.py; the panels: tests/tall_stride_device.py).

Several kernels address with 32 bits on purpose and a host rule keeps them away from panels they cannot reach; the others are written with
64-bit row offsets.  Here every one of them gathers X rows that start beyond byte 2^31 and beyond byte 2^32 of their panel: the 32-bit
ones just below their guard (offsets in [2^31, 2^32): a signed intermediate or a sign-extending addressing mode goes wrong there while
the guard still says yes) and their fall-backs just above it.  Every case asserts which kernel ran and equality with the exact integer
product, compares with the same product on compact panels bit for bit, and checks that the NaN put beside the windows is still there.

Every test makes its own context, holds at most 24 GiB of device memory at once (the largest single panel is 17.6 GB) and destroys its
tall panels before it ends."""
import numpy as np
import pytest

import bsr_reference as BR
import partition_ranks as PR
import spmm_reference as R
import tall_stride_cases as T
import tall_stride_device as D

pytestmark = pytest.mark.gpu


def make_operator(ctx, o, variant):
    import rails_amd

    if o.n_rows == o.n_cols:
        op = rails_amd.HipOperatorWrapper(ctx, o.rowptr, o.col, o.val)
    else:
        op = rails_amd.HipOperatorWrapper.rect(ctx, o.n_rows, o.n_cols, o.rowptr, o.col, o.val)
    op.set_variant(variant)
    return op


def tall_product(ctx, op, Xh, x_rows, y_rows, ldx, ldy, xoff, yoff):
    """(Y, kernel) of Y = A Xh with X the window at column xoff of an x_rows x ldx panel and Y the window at column yoff of a y_rows x ldy
    panel (ldy None: of a compact panel); the guards of both are checked"""
    nc = Xh.shape[1]
    with D.tall(ctx, x_rows, ldx) as XP:
        X = XP.guarded(xoff, nc, Xh)
        if ldy is None:
            out = D.CompactOut(ctx, y_rows, yoff, nc)
            op.apply(X, out.view)
            kernel = op.last_kernel()
            Y = out.view.to_host()
            assert out.intact(), "columns beside the Y window were written"
        else:
            with D.tall(ctx, y_rows, ldy) as YP:
                Yw = YP.guarded(yoff, nc)
                Yw.assign(D.NAN)
                op.apply(X, Yw)
                kernel = op.last_kernel()
                Y = Yw.to_host()
                assert YP.intact(), "columns beside the Y window were written"
        assert XP.intact() and D.same_bits(X.to_host(), Xh), "the X panel was written"
    return Y, kernel


def assert_exact(Y, want, tag):
    bad = np.argwhere(Y != want)
    assert bad.size == 0, "%s: %d entries differ from the exact product, first at %s: %r instead of %r" % (
        tag, len(bad), bad[0], Y[tuple(bad[0])], want[tuple(bad[0])])


# --------------------------------------------------------------------------------------------------------------- the row kernels
@pytest.mark.parametrize("case", T.ROW_CASES, ids=[c.name for c in T.ROW_CASES])
def test_row_kernels(case):
    """k_spmm_narrow just below its guard (M_BELOW x LD_TALL: byte offsets up to 4.27e9), k_spmm_rowgather_cc and k_spmm_rowgather just
    above it and well above 4 GiB, square and rectangular (the extra rows follow X in the same panel)"""
    o = T.operator(case.rows, case.cols)
    Xh, want = np.asfortranarray(o.X[:, :case.nc]), o.ref[:, :case.nc]
    with D.context() as ctx:
        op = make_operator(ctx, o, case.variant)
        Y, kernel = tall_product(ctx, op, Xh, case.cols, case.rows, case.ldx, case.ldy, case.xoff, case.yoff)
        assert kernel == case.kernel, (case, kernel)
        assert_exact(Y, want, case.name)
        assert (Y[np.diff(o.rowptr) == 0] == 0).all()
        # the same product on compact panels
        Yc = op.apply(D.MV(ctx, data=Xh)).to_host()
        assert D.same_bits(Y, Yc), case.name


# --------------------------------------------------------------------------------------------------- the lean kernel's ghost form
@pytest.mark.parametrize("m_local,kernel", [(T.M_BELOW, T.NARROW), (T.M_ABOVE, T.CC)], ids=["below", "above"])
def test_ghost_rows_on_two_ranks(m_local, kernel):
    """two rank threads, each with its block of a 2 m_local-row operator: the local X is a window of an m_local x LD_TALL panel, so local
    rows are addressed past 2^31 (and, above the guard, past 2^32) while the ghost rows come from the halo buffer.  Below the guard the
    ghost form of k_spmm_narrow, above it the chunked kernel; the stacked result is the exact global product"""
    from test_gpu_partition import _rank_setup

    o = T.operator(2 * m_local)
    nc, xoff = 16, 2
    starts = np.array([0, m_local, 2 * m_local], dtype=np.int64)
    ranks = PR.MailboxRanks(2)

    def work(r):
        ctx, op, plan = _rank_setup(ranks, r, starts, (o.rowptr, o.col, o.val), seed=5)
        try:
            op.set_variant(1)
            r0, r1 = int(starts[r]), int(starts[r + 1])
            Xh = np.asfortranarray(o.X[r0:r1, :nc])
            with D.tall(ctx, m_local, T.LD_TALL) as XP:
                X = XP.guarded(xoff, nc, Xh)
                out = D.CompactOut(ctx, m_local, 0, nc)
                op.apply(X, out.view)
                res = dict(Y=out.view.to_host(), kernel=op.last_kernel(), n_ghost=plan.n_ghost, n_send=plan.n_send, intact=out.intact() and XP.intact())
            return res
        finally:
            ctx.close()

    res = ranks.run(work)
    for r in range(2):
        assert res[r]["n_ghost"] > 0 and res[r]["n_send"] > 0 and res[r]["intact"], r
        assert res[r]["kernel"] == kernel, (r, res[r]["kernel"])
    assert_exact(np.vstack([res[0]["Y"], res[1]["Y"]]), o.ref[:, :nc], "ghost rows, m_local = %d" % m_local)
    assert ranks.exchanges == [1, 1]


# -------------------------------------------------------------------------------------------------------- the LDS-staged kernels
TILED_M_BELOW, TILED_M_ABOVE = 1072, 1100  # 1072 x LD_TALL = 2.144e9 elements < 0x7fffffff <= 1100 x LD_TALL; 17.2 GB and 17.6 GB


def _tiled_operator(m):
    from rails_amd import problems as P

    rowptr, col, _ = P.banded_random(m, 12, 40, seed=1)
    # every row also gathers the last row of the panel: an element offset of 2^31 - 3.0e6 below the guard, beyond 2^31 above it
    rows = np.repeat(np.arange(m), np.diff(rowptr))
    last = col[np.asarray(rowptr[1:]) - 1]
    col = np.array(col, dtype=np.int64)
    col[np.asarray(rowptr[1:]) - 1] = np.where(last < m - 1, m - 1, last)
    assert np.all(np.diff(col)[rows[1:] == rows[:-1]] >= 0)  # (a row may name a column twice: entries add up)
    val = R.int_values(col.size, seed=7)
    X = R.int_panel(m, 64)
    return rowptr, col, val, X, R.spmm_exact_int(rowptr, col, val, X)


@pytest.mark.parametrize("m,kernels", [(TILED_M_BELOW, (T.TILED_REG,)), (TILED_M_ABOVE, (T.TILED_PIPE, T.TILED))], ids=["reg_below", "refused_above"])
def test_lds_staged_kernels(m, kernels):
    """variant 2 on a banded operator (12 entries per row, the pattern of test_gpu_spmm_tiled.py's banded_12_40 at fewer rows) with X in
    one m x LD_TALL panel.  m * ldx below 2^31 elements: the register kernel, whose 31-bit element offsets reach 2^29 and more (4 GiB
    and more in bytes) from row 269 on, up to 2.144e9 at the last row.  From 0x7fffffff elements on it is refused and the pipelined or
    the plain staged kernel computes the same bits"""
    assert T.tiled_reg_allowed(m, T.LD_TALL) == (kernels[0] == T.TILED_REG) and T.panel_bytes(m, T.LD_TALL) < 24 << 30
    rowptr, col, val, Xall, ref = _tiled_operator(m)
    with D.context() as ctx:
        import rails_amd

        op = rails_amd.HipOperatorWrapper(ctx, rowptr, col, val)
        op.set_variant(2)
        with D.tall(ctx, m, T.LD_TALL) as XP:
            for nc in (16, 64):
                Xh = np.asfortranarray(Xall[:, :nc])
                X = XP.guarded(2, nc, Xh)
                out = D.CompactOut(ctx, m, 0, nc)
                op.apply(X, out.view)
                st = op.tile_stats()
                assert st["accepted"] and op.last_kernel() == st["kernel"] and st["kernel"] in kernels, (nc, st, op.last_kernel())
                Y = out.view.to_host()
                assert out.intact() and XP.intact()
                assert_exact(Y, ref[:, :nc], "tiled m = %d, nc = %d" % (m, nc))
                Yc = op.apply(D.MV(ctx, data=Xh)).to_host()
                assert D.same_bits(Y, Yc), (m, nc)


# ------------------------------------------------------------------------------------------------------------------ block-CSR
@pytest.mark.parametrize("b,mb", [(2, 134), (5, 54), (8, 34)])
def test_block_csr(b, mb):
    """k_spmm_bsr (bsr_row_gather.inc: src + r * ldx8) with tall X and tall Y, m = mb * b = 268, 270, 272 rows at LD_TALL; every block row's
    last block is the last block column, whose rows start beyond byte 2^32 for b = 5 and 8.  Against the exact block product and the
    same product on compact panels"""
    m = mb * b
    assert 264 <= m <= 272
    indptr, indices, data = BR.integer_problem(BR.counts_full(mb, 6), b, seed=10 + b)
    indptr, indices, data = BR.with_shared_column(indptr, indices, data, np.arange(mb), mb - 1)
    with D.context() as ctx:
        import rails_amd

        op = rails_amd.HipOperatorWrapper.from_bsr(ctx, indptr, indices, data)
        for nc, xoff, yoff in ((16, 2, 0), (17, 3, 3), (33, 0, 2)):
            Xh = np.asfortranarray(BR.integer_panel(m, nc, seed=3))
            want = BR.reference(indptr, indices, data, Xh)
            Y, kernel = tall_product(ctx, op, Xh, m, m, T.LD_TALL, T.LD_TALL, xoff, yoff)
            assert kernel == "k_spmm_bsr", kernel
            assert_exact(Y, want, "block-CSR b = %d, nc = %d" % (b, nc))
            Yc = op.apply(D.MV(ctx, data=Xh)).to_host()
            assert D.same_bits(Y, Yc), (b, nc)


def _int64_product(rowptr, col, val, X):
    """spmm_reference.spmm_exact_int's integers by scipy's CSR product on int64 arrays (a million rows of entries in one call)"""
    import scipy.sparse as sp

    vi, Xi = np.rint(val).astype(np.int64), np.rint(X).astype(np.int64)
    assert np.array_equal(vi, val) and np.array_equal(Xi, X)
    Y = sp.csr_matrix((vi, np.asarray(col), np.asarray(rowptr)), shape=(len(rowptr) - 1, X.shape[0])) @ Xi
    assert Y.dtype == np.int64
    return Y


# ------------------------------------------------------------------------------------------------------------- the plane sweep
@pytest.mark.parametrize("side", ["below", "above"])
def test_plane_sweep(side):
    """The smallest grid planes_reference.find_grid gives one z segment of seven planes at 16 columns on this device's CU count
    (513 x 17 x 7 on 256 CUs: 8721 rows per plane), the 7-point pattern with integer values.  The kernel addresses inside a plane with
    int element offsets and is guarded by gx gy max(ldx, ldy) 8 < 0x7fffffff: with ld the largest multiple of 16 below that (30768 on 256
    CUs, one plane of X 2,146,621,824 bytes, the panel 15.0 GB) k_spmm_planes runs, with 16 more (one plane 2,147,738,112 bytes) the
    automatic choice falls back to k_spmm_rowgather_cc.  Y is compact."""
    import planes_reference as PL
    import rails_amd
    from rails_amd import problems as P

    nc, xoff = 16, 2
    with D.context() as ctx:
        num_cu = int(ctx.lib.rails_ctx_num_cu(ctx.h))
        grid = PL.find_grid(nc, num_cu, 7, False)
        assert grid is not None and grid[2] == 7, grid
        gx, gy, gz = grid
        ld_below = (0x7FFFFFFF - 1) // (8 * gx * gy) // 16 * 16
        ld = ld_below if side == "below" else ld_below + 16
        assert T.planes_allowed(gx, gy, ld, 16) == (side == "below") and T.planes_allowed(gx, gy, ld_below, 16) and not T.planes_allowed(gx, gy, ld_below + 16, 16)
        m = gx * gy * gz
        assert T.panel_bytes(m, ld) < 24 << 30 and T.panel_bytes(gx * gy, ld) > T.TWO31 - (1 << 22)
        rowptr, col, _ = P.laplace7(gx, gy, gz)
        val = R.int_values(col.size, seed=7)
        Xh = np.asfortranarray(R.int_panel(m, nc))
        want = _int64_product(rowptr, col, val, Xh)
        op = rails_amd.HipOperatorWrapper(ctx, rowptr, col, val)
        op.set_variant(9 if side == "below" else 0)
        with D.tall(ctx, m, ld, 24) as XP:
            X = XP.guarded(xoff, nc, Xh)
            out = D.CompactOut(ctx, m, 0, nc)
            op.apply(X, out.view)
            kernel = op.last_kernel()
            st = op.planes_stats()
            Y = out.view.to_host()
            assert out.intact() and XP.intact()
        if side == "below":
            p = PL.plan(grid, nc, num_cu)
            assert kernel == "k_spmm_planes" and st["accepted"] and st["grid"] == tuple(grid) and (st["seglen"], st["nseg"]) == (7, 1) == (p["seglen"], p["nseg"]), (kernel, st)
        else:
            assert kernel == T.CC, (kernel, st)
        assert_exact(Y, want, "plane sweep, %s the guard" % side)
        Yc = op.apply(D.MV(ctx, data=Xh)).to_host()
        assert D.same_bits(Y, Yc) or np.array_equal(Y, Yc)  # (the sign of an exact zero may differ between two kernels)


# ------------------------------------------------------------------------------------------------------------- the sweep kernel
SWEEP_M, SWEEP_LD = 131072, 4352


@pytest.mark.parametrize("tall_y", (False, True), ids=["compact_y", "tall_y"])
def test_sweep_kernel(tall_y):
    """tests/test_gpu_sweep.py's banded operator of 131072 rows at 128 columns, forced (variant 7), with X a window of a panel whose rows
    are 4352 doubles apart (4.56 GB: rows from 123362 on start past 2^32) and then Y in such a panel as well.  The kernel advances 64-bit
    scalar bases per step and adds uint32 per-lane offsets; integer operands, the exact product"""
    import rails_amd
    from rails_amd import problems as P

    m, nc = SWEEP_M, 128
    assert SWEEP_LD % 16 == 0 and T.panel_bytes(m, SWEEP_LD) > T.TWO32 and T.row_start_byte(123362, SWEEP_LD) >= T.TWO32
    rowptr, col, _ = P.banded_random(m, 27, 4096, seed=m % 7)
    val = R.int_values(col.size, seed=7)
    Xh = np.asfortranarray(R.int_panel(m, nc))
    want = _int64_product(rowptr, col, val, Xh)
    with D.context() as ctx:
        op = rails_amd.HipOperatorWrapper(ctx, rowptr, col, val)
        op.set_variant(7)
        Y, kernel = tall_product(ctx, op, Xh, m, m, SWEEP_LD, SWEEP_LD if tall_y else None, 2, 4 if tall_y else 0)
        assert kernel.startswith("k_spmm_sweep"), kernel
        assert op.sweep_stats(nc)["built"]
        assert_exact(Y, want, "sweep")
