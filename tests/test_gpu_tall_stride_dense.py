"""The dense, BLAS-1, transfer, row-move and solve kernels on windows of panels whose byte extent crosses 2^32: these kernels are written
with int64_t row * ld, and nothing else in the suite would notice a single `int` in a row index.  Panels are M_FAR x LD_TALL (300 rows
2,000,000 doubles apart, 4.8 GB: rows start past 2^31 from row 135 and past 2^32 from row 269; tests/tall_stride_cases.py), windows sit at
columns 0 and 3, the columns beside a window hold NaN and must still hold it afterwards.

Operands are integers -- panels in [-16, 16], coefficient matrices in [-8, 8], every partial sum far below 2^53 -- so the Gram blocks,
panel updates, row forms and moves equal their int64 references bit for bit whatever the order of summation.  Where the arithmetic is not
exact (orthogonalisation, the Lanczos recurrence, triangular solves) the tall call is compared with the same call on compact panels,
bit for bit: the kernels do not know the leading dimension beyond the address arithmetic.

The widths are those at which tests/dense_choice_cases.py reaches each primitive's instantiation families, one per family; this is not a
second copy of test_gpu_dense_choice.py.  The one-pass update + second projection runs from 4096 rows on only (dense_choice.h), so its
panels are 4099 rows 140,000 doubles apart: 4.59 GB, rows start past 2^32 from row 3835.

Every test makes its own context and destroys its tall panels before it ends; at most four of them (19.2 GB) exist at once."""
import ctypes as C

import numpy as np
import pytest

import tall_stride_cases as T
import tall_stride_device as D

pytestmark = pytest.mark.gpu

DP = C.POINTER(C.c_double)
_i32p = C.POINTER(C.c_int32)
M, LD = T.DENSE_ROWS, T.DENSE_LD
OFFSETS = T.DENSE_OFFSETS


def chk(ctx, rc, what):
    from rails_amd._lib import check

    check(rc, what)


def fcol(A):
    return np.asfortranarray(A, dtype=np.float64)


def ptr(A):
    return A.ctypes.data_as(DP)


def exact(got, want, bound, tag):
    T.assert_exact(want, bound)
    assert got.shape == want.shape and np.array_equal(got, want), "%s: %d entries differ from the exact result" % (tag, int((got != want).sum()))


# ------------------------------------------------------------------------------------------------- transfers and BLAS-1
@pytest.mark.parametrize("off", OFFSETS)
def test_transfers_copy_fill_scale_axpy(off):
    nc = 33
    Ah, Bh = T.dense_panel(M, nc), T.dense_panel(M, nc, shift=9)
    with D.context() as ctx, D.tall(ctx, M, LD) as PA, D.tall(ctx, M, LD) as PB:
        a = PA.guarded(off, nc, fcol(Ah))
        assert D.same_bits(a.to_host(), Ah)  # upload and download of a window
        # a download with a host leading dimension of its own
        H = np.full((M + 5, nc), -7.25, order="F")
        chk(ctx, ctx.lib.rails_panel_download(ctx.h, PA.h, off, nc, ptr(H), M + 5), "rails_panel_download")
        assert np.array_equal(H[:M], Ah) and (H[M:] == -7.25).all()
        b = PB.guarded(3 - off, nc, fcol(Bh))
        ca, cb = D.MV(ctx, data=Ah), D.MV(ctx, data=Bh)
        # copy between two tall windows, and out of one into a compact panel
        b.assign(a)
        assert D.same_bits(b.to_host(), Ah)
        c = D.MV(ctx, m=M, n=nc + 2, capacity=nc + 2)
        c.assign(-7.25)
        c.view(1, nc).assign(a)
        assert np.array_equal(c.to_host()[:, 1:nc + 1], Ah) and (c.to_host()[:, [0, nc + 1]] == -7.25).all()
        # fill, scale, axpy
        b.assign(5.0)
        assert (b.to_host() == 5.0).all()
        b.from_host(fcol(Bh))
        b *= -3.0
        cb *= -3.0
        exact(b.to_host(), -3.0 * Bh, 48, "scale")
        b += a
        b -= PA.window(off, nc)
        b += a
        cb += ca
        exact(b.to_host(), -3.0 * Bh + Ah, 64, "axpy +-1")
        chk(ctx, ctx.lib.rails_panel_axpy(ctx.h, 7.0, PA.h, off, nc, PB.h, 3 - off), "rails_panel_axpy")
        chk(ctx, ctx.lib.rails_panel_axpy(ctx.h, 7.0, ca.panel.h, 0, nc, cb.panel.h, 0), "rails_panel_axpy")
        exact(b.to_host(), -3.0 * Bh + 8.0 * Ah, 256, "axpy 7")
        assert D.same_bits(b.to_host(), cb.to_host())
        assert PA.intact() and PB.intact() and D.same_bits(a.to_host(), Ah)


# ------------------------------------------------------------------------------------------------------------- Gram blocks
# (a, b) of rails_gram: k_gram's tile shapes, k_gram_cols at each of its TI, with and without the extra column
GRAM_SHAPES = ((1, 1), (1, 17), (17, 17), (17, 33), (33, 17), (17, 1), (128, 18), (128, 17), (193, 18), (289, 1), (289, 17), (257, 18), (257, 1))


@pytest.mark.parametrize("off", OFFSETS)
def test_gram_and_colnorms2(off):
    wmax = max(max(s) for s in GRAM_SHAPES)
    Xall, Yall = T.dense_panel(M, wmax), T.dense_panel(M, wmax, shift=7)
    bound = T.dense_partial_bound(M, 1)
    with D.context() as ctx, D.tall(ctx, M, LD, 304) as PX, D.tall(ctx, M, LD, 304) as PY:
        for a, b in GRAM_SHAPES:
            Xh, Yh = Xall[:, :a], Yall[:, :b]
            x, y = PX.guarded(off, a, fcol(Xh)), PY.guarded(3 - off, b, fcol(Yh))
            G = x.dot(y)
            exact(G, Xh.T @ Yh, bound, "gram %d x %d" % (a, b))
            assert D.same_bits(G, D.MV(ctx, data=Xh).dot(D.MV(ctx, data=Yh))), (a, b)
            # ... and of a window with itself
            exact(x.dot(x), Xh.T @ Xh, bound, "gram %d x %d, one panel" % (a, a))
            exact(x.colnorms2(), (Xh * Xh).sum(0), bound, "colnorms2 %d" % a)
            assert PX.intact() and PY.intact()


@pytest.mark.parametrize("off", OFFSETS)
def test_two_segment_gram_and_update(off):
    """rails_orthogonalize_deflated projects [N | V_old] out of a block as one left operand in two segments (k_gram2, k_gram_cols2,
    k_panel_gemm2): V in a tall panel (the orthogonalisation wants column 0: the window's offset is N's), N in another; the same call on
    compact panels gives the same bits"""
    g = np.random.default_rng(5)
    for a, w in ((5, 17), (24, 1), (132, 18)):
        q = 1 if a < 8 else 4
        NV = np.linalg.qr(g.uniform(-1, 1, (M, a)))[0]
        N, Vold, W = NV[:, :q], NV[:, q:], g.uniform(-1, 1, (M, w))
        VW = fcol(np.hstack([Vold, W]))
        with D.context() as ctx:
            c = D.MV(ctx, data=VW, capacity=a - q + w)
            c.orthogonalized = a - q
            used_c = c.orthogonalize_deflated(D.MV(ctx, data=N), 0)
            want = c.to_host()
            with D.tall(ctx, M, LD, 304) as PV, D.tall(ctx, M, LD) as PN:
                v = PV.guarded(0, a - q + w, VW)
                v.is_view = False
                v.orthogonalized = a - q
                used = v.orthogonalize_deflated(PN.guarded(off, q, fcol(N)), 0)
                got = v.to_host()
                assert PV.intact() and PN.intact()
            assert used == used_c and D.same_bits(got, want), (a, w)
            Q = got[:, a - q:]
            assert np.abs(NV.T @ Q).max() <= 1e-13 and np.abs(Q.T @ Q - np.eye(w)).max() <= 1e-13


# ------------------------------------------------------------------------------------------------------------- panel updates
@pytest.mark.parametrize("off", OFFSETS)
def test_panel_gemm(off):
    k = 33
    Xh = T.dense_panel(M, k)
    with D.context() as ctx, D.tall(ctx, M, LD) as PX, D.tall(ctx, M, LD) as PY:
        lib = ctx.lib
        PX.guarded(off, k, fcol(Xh))
        for r in (1, 17, 33, 65, 129):  # k_panel_gemm<1 | 2 | 4 | 8, 32>, <16, 16>
            Y0, Ch = T.dense_panel(M, r, shift=11), fcol(T.dense_coef(k, r, seed=r))
            for alpha, beta in ((1.0, 0.0), (-2.0, 1.0)):
                y = PY.guarded(3 - off, r, fcol(Y0))
                chk(ctx, lib.rails_panel_gemm(ctx.h, alpha, PX.h, off, k, ptr(Ch), k, r, beta, PY.h, 3 - off), "rails_panel_gemm")
                exact(y.to_host(), beta * Y0 + alpha * (Xh @ Ch), 16 + 2 * T.dense_partial_bound(1, k), "panel_gemm r = %d" % r)
                assert PY.intact() and PX.intact()
                cx, cy = D.MV(ctx, data=Xh), D.MV(ctx, data=Y0)  # (named: a temporary's panel is destroyed before the call reads its handle)
                chk(ctx, lib.rails_panel_gemm(ctx.h, alpha, cx.panel.h, 0, k, ptr(Ch), k, r, beta, cy.panel.h, 0), "rails_panel_gemm")
                assert D.same_bits(y.to_host(), cy.to_host()), (r, alpha, beta)


@pytest.mark.parametrize("off", OFFSETS)
def test_panel_gemm_wide(off):
    k = 32
    Xh = T.dense_panel(M, k)
    with D.context() as ctx, D.tall(ctx, M, LD) as PX, D.tall(ctx, M, LD, 304) as PY:
        lib = ctx.lib
        PX.guarded(off, k, fcol(Xh))
        for r, alpha, beta in ((65, 1.0, 0.0), (129, -1.0, 2.0), (273, 1.0, 0.0)):  # k_panel_gemm_wide<6 | 10 | 18>
            Y0, Qh = T.dense_panel(M, r, shift=11), fcol(T.dense_coef(k, r, seed=r))
            y = PY.guarded(3 - off, r, fcol(Y0))
            chk(ctx, lib.rails_panel_gemm_wide(ctx.h, alpha, PX.h, off, k, ptr(Qh), k, r, beta, PY.h, 3 - off), "rails_panel_gemm_wide")
            exact(y.to_host(), beta * Y0 + alpha * (Xh @ Qh), 32 + T.dense_partial_bound(1, k), "gemm_wide r = %d" % r)
            assert PY.intact() and PX.intact()
            cx, cy = D.MV(ctx, data=Xh), D.MV(ctx, data=Y0)
            chk(ctx, lib.rails_panel_gemm_wide(ctx.h, alpha, cx.panel.h, 0, k, ptr(Qh), k, r, beta, cy.panel.h, 0), "rails_panel_gemm_wide")
            assert D.same_bits(y.to_host(), cy.to_host()), r


UG_ROWS, UG_LD = 4099, 140_000


@pytest.mark.parametrize("pipeline", (1, 0), ids=["pipelined", "earlier"])
@pytest.mark.parametrize("in_place", (True, False), ids=["in_place", "out"])
def test_update_and_second_projection(pipeline, in_place):
    """rails_update_gram_deferred[_out] on 4099 x 140,000 panels (4.59 GB).  X at column 0: one pass (k_update_gram_p or k_update_gram by
    the schedule switch, asserted); X at column 3, rows only 8-byte aligned: the two separate kernels.  Y and the output sit at column 3
    of panels of their own."""
    assert UG_LD % 16 == 0 and T.panel_bytes(UG_ROWS, UG_LD) > T.TWO32 and T.row_start_byte(3835, UG_LD) >= T.TWO32 > T.row_start_byte(3834, UG_LD)
    k, r, r2 = 32, 17, 16
    Xh, Y0, Ch = T.dense_panel(UG_ROWS, k), T.dense_panel(UG_ROWS, r, shift=13), fcol(T.dense_coef(k, r, seed=1))
    Ynew = Y0 - Xh @ Ch
    want_slot = Xh.T @ Ynew[:, :r2]
    bound = UG_ROWS * 16 * (16 + T.dense_partial_bound(1, k))
    with D.context() as ctx, D.tall(ctx, UG_ROWS, UG_LD) as PX, D.tall(ctx, UG_ROWS, UG_LD) as PY, D.tall(ctx, UG_ROWS, UG_LD) as PO:
        lib = ctx.lib
        before = lib.rails_dense_update_gram_pipeline()
        lib.rails_dense_set_update_gram_pipeline(pipeline)
        try:
            chk(ctx, lib.rails_deferred_reserve(ctx.h, 3, (k + 64) * 32), "rails_deferred_reserve")
            for xoff in OFFSETS:
                PX.guarded(xoff, k, fcol(Xh))
                y = PY.guarded(3, r, fcol(Y0))
                o = PO.guarded(3, r)
                o.assign(D.NAN)
                fused0 = ctx.stats().get("update_gram_fused", 0)
                if in_place:
                    rc = lib.rails_update_gram_deferred(ctx.h, -1.0, PX.h, xoff, k, ptr(Ch), k, r, PY.h, 3, r2, 1)
                else:
                    rc = lib.rails_update_gram_deferred_out(ctx.h, -1.0, PX.h, xoff, k, ptr(Ch), k, r, PY.h, 3, PO.h, 3, r2, 1)
                chk(ctx, rc, "rails_update_gram_deferred")
                ctx.sync()
                form = C.c_int(-1)
                assert lib.rails_dense_last_update_gram_form(ctx.h, C.byref(form)) == 0
                fused = ctx.stats().get("update_gram_fused", 0) - fused0
                assert fused == (1 if xoff % 2 == 0 else 0), (xoff, fused)
                if fused:
                    assert form.value == (2 if pipeline else 1), form.value
                slot = np.zeros((k, r2), order="F")
                chk(ctx, lib.rails_deferred_fetch(ctx.h, 1, k * r2, ptr(slot)), "rails_deferred_fetch")
                exact(slot, want_slot, bound, "second projection, X at column %d" % xoff)
                exact((y if in_place else o).to_host(), Ynew, bound, "update, X at column %d" % xoff)
                if not in_place:
                    assert D.same_bits(y.to_host(), Y0)
                assert PX.intact() and PY.intact() and PO.intact()
        finally:
            lib.rails_dense_set_update_gram_pipeline(before)


# ------------------------------------------------------------------------------------------------------------- row forms
@pytest.mark.parametrize("off", OFFSETS)
def test_rowquad_and_rowpair(off):
    for k in (5, 40, 130):
        Uh, Sh = T.dense_panel(M, k), fcol(T.dense_coef(k, k, seed=k))
        bound = k * k * 16 * 8 * 16
        with D.context() as ctx, D.tall(ctx, M, LD) as PU, D.tall(ctx, M, LD) as PO:
            u = PU.guarded(off, k, fcol(Uh))
            o = PO.guarded(3 - off, 1)
            o.assign(D.NAN)
            chk(ctx, ctx.lib.rails_panel_rowquad(ctx.h, PU.h, off, k, ptr(Sh), k, PO.h, 3 - off), "rails_panel_rowquad")
            exact(o.to_host()[:, 0], np.einsum("ij,jl,il->i", Uh, Sh, Uh), bound, "rowquad k = %d" % k)
            assert D.same_bits(o.to_host(), D.MV(ctx, data=Uh).rowquad(Sh).to_host())
            # pairs of rows on both sides of 2^31 and 2^32, into the first rows of the tall output
            g = np.random.default_rng(k)
            ia, ib = g.integers(0, M, 200).astype(np.int32), g.integers(0, M, 200).astype(np.int32)
            ia[:3], ib[:3] = (0, M - 1, T.ROW_PAST_2G), (M - 1, 0, T.ROW_PAST_4G)
            o.assign(D.NAN)
            u.rowpair(Sh, ia, ib, out=o)
            got = o.to_host()[:, 0]
            exact(got[:200], np.einsum("ij,jl,il->i", Uh[ia], Sh, Uh[ib]), bound, "rowpair k = %d" % k)
            assert np.isnan(got[200:]).all() and PU.intact() and PO.intact()
            assert D.same_bits(got[:200], D.MV(ctx, data=Uh).rowpair(Sh, ia, ib).to_host()[:, 0])


# ------------------------------------------------------------------------------------------------------------- row moves
@pytest.mark.parametrize("off", OFFSETS)
def test_move_rows_and_permute_rows(off):
    nc = 33
    Xh = T.dense_panel(M, nc)
    g = np.random.default_rng(2)
    with D.context() as ctx, D.tall(ctx, M, LD) as PX, D.tall(ctx, M, LD) as PY:
        lib = ctx.lib
        PX.guarded(off, nc, fcol(Xh))
        # gather with repeats out of the tall panel into a compact one, and into the first rows of another tall one
        idx = g.integers(0, M, 120).astype(np.int32)
        idx[:4] = (M - 1, 0, T.ROW_PAST_4G, T.ROW_PAST_2G)
        c = D.MV(ctx, m=120, n=nc, capacity=nc)
        chk(ctx, lib.rails_panel_move_rows(ctx.h, PX.h, off, nc, idx.ctypes.data_as(_i32p), idx.size, 0, c.panel.h, 0), "rails_panel_move_rows")
        assert D.same_bits(c.to_host(), Xh[idx])
        # scatter the rows of a compact panel to distinct rows of the tall one; the other rows keep their NaN
        y = PY.guarded(3 - off, nc)
        y.assign(D.NAN)
        rows = np.sort(g.permutation(M)[:120]).astype(np.int32)
        rows[-3:] = (M - 3, M - 2, M - 1)
        assert np.unique(rows).size == 120
        chk(ctx, lib.rails_panel_move_rows(ctx.h, c.panel.h, 0, nc, rows.ctypes.data_as(_i32p), rows.size, 1, PY.h, 3 - off), "rails_panel_move_rows")
        got = y.to_host()
        assert D.same_bits(got[rows], Xh[idx]) and np.isnan(np.delete(got, rows, axis=0)).all()
        # a permutation of all rows between the two tall panels, both directions (device indices)
        perm = g.permutation(M).astype(np.int32)
        dev = C.c_void_p()
        chk(ctx, lib.rails_index_upload(ctx.h, perm.ctypes.data_as(_i32p), perm.size, C.byref(dev)), "rails_index_upload")
        try:
            for scatter in (0, 1):
                y.assign(D.NAN)
                chk(ctx, lib.rails_panel_permute_rows(ctx.h, PX.h, off, nc, dev, scatter, PY.h, 3 - off), "rails_panel_permute_rows")
                want = np.empty_like(Xh)
                if scatter:
                    want[perm] = Xh
                else:
                    want = Xh[perm]
                assert D.same_bits(y.to_host(), want), scatter
        finally:
            lib.rails_index_free(ctx.h, dev)
        assert PX.intact() and PY.intact() and D.same_bits(PX.window(off, nc).to_host(), Xh)


# ------------------------------------------------------------------------------------------------------ sparse right-hand side
def _sparse_b(p, seed):
    """an M x p CSR matrix with 0..6 integer entries per row (distinct columns), rows 0 and M - 1 among the non-empty ones"""
    g = np.random.default_rng(seed)
    counts = g.integers(0, min(p, 6) + 1, M)
    counts[[0, T.ROW_PAST_2G, T.ROW_PAST_4G, M - 1]] = min(p, 3)
    rowptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    col = np.concatenate([np.sort(g.choice(p, size=c, replace=False)) for c in counts]).astype(np.int32)
    val = (g.integers(1, 9, col.size) * g.choice(np.array([-1, 1]), col.size)).astype(np.float64)
    dense = np.zeros((M, p))
    dense[np.repeat(np.arange(M), counts), col] = val
    return rowptr, col, val, dense


@pytest.mark.parametrize("off", OFFSETS)
def test_sparse_rhs_apply_both_directions(off):
    from rails_amd.sparse_rhs import SparseRHS

    p, nc = 9, 17
    rowptr, col, val, Bd = _sparse_b(p, seed=4)
    Xp, Xm = T.dense_panel(p, nc), T.dense_panel(M, nc, shift=3)
    with D.context() as ctx, D.tall(ctx, M, LD) as PA, D.tall(ctx, M, LD) as PB:
        S = SparseRHS(ctx, rowptr, col, val, p)
        try:
            # Y = B X: X of p rows, compact; Y a tall window
            y = PA.guarded(off, nc)
            y.assign(D.NAN)
            S.apply(D.MV(ctx, data=Xp), y)
            exact(y.to_host(), Bd @ Xp, 6 * 8 * 16, "B X")
            # Y = B'X: X a tall window, Y of p rows
            x = PB.guarded(3 - off, nc, fcol(Xm))
            Yt = S.apply(x, trans=True)
            exact(Yt.to_host(), Bd.T @ Xm, M * 8 * 16, "B'X")
            assert D.same_bits(Yt.to_host(), S.apply(D.MV(ctx, data=Xm), trans=True).to_host())
            assert PA.intact() and PB.intact()
        finally:
            S.close()


# ------------------------------------------------------------------------------------------------------ fused residual Lanczos
def _lanczos_plan(ctx):
    nch, unroll, nblocks = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    chk(ctx, ctx.lib.rails_lanczos_last_launch(ctx.h, C.byref(nch), C.byref(unroll), C.byref(nblocks)), "rails_lanczos_last_launch")
    return nch.value, unroll.value, nblocks.value


@pytest.mark.parametrize("sparse_b", (False, True), ids=["dense_B", "sparse_B"])
def test_fused_residual_lanczos(sparse_b):
    """[AV MV B] held in windows (at even columns: the pass asks for them) of three tall panels against the same call on compact panels:
    the same plan, then the same H, step count and Lanczos vectors bit for bit (both runs draw the start vector from the same seed)"""
    from rails_amd.sparse_rhs import SparseRHS, resid_lanczos_sparse
    from rails_amd.wrappers import lanczos_vectors, resid_lanczos

    k, p, L = 24, 6, 8
    g = np.random.default_rng(11)
    V = np.linalg.qr(g.uniform(-1, 1, (M, k)))[0]
    AV = g.uniform(-1, 1, (M, k))
    Tm = g.uniform(-1, 1, (k, k))
    Tm = fcol(Tm + Tm.T)
    rowptr, col, val, Bd = _sparse_b(p, seed=6)

    def run(ctx, av, v, b):
        ctx.set_seed(77)
        out = resid_lanczos_sparse(ctx, av, v, Tm, b, L) if sparse_b else resid_lanczos(ctx, av, v, Tm, b, L)
        plan = _lanczos_plan(ctx)
        Q = D.MV(ctx, m=M, n=out["steps"], capacity=L + 1)
        lanczos_vectors(ctx, np.eye(out["steps"]), Q)
        return plan, out["steps"], out["H"], Q.to_host()

    with D.context() as ctx:
        Bs = SparseRHS(ctx, rowptr, col, val, p) if sparse_b else None
        try:
            want = run(ctx, D.MV(ctx, data=AV), D.MV(ctx, data=V), Bs if sparse_b else D.MV(ctx, data=Bd))
            with D.tall(ctx, M, LD) as PA, D.tall(ctx, M, LD) as PV, D.tall(ctx, M, LD) as PB:
                av, v = PA.guarded(2, k, fcol(AV)), PV.guarded(0, k, fcol(V))
                b = Bs if sparse_b else PB.guarded(4, p, fcol(Bd))
                got = run(ctx, av, v, b)
                assert PA.intact() and PV.intact() and PB.intact()
        finally:
            if Bs is not None:
                Bs.close()
    assert got[0] == want[0], (got[0], want[0])
    assert got[1] == want[1] and got[1] >= 2, (got[1], want[1])
    assert D.same_bits(got[2], want[2]) and D.same_bits(got[3], want[3])
    assert np.abs(got[3].T @ got[3] - np.eye(got[1])).max() <= 1e-10


# ------------------------------------------------------------------------------------------------------------------ solves
@pytest.mark.parametrize("off", OFFSETS)
def test_lu_solve_and_triangular_solve(off):
    """one rails_lu_solve (block-diagonal factors with permutations, both directions) and one rails_sptrsv_solve (in place) with X and Y
    windows of tall panels against the compact solves, bit for bit; that the columns of a solve do not depend on each other is tested
    elsewhere (test_gpu_lu_levels.py)"""
    import scipy.sparse as sp

    import lu_fixtures as LF
    from rails_amd.splu import SparseLU

    nc = 17
    F = LF.block_factors(M // 3, 3, seed=2)
    Bh = T.dense_panel(M, nc)
    with D.context() as ctx, D.tall(ctx, M, LD) as PX, D.tall(ctx, M, LD) as PY:
        lu = SparseLU(ctx, F.A, lu=F)
        try:
            for trans in (False, True):
                x = PX.guarded(off, nc, fcol(Bh))
                y = PY.guarded(3 - off, nc)
                y.assign(D.NAN)
                lu.solve(x, y, trans=trans)
                got = y.to_host()
                want = lu.solve(D.MV(ctx, data=Bh), trans=trans).to_host()
                assert D.same_bits(got, want), trans
                A = sp.csr_matrix(F.A)
                res = (A.T if trans else A) @ got - Bh
                assert np.abs(res).max() <= 1e-10 * np.abs(Bh).max()
                assert PX.intact() and PY.intact() and D.same_bits(x.to_host(), Bh)
        finally:
            lu.close()
        # a lower triangle with its diagonal: banded, dyadic entries
        g = np.random.default_rng(8)
        Tl = sp.tril(sp.random(M, M, density=0.03, random_state=3, data_rvs=lambda n: g.choice(np.array([-0.5, 0.25, 0.5]), n)), k=-1) + sp.diags(g.choice(np.array([1.0, 2.0, -2.0]), M))
        Tl = sp.csr_matrix(Tl)
        Tl.sort_indices()
        rp, ci, va = Tl.indptr.astype(np.int64), Tl.indices.astype(np.int32), Tl.data.astype(np.float64)
        h = C.c_void_p()
        chk(ctx, ctx.lib.rails_sptrsv_create(ctx.h, M, rp.ctypes.data_as(C.POINTER(C.c_int64)), ci.ctypes.data_as(_i32p), ptr(va), 1, 0, C.byref(h)), "rails_sptrsv_create")
        try:
            x = PX.guarded(off, nc, fcol(Bh))
            chk(ctx, ctx.lib.rails_sptrsv_solve(ctx.h, h, PX.h, off, nc), "rails_sptrsv_solve")
            c = D.MV(ctx, data=Bh)
            chk(ctx, ctx.lib.rails_sptrsv_solve(ctx.h, h, c.panel.h, 0, nc), "rails_sptrsv_solve")
            got = x.to_host()
            assert D.same_bits(got, c.to_host()) and PX.intact()
            assert np.abs(Tl @ got - Bh).max() <= 1e-9 * max(1.0, np.abs(got).max())
        finally:
            ctx.lib.rails_sptrsv_destroy(h)
