"""The fused update + second projection on its pipelined schedule (k_update_gram_p) against the kernel as it was
(rails_dense_set_update_gram_pipeline 1 / 0).  The new schedule forms the same partial sums and adds them in the same order, so every
call is made with both in one process and compared bit for bit: the updated block, the whole panel around it (NaN columns beside the
block and beyond r, which nothing may read or write) and the k x r2 slot; rails_dense_last_update_gram_form says which kernel ran.
With the new schedule the results are also held against a float64 numpy product within the bounds that
tests/test_gpu_kernels.py::test_update_and_second_projection_in_one_pass uses for the same entry point."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DP = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def ctx():
    import rails_amd

    c = rails_amd.Context(device=0, seed=5)
    before = c.lib.rails_dense_update_gram_pipeline()
    yield c
    c.lib.rails_dense_set_update_gram_pipeline(before)
    c.close()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _form(ctx):
    f = C.c_int(-1)
    assert ctx.lib.rails_dense_last_update_gram_form(ctx.h, C.byref(f)) == 0
    return f.value


def test_setter_is_read_back(ctx):
    lib = ctx.lib
    lib.rails_dense_set_update_gram_pipeline(0)
    assert lib.rails_dense_update_gram_pipeline() == 0
    lib.rails_dense_set_update_gram_pipeline(1)
    assert lib.rails_dense_update_gram_pipeline() == 1


# Row counts, with G = 2 * num_cu workgroups (read from the context): A fewer tiles than workgroups, one tile each (the prefetch of a
# second tile must load nothing that is used); B a partial last tile; C some workgroups get two tiles and most one; D three or four
# tiles per workgroup, an odd count for some; E five each and a last tile of a single row.
def _rows(which, G):
    return {"A": 4096, "B": 4096 + 5, "C": 16 * G + 16 * 3 + 7, "D": 16 * (3 * G + G // 2) + 9, "E": 16 * (5 * G) + 1}[which]


# (rows, k, r, r2, xoff, ld_out, alpha).  k: the edges of every instantiation (NBW = 4: k <= 256, 5: <= 320, 6: <= 384, 8: <= 512) and of
# the four-column load; where k is no multiple of 4 Y sits right behind X in X's panel (the columns between k and k rounded up to 4
# come from Y), where it is one Y is in a panel of its own.  (r, r2): with and without the 17th column, fewer Gram columns than
# update columns, one MFMA column tile partly filled, a single column.  xoff: the X window's (even) first column.  ld_out: 0 the update
# in place, 18 into a compact panel of row stride 18 (the solver's form), 17 an odd row stride.  The last rows are the widths of the
# benchmark's trips in the solver's form at three to five tiles per workgroup.
CASES = [
    ("A", 32, 17, 16, 0, 0, -1.0), ("C", 32, 1, 1, 2, 18, -0.5), ("A", 255, 17, 16, 0, 18, -0.5), ("D", 255, 1, 1, 0, 0, -1.0),
    ("B", 256, 16, 16, 2, 0, -1.0), ("E", 256, 17, 12, 0, 17, -0.5), ("A", 257, 17, 16, 0, 0, -0.5), ("C", 257, 9, 9, 2, 18, -1.0),
    ("B", 318, 17, 12, 0, 17, -1.0), ("D", 318, 5, 3, 0, 0, -0.5), ("A", 320, 17, 16, 2, 18, -1.0), ("E", 320, 9, 9, 0, 0, -0.5),
    ("B", 321, 17, 16, 0, 0, -1.0), ("C", 321, 16, 16, 0, 18, -0.5), ("A", 384, 17, 16, 0, 17, -0.5), ("D", 384, 5, 3, 2, 0, -1.0),
    ("B", 385, 17, 16, 0, 18, -1.0), ("C", 385, 9, 9, 0, 0, -0.5), ("A", 510, 17, 16, 2, 0, -1.0), ("C", 510, 16, 16, 0, 17, -0.5),
    ("B", 512, 17, 12, 0, 18, -0.5), ("C", 512, 1, 1, 0, 0, -1.0),
    ("B", 35, 5, 3, 0, 18, -0.5), ("A", 100, 9, 9, 0, 0, -1.0), ("E", 64, 17, 16, 0, 0, -0.5), ("D", 128, 16, 16, 2, 17, -1.0),
    ("E", 257, 17, 16, 0, 0, -1.0), ("D", 321, 17, 12, 0, 17, -0.5), ("C", 384, 17, 16, 0, 0, -1.0), ("B", 320, 16, 16, 0, 0, -0.5),
    ("A", 448, 17, 16, 0, 0, -1.0), ("E", 384, 17, 16, 2, 18, -0.5), ("A", 318, 17, 16, 2, 0, -1.0), ("D", 512, 17, 16, 0, 18, -1.0),
    ("E", 240, 17, 16, 0, 18, -1.0), ("C", 274, 17, 16, 0, 18, -1.0), ("D", 289, 17, 16, 0, 18, -1.0), ("D", 316, 9, 9, 0, 0, -1.0),
    ("D", 340, 17, 16, 0, 18, -1.0), ("E", 345, 9, 9, 0, 18, -1.0),
]


@pytest.mark.parametrize("rows,k,r,r2,xoff,ld_out,alpha", CASES)
def test_same_bits_as_the_kernel_before_and_close_to_numpy(ctx, rows, k, r, r2, xoff, ld_out, alpha):
    import rails_amd

    lib, chk = ctx.lib, rails_amd._lib.check
    G = 2 * lib.rails_ctx_num_cu(ctx.h)
    assert G > 0
    m = _rows(rows, G)
    behind = k % 4 != 0
    assert xoff % 2 == 0 and (not behind or r >= ((k + 3) & ~3) - k)
    g = np.random.default_rng(1000 * k + 10 * r + len(rows) + m)
    # X's panel: [xoff columns of NaN | X | (Y | 2 columns of NaN, where Y is behind X) or (3 columns of NaN)]
    Xa = g.uniform(-1, 1, (m, k))
    Ya = g.uniform(-1, 1, (m, r))
    nanc = lambda n: np.full((m, n), np.nan)
    if behind:
        Xpanel, Ypanel, yc0 = np.hstack([nanc(xoff), Xa, Ya, nanc(2)]), None, xoff + k
    else:
        Xpanel, Ypanel, yc0 = np.hstack([nanc(xoff), Xa, nanc(3)]), np.hstack([nanc(2), Ya, nanc(3)]), 2
    Ch = np.asfortranarray(g.uniform(-1, 1, (k + 3, r)))
    chk(lib.rails_deferred_reserve(ctx.h, 3, (k + 64) * 32), "rails_deferred_reserve")
    out = {}
    for pipeline in (1, 0):
        lib.rails_dense_set_update_gram_pipeline(pipeline)
        PX = rails_amd.HipMultiVectorWrapper(ctx, data=Xpanel)
        PY = PX if behind else rails_amd.HipMultiVectorWrapper(ctx, data=Ypanel)
        S = None
        if ld_out:
            S = C.c_void_p()
            chk(lib.rails_panel_create_ld(ctx.h, m, ld_out, ld_out, C.byref(S)), "rails_panel_create_ld")
            assert lib.rails_panel_ld(S) == ld_out
            chk(lib.rails_panel_fill(ctx.h, S, 0, ld_out, float("nan")), "rails_panel_fill")
        try:
            fused0 = ctx.stats().get("update_gram_fused", 0)
            if S is None:
                chk(lib.rails_update_gram_deferred(ctx.h, alpha, PX.panel.h, xoff, k, Ch.ctypes.data_as(DP), k + 3, r, PY.panel.h, yc0, r2, 1), "rails_update_gram_deferred")
            else:
                chk(lib.rails_update_gram_deferred_out(ctx.h, alpha, PX.panel.h, xoff, k, Ch.ctypes.data_as(DP), k + 3, r, PY.panel.h, yc0, S, 0, r2, 1),
                    "rails_update_gram_deferred_out")
            ctx.sync()
            assert ctx.stats().get("update_gram_fused", 0) - fused0 == 1
            slot = np.zeros((k, r2), order="F")
            chk(lib.rails_deferred_fetch(ctx.h, 1, k * r2, slot.ctypes.data_as(DP)), "rails_deferred_fetch")
            spanel = None
            if S is not None:
                spanel = np.zeros((m, ld_out), order="F")
                chk(lib.rails_panel_download(ctx.h, S, 0, ld_out, spanel.ctypes.data_as(DP), m), "rails_panel_download")
            out[pipeline] = (PX.to_host(), PY.to_host(), spanel, slot, _form(ctx))
        finally:
            if S is not None:
                lib.rails_panel_destroy(S)
    assert out[1][4] == 2 and out[0][4] == 1  # the pipelined kernel, the kernel before
    for a, b in zip(out[1][:4], out[0][:4]):
        assert (a is None and b is None) or _same_bits(a, b)
    # against numpy, with the bounds of test_update_and_second_projection_in_one_pass; everything around the block as it was
    xp, yp, sp, slot, _ = out[1]
    Ynew = Ya + alpha * (Xa @ Ch[:k])
    scale = np.abs(Ynew).max()
    if sp is None:
        got = yp[:, yc0:yc0 + r]
        want_y = (Xpanel if behind else Ypanel).copy()
        want_y[:, yc0:yc0 + r] = got
        assert _same_bits(yp, want_y)
        if not behind:
            assert _same_bits(xp, Xpanel)
    else:
        got = sp[:, :r]
        assert np.all(np.isnan(sp[:, r:]))
        assert _same_bits(xp, Xpanel) and (behind or _same_bits(yp, Ypanel))  # the input Y stays
    np.testing.assert_allclose(got, Ynew, rtol=0, atol=1e-13 * k * scale)
    np.testing.assert_allclose(slot, Xa.T @ Ynew[:, :r2], rtol=0, atol=1e-13 * m * scale)


def test_solve_same_bits_with_either_schedule():
    """One small solve on the coordinate-space back end with the overlapped orthogonalisation at work (the banded pattern of
    tests/test_gpu_block_scratch.py, 20000 rows so that every block with 32 basis columns or more takes the one-pass kernel): T, V and
    the residual history bit for bit with the schedule switched."""
    import rails_amd
    from rails_amd import problems as P

    m = 20000
    A = P.banded_random(m, nnz_row=9, bandwidth=64, seed=3)
    B = P.rhs(m, 4, seed=5)
    params = {"Restart size": 40, "Reduced size": 24, "Expand size": 4, "Lanczos iterations": 8, "Tolerance": 1e-30, "Maximum iterations": 100000}
    lib = rails_amd.load()
    before = lib.rails_dense_update_gram_pipeline()
    runs = {}
    try:
        for pipeline in (1, 0):
            lib.rails_dense_set_update_gram_pipeline(pipeline)
            c = rails_amd.Context(device=0, seed=1)
            c.set_seed(9, 0)
            op = rails_amd.HipOperatorWrapper(c, *A)
            s = rails_amd.Solver(c, op, B)
            assert s.set_parameters(params) == 0
            s.set_option("verbose", 0)
            s.set_option("subspace", 1)
            s.set_option("max_trips", 25)
            code, V, T = s.solve()
            runs[pipeline] = (code, s.trips(), np.array(s.history()), V, T, s.backend_stats(), c.stats().get("update_gram_fused", 0), _form(c))
            s.close()
            c.close()
    finally:
        lib.rails_dense_set_update_gram_pipeline(before)
    (c1, t1, h1, V1, T1, st1, f1, form1), (c0, t0, h0, V0, T0, st0, f0, form0) = runs[1], runs[0]
    assert t0 == t1 == 25 and c0 == c1
    assert st1["overlapped_blocks"] > 0 and st1["second_rounds"] > 0 and f1 > 0 and f0 == f1
    assert form1 == 2 and form0 == 1
    assert _same_bits(h1, h0) and _same_bits(V1, V0) and _same_bits(T1, T0)
