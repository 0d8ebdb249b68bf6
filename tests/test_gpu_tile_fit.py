"""Tile counts of the dense kernels fitted to the widths a solve runs at (rails_dense_set_tile_fit): the fused
update + second projection with five column blocks per wave, the wide-X Gram with five tiles per wave, the restart rotation with an odd
number of output tiles and without the half chunk that lies past k.  The fitted forms leave out work on zero padding and nothing else,
so every call is made with the switch on and off in one process and the results are compared bit for bit; with the switch on they
are also held against a float64 numpy product within the bounds tests/test_gpu_kernels.py uses for the same entry points, and
rails_dense_last_tiles says which instantiation ran."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DP = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def ctx():
    import rails_amd

    c = rails_amd.Context(device=0, seed=5)
    before = c.lib.rails_dense_tile_fit()
    yield c
    c.lib.rails_dense_set_tile_fit(before)
    c.close()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _last_tiles(ctx):
    nbw, ti, tr = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    assert ctx.lib.rails_dense_last_tiles(ctx.h, C.byref(nbw), C.byref(ti), C.byref(tr)) == 0
    return nbw.value, ti.value, tr.value


def test_setter_is_read_back(ctx):
    lib = ctx.lib
    lib.rails_dense_set_tile_fit(0)
    assert lib.rails_dense_tile_fit() == 0
    lib.rails_dense_set_tile_fit(1)
    assert lib.rails_dense_tile_fit() == 1


# m = 4099: the fused kernel (from 4096 rows on) with a partial row tile; k around the edges of <5, .> (256 < k <= 320) with k % 4 = 1, 0,
# 3, 0, 1, 0; the block right behind the basis in the same panel, with and without its 17th column.
@pytest.mark.parametrize("r,r2", [(17, 16), (16, 16)])
@pytest.mark.parametrize("k", [257, 268, 319, 320, 321, 384])
def test_fused_pass_same_bits_with_five_blocks_per_wave(ctx, k, r, r2):
    import rails_amd

    lib, chk = ctx.lib, rails_amd._lib.check
    m = 4099
    g = np.random.default_rng(100 * k + r)
    Xh = g.uniform(-1, 1, (m, k + r + 2))
    Ch = np.asfortranarray(g.uniform(-1, 1, (k + 3, r)))
    chk(lib.rails_deferred_reserve(ctx.h, 3, (k + 64) * 32), "rails_deferred_reserve")
    out = {}
    for fit in (1, 0):
        lib.rails_dense_set_tile_fit(fit)
        P = rails_amd.HipMultiVectorWrapper(ctx, data=Xh)
        fused0 = ctx.stats().get("update_gram_fused", 0)
        chk(lib.rails_update_gram_deferred(ctx.h, -0.5, P.panel.h, 0, k, Ch.ctypes.data_as(DP), k + 3, r, P.panel.h, k, r2, 1), "rails_update_gram_deferred")
        ctx.sync()
        assert ctx.stats().get("update_gram_fused", 0) - fused0 == 1
        slot = np.zeros((k, r2), order="F")
        chk(lib.rails_deferred_fetch(ctx.h, 1, k * r2, slot.ctypes.data_as(DP)), "rails_deferred_fetch")
        out[fit] = (P.to_host(), slot, _last_tiles(ctx)[0])
    assert out[1][2] == (5 if k <= 320 else 6) and out[0][2] == 6
    assert _same_bits(out[1][0], out[0][0])  # the updated block (and everything around it)
    assert _same_bits(out[1][1], out[0][1])  # the k x r2 slot
    # against numpy, with the bounds of test_update_and_second_projection_in_one_pass
    panel, slot, _ = out[1]
    Xa = Xh[:, :k]
    Ynew = Xh[:, k:k + r] - 0.5 * (Xa @ Ch[:k])
    scale = np.abs(Ynew).max()
    np.testing.assert_allclose(panel[:, k:k + r], Ynew, rtol=0, atol=1e-13 * k * scale)
    assert np.array_equal(panel[:, :k], Xa) and np.array_equal(panel[:, k + r:], Xh[:, k + r:])
    np.testing.assert_allclose(slot, Xa.T @ Ynew[:, :r2], rtol=0, atol=1e-13 * m * scale)


# a = 273, 285, 288 (18 tiles: three waves of six, as before), 289, 304 (19 tiles: the first width of five per wave), 320 (20: the last),
# 321, 336 (21: six per wave as before); b = 16 and the 17th column on the vector unit.  Y is the tail of X, as in the first
# projection [P | X]' X.
@pytest.mark.parametrize("b", [16, 17])
@pytest.mark.parametrize("a", [273, 285, 288, 289, 304, 320, 321, 336])
def test_wide_gram_same_bits_with_five_tiles_per_wave(ctx, a, b):
    import rails_amd

    lib, chk = ctx.lib, rails_amd._lib.check
    m = 4099
    g = np.random.default_rng(100 * a + b)
    Xh = g.uniform(-1, 1, (m, a))
    X = rails_amd.HipMultiVectorWrapper(ctx, data=Xh)
    out = {}
    for fit in (1, 0):
        lib.rails_dense_set_tile_fit(fit)
        G = np.zeros((a, b), order="F")
        chk(lib.rails_gram(ctx.h, X.panel.h, 0, a, X.panel.h, a - b, b, G.ctypes.data_as(DP), a), "rails_gram")
        out[fit] = (G, _last_tiles(ctx)[1])
    assert out[1][1] == (5 if 288 < a <= 320 else 6) and out[0][1] == 6
    assert _same_bits(out[1][0], out[0][0])
    # the bound of test_gram_matches_oracle
    assert np.abs(out[1][0] - Xh.T @ Xh[:, a - b:]).max() <= 1e-14 * m + 1e-13 * np.sqrt(m)


# r: 13, 15 and 17 output tiles (200, 232; 257, 268, 272) and their even neighbours (241: 16; 273, 288: 18); k: the last chunk of 32
# with its second half past k (324, 336, 353, 357, 368, and 352: no partial chunk at all) and not (337).  m = 1003: eight blocks, a partial one.
ROT_K = (324, 336, 337, 352, 353, 357, 368)


@pytest.fixture(scope="module")
def rotation_operands(ctx):
    import rails_amd

    m = 1003
    g = np.random.default_rng(31)
    Xh = g.uniform(-1, 1, (m, max(ROT_K)))
    Qh = np.asfortranarray(g.uniform(-1, 1, (max(ROT_K), 288)))
    Y0 = g.uniform(-1, 1, (m, 288))
    return m, Xh, Qh, Y0, rails_amd.HipMultiVectorWrapper(ctx, data=Xh)


@pytest.mark.parametrize("r,tr_fit,tr_before", [(200, 13, 14), (232, 15, 16), (241, 16, 16), (257, 17, 18), (268, 17, 18), (272, 17, 18), (273, 18, 18), (288, 18, 18)])
def test_rotation_same_bits_with_exact_tile_count(ctx, rotation_operands, r, tr_fit, tr_before):
    import rails_amd

    lib, chk = ctx.lib, rails_amd._lib.check
    m, Xh, Qh, Y0, X = rotation_operands
    Y = rails_amd.HipMultiVectorWrapper(ctx, m=m, n=r, capacity=r)
    for k in ROT_K:
        for alpha, beta in ((1.0, 0.0),) + (((-0.5, 1.0),) if k == 357 else ()):
            out = {}
            for fit in (1, 0):
                lib.rails_dense_set_tile_fit(fit)
                Y.from_host(Y0[:, :r])
                chk(lib.rails_panel_gemm_wide(ctx.h, alpha, X.panel.h, 0, k, Qh.ctypes.data_as(DP), Qh.shape[0], r, beta, Y.panel.h, 0), "rails_panel_gemm_wide")
                out[fit] = (Y.to_host(), _last_tiles(ctx)[2])
            assert out[1][1] == tr_fit and out[0][1] == tr_before, (k, out[1][1], out[0][1])
            assert _same_bits(out[1][0], out[0][0]), (k, beta)
            # the bound of test_panel_gemm_wide_matches_numpy
            want = beta * Y0[:, :r] + alpha * (Xh[:, :k] @ Qh[:k, :r])
            np.testing.assert_allclose(out[1][0], want, rtol=0, atol=1e-13 * k)
