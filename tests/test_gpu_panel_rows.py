"""rails_panel_move_rows (k_move_rows, solution.hip: host indices, panels of different row counts) and rails_panel_permute_rows
(k_gather_rows, sptrsv.hip: device indices, one row count) against numpy fancy indexing, bit for bit: the data holds -0.0, +-inf, NaNs with
distinct payloads and subnormals and is compared as uint64.  Shapes put n * nc at 1, 255, 256, 257 (one block of 256 threads, either side)
and at a few thousand; windows start at columns 0, 1 and 5 of wider panels whose other entries must keep their sentinel; every refusal
must leave the target panel's bytes as they were."""
import ctypes as C

import numpy as np
import pytest

import solution_reference as R

pytestmark = pytest.mark.gpu

_i32p = C.POINTER(C.c_int32)
SHAPES = [(1, 1), (17, 15), (16, 16), (257, 1), (1000, 33)]  # n * nc = 1, 255, 256, 257, 33000
OFFSETS = [(0, 0), (1, 5), (5, 0), (5, 1)]
SENTINEL = -7.25


@pytest.fixture(scope="module")
def ctx():
    import rails_amd

    c = rails_amd.Context(device=0, seed=1)
    yield c
    c.close()


def MV(ctx, data):
    import rails_amd

    return rails_amd.HipMultiVectorWrapper(ctx, data=data)


def _move(ctx, Xd, xc0, nc, idx, scatter, Yd, yc0, n=None):
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    return ctx.lib.rails_panel_move_rows(ctx.h, Xd.panel.h, xc0, nc, idx.ctypes.data_as(_i32p), idx.size if n is None else n, scatter, Yd.panel.h, yc0)


class _Index:
    """indices in device memory (rails_index_upload)"""

    def __init__(self, ctx, idx):
        self.ctx, self.h = ctx, C.c_void_p()
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        assert ctx.lib.rails_index_upload(ctx.h, idx.ctypes.data_as(_i32p), idx.size, C.byref(self.h)) == 0

    def free(self):
        self.ctx.lib.rails_index_free(self.ctx.h, self.h)


def _wide(g, m, c0, nc):
    """special data in columns [c0, c0 + nc) of an m x (c0 + nc + 2) array of sentinels"""
    A = np.full((m, c0 + nc + 2), SENTINEL, order="F")
    A[:, c0:c0 + nc] = R.special_data(g, m, nc)
    return A


def _same(a, b):
    return np.array_equal(R.bits(a), R.bits(b))


@pytest.mark.parametrize("n,nc", SHAPES)
def test_move_rows_gather_and_scatter(ctx, n, nc):
    g = np.random.default_rng(100 * n + nc)
    for xc0, yc0 in OFFSETS:
        # gather: n rows, with repeats, out of a panel of n + 9 rows into a panel of n + 2 rows; its last two rows keep the sentinel
        X = _wide(g, n + 9, xc0, nc)
        idx = g.integers(0, n + 9, n)
        idx[0], idx[-1] = n + 8, (0 if n > 1 else n + 8)
        Xd, Yd = MV(ctx, X), MV(ctx, np.full((n + 2, yc0 + nc + 3), SENTINEL))
        assert _move(ctx, Xd, xc0, nc, idx, 0, Yd, yc0) == 0
        want = np.full((n + 2, yc0 + nc + 3), SENTINEL)
        want[:n, yc0:yc0 + nc] = X[idx, xc0:xc0 + nc]
        assert _same(Yd.to_host(), want), (n, nc, xc0, yc0)
        assert _same(Xd.to_host(), X)
        # scatter: the n rows of a panel to distinct rows of a panel of 2 n + 3 rows; the other rows and columns keep the sentinel
        X = _wide(g, n, xc0, nc)
        idx = g.permutation(2 * n + 3)[:n]
        if 2 * n + 2 not in idx:
            idx[0] = 2 * n + 2  # the last row is among them
        assert np.unique(idx).size == n
        Xd, Yd = MV(ctx, X), MV(ctx, np.full((2 * n + 3, yc0 + nc + 3), SENTINEL))
        assert _move(ctx, Xd, xc0, nc, idx, 1, Yd, yc0) == 0
        want = np.full((2 * n + 3, yc0 + nc + 3), SENTINEL)
        want[idx, yc0:yc0 + nc] = X[:, xc0:xc0 + nc]
        assert _same(Yd.to_host(), want), (n, nc, xc0, yc0)


def test_move_rows_from_a_tall_panel_into_seven_rows(ctx):
    g = np.random.default_rng(3)
    X = _wide(g, 1000, 1, 33)
    Xd = MV(ctx, X)
    for idx in ([999, 0, 500, 500, 999, 1, 500], [0, 0, 0], [999]):
        Yd = MV(ctx, np.full((7, 40), SENTINEL))
        assert _move(ctx, Xd, 1, 33, idx, 0, Yd, 5) == 0
        want = np.full((7, 40), SENTINEL)
        want[:len(idx), 5:38] = X[idx, 1:34]
        assert _same(Yd.to_host(), want), idx


def test_move_rows_nothing_to_move(ctx):
    g = np.random.default_rng(4)
    X, Y = _wide(g, 20, 1, 6), _wide(g, 9, 0, 8)
    Xd, Yd = MV(ctx, X), MV(ctx, Y)
    none = np.zeros(0, dtype=np.int32)
    for scatter in (0, 1):
        assert ctx.lib.rails_panel_move_rows(ctx.h, Xd.panel.h, 1, 6, None, 0, scatter, Yd.panel.h, 0) == 0  # n = 0, no index array at all
        assert _move(ctx, Xd, 1, 6, none, scatter, Yd, 0) == 0
        assert _move(ctx, Xd, 1, 0, [3, 4], scatter, Yd, 2) == 0  # nc = 0
        assert _move(ctx, Xd, 9, 0, [3, 4], scatter, Yd, 10) == 0  # an empty window at the very end of both capacities
    assert _same(Yd.to_host(), Y) and _same(Xd.to_host(), X)


@pytest.mark.parametrize("n,nc", SHAPES)
def test_permute_rows_both_directions(ctx, n, nc):
    g = np.random.default_rng(200 * n + nc)
    perm = g.permutation(n)
    P = _Index(ctx, perm)
    for xc0, yc0 in OFFSETS:
        X = _wide(g, n, xc0, nc)
        Xd = MV(ctx, X)
        Gd, Sd, Bd = (MV(ctx, np.full((n, yc0 + nc + 3), SENTINEL)) for _ in range(3))
        want = np.full((n, yc0 + nc + 3), SENTINEL)
        assert ctx.lib.rails_panel_permute_rows(ctx.h, Xd.panel.h, xc0, nc, P.h, 0, Gd.panel.h, yc0) == 0  # gather: row i <- row perm[i]
        want[:, yc0:yc0 + nc] = X[perm, xc0:xc0 + nc]
        assert _same(Gd.to_host(), want), (n, nc, xc0, yc0)
        assert ctx.lib.rails_panel_permute_rows(ctx.h, Xd.panel.h, xc0, nc, P.h, 1, Sd.panel.h, yc0) == 0  # scatter: row perm[i] <- row i
        want[perm, yc0:yc0 + nc] = X[:, xc0:xc0 + nc]
        assert _same(Sd.to_host(), want), (n, nc, xc0, yc0)
        # scatter, then gather with the same permutation: the identity
        assert ctx.lib.rails_panel_permute_rows(ctx.h, Sd.panel.h, yc0, nc, P.h, 0, Bd.panel.h, yc0) == 0
        want[:, yc0:yc0 + nc] = X[:, xc0:xc0 + nc]
        assert _same(Bd.to_host(), want), (n, nc, xc0, yc0)
        assert _same(Xd.to_host(), X)
    P.free()


def test_refusals_leave_the_target_alone(ctx):
    import rails_amd

    g = np.random.default_rng(5)
    X, Y, T = _wide(g, 20, 1, 6), _wide(g, 9, 0, 8), _wide(g, 20, 0, 8)  # capacities 9, 10, 10
    Xd, Yd, Td = MV(ctx, X), MV(ctx, Y), MV(ctx, T)
    for scatter, idx, why in ((0, [3, -1, 4], "index -1"), (0, [3, 20, 4], "index = rows of the source"), (0, [19] * 10, "10 indices for a target of 9 rows"),
                              (1, [3, -1, 4], "index -1"), (1, [3, 9, 4], "index = rows of the target"), (1, list(range(9)) * 3, "27 indices for a source of 20 rows")):
        assert _move(ctx, Xd, 1, 6, idx, scatter, Yd, 0) != 0, why
        assert rails_amd.load().rails_last_error() != b""
    for scatter in (0, 1):
        assert _move(ctx, Xd, 1, 6, [1, 2], scatter, Xd, 1) != 0  # source and target the same panel
        assert _move(ctx, Xd, 4, 6, [1, 2], scatter, Yd, 0) != 0  # [4, 10) leaves the source's capacity 9
        assert _move(ctx, Xd, 1, 6, [1, 2], scatter, Yd, 5) != 0  # [5, 11) leaves the target's capacity 10
        assert _move(ctx, Xd, -1, 2, [1, 2], scatter, Yd, 0) != 0 and _move(ctx, Xd, 0, 2, [1, 2], scatter, Yd, -1) != 0
        assert _move(ctx, Xd, 0, -1, [1, 2], scatter, Yd, 0) != 0 and _move(ctx, Xd, 0, 2, [1, 2], scatter, Yd, 0, n=-1) != 0
    P = _Index(ctx, g.permutation(20))
    for scatter in (0, 1):
        assert ctx.lib.rails_panel_permute_rows(ctx.h, Xd.panel.h, 1, 6, P.h, scatter, Yd.panel.h, 0) != 0  # 20 rows against 9
        assert ctx.lib.rails_panel_permute_rows(ctx.h, Xd.panel.h, 1, 6, P.h, scatter, Xd.panel.h, 1) != 0  # in place
        assert ctx.lib.rails_panel_permute_rows(ctx.h, Xd.panel.h, 4, 6, P.h, scatter, Td.panel.h, 0) != 0  # windows outside the capacities
        assert ctx.lib.rails_panel_permute_rows(ctx.h, Xd.panel.h, 1, 6, P.h, scatter, Td.panel.h, 5) != 0
        assert ctx.lib.rails_panel_permute_rows(ctx.h, Xd.panel.h, 1, 6, None, scatter, Td.panel.h, 0) != 0  # no indices
    P.free()
    assert _same(Yd.to_host(), Y) and _same(Td.to_host(), T) and _same(Xd.to_host(), X)
    # ... and the panels still work
    assert _move(ctx, Xd, 1, 6, [19, 0], 0, Yd, 2) == 0
    Y[:2, 2:8] = X[[19, 0], 1:7]
    assert _same(Yd.to_host(), Y)
