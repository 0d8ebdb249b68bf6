"""The panel primitives of ctx.hip -- upload, download, copy, fill, scale, axpy, random, reserve and the buffer recycling of
rails_panel_create_ld -- each checked alone.  Every other GPU test reads and writes the device through upload and download, so here the
device memory is reached a second way: torch wraps the panel's raw m x ld buffer (rails_amd.partition.wrap_buffer on
rails_panel_device_ptr, after ctx.sync(); torch.cuda.synchronize() after torch writes).  An upload is read back through torch and a
download returns what torch wrote, so the two transposes cannot err symmetrically.  Data holds -0.0, +-inf, NaN payloads and subnormals and
is compared as uint64.

The BLAS-1 kernels round once per element, so they must equal numpy bit for bit.  For axpy that needs alpha * x to be exact (the device
may fuse the multiply and the add, numpy does not): alpha = +-1, or alpha and x both float32 values (24-bit significands, a 48-bit product)."""
import ctypes as C

import numpy as np
import pytest

import solution_reference as R

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
_dp = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def ctx():
    import rails_amd

    c = rails_amd.Context(device=0, seed=1)
    yield c
    c.close()


class Panel:
    """a panel made with the C calls directly, and its raw buffer through torch"""

    def __init__(self, ctx, m, cap, ld=None):
        self.ctx, self.lib, self.h, self.m = ctx, ctx.lib, C.c_void_p(), m
        if ld is None:
            assert self.lib.rails_panel_create(ctx.h, m, cap, C.byref(self.h)) == 0
        else:
            assert self.lib.rails_panel_create_ld(ctx.h, m, cap, ld, C.byref(self.h)) == 0

    ld = property(lambda self: self.lib.rails_panel_ld(self.h))
    cap = property(lambda self: self.lib.rails_panel_capacity(self.h))
    ptr = property(lambda self: self.lib.rails_panel_device_ptr(self.h))

    def _tensor(self):
        import torch
        from rails_amd.partition import wrap_buffer

        return wrap_buffer(self.ptr, self.m * self.ld, True).view(torch.int64)

    def raw(self):
        """the m x ld doubles of the buffer, padding included"""
        self.ctx.sync()
        return self._tensor().cpu().numpy().view(np.float64).reshape(self.m, self.ld)

    def set_raw(self, A):
        import torch

        assert A.shape == (self.m, self.ld)
        self.ctx.sync()
        self._tensor().copy_(torch.from_numpy(np.ascontiguousarray(A).view(np.int64).ravel()))
        torch.cuda.synchronize()

    def upload(self, c0, H, ldh=None):
        H = np.asfortranarray(H)
        return self.lib.rails_panel_upload(self.ctx.h, self.h, c0, H.shape[1], H.ctypes.data_as(_dp), H.shape[0] if ldh is None else ldh)

    def download(self, c0, H, ldh=None):
        assert H.flags.f_contiguous
        return self.lib.rails_panel_download(self.ctx.h, self.h, c0, H.shape[1], H.ctypes.data_as(_dp), H.shape[0] if ldh is None else ldh)

    def fill(self, c0, nc, v):
        assert self.lib.rails_panel_fill(self.ctx.h, self.h, c0, nc, v) == 0

    def destroy(self):
        assert self.lib.rails_panel_destroy(self.h) == 0
        self.h = None


def _same(a, b):
    return a.shape == b.shape and np.array_equal(R.bits(a), R.bits(b))


def _raw_with(ctx, A, cap=None):
    """a panel whose first columns hold A (through torch), sentinels up to `cap`, zeros in the padding; and that m x ld array"""
    m, n = A.shape
    P = Panel(ctx, m, cap or n)
    full = np.zeros((m, P.ld))
    full[:, :P.cap] = SENTINEL
    full[:, :n] = A
    P.set_raw(full)
    return P, full


M_LIST = [1, 31, 32, 33, 257]
NC_LIST = [1, 31, 32, 33, 64, 65, 100]  # the 32-column chunk of the transfers and the 32 x 32 tile of the transposes, either side
C0_LIST = [0, 1, 7]


@pytest.mark.parametrize("m", M_LIST)
def test_upload_alone(ctx, m):
    g = np.random.default_rng(m)
    for nc in NC_LIST:
        for c0 in C0_LIST:
            for extra in (0, 3):  # ldh = m and ldh = m + 3
                P = Panel(ctx, m, c0 + nc + 2)
                P.fill(0, P.cap, SENTINEL)
                H = R.special_data(g, m + extra, nc)
                assert P.upload(c0, H) == 0
                want = np.zeros((m, P.ld))
                want[:, :P.cap] = SENTINEL
                want[:, c0:c0 + nc] = H[:m]
                assert _same(P.raw(), want), (m, nc, c0, extra)
                P.destroy()


@pytest.mark.parametrize("m", M_LIST)
def test_download_alone(ctx, m):
    g = np.random.default_rng(50 + m)
    for nc in NC_LIST:
        for c0 in C0_LIST:
            P = Panel(ctx, m, c0 + nc + 2)
            A = np.ascontiguousarray(R.special_data(g, m, P.ld))  # the whole buffer, padding included
            P.set_raw(A)
            for extra in (0, 3):
                H = np.full((m + extra, nc), SENTINEL, order="F")
                assert P.download(c0, H) == 0
                assert _same(H[:m], A[:, c0:c0 + nc]), (m, nc, c0, extra)
                assert np.all(H[m:] == SENTINEL)  # the host rows past m are not written
            assert _same(P.raw(), A)
            P.destroy()


def test_short_host_leading_dimension_and_bad_windows_are_refused(ctx):
    g = np.random.default_rng(6)
    A = R.special_data(g, 33, 10)
    P, full = _raw_with(ctx, A)
    H = np.full((33, 4), SENTINEL, order="F")
    assert P.upload(2, H, ldh=32) != 0 and P.download(2, H, ldh=32) != 0  # ldh < m
    assert P.upload(7, H) != 0 and P.download(7, H) != 0  # [7, 11) leaves the capacity 10
    assert P.upload(-1, H) != 0 and P.download(-1, H) != 0
    assert np.all(H == SENTINEL) and _same(P.raw(), full)
    P.destroy()


BLAS1_WINDOWS = [(1, 0, 3), (33, 1, 6), (32, 5, 0), (16, 2, 2)]  # (nc, xc0, yc0)


def _blas1_panels(ctx, g, m, nc, xc0, yc0, special):
    make = (lambda r, c: R.special_data(g, r, c)) if special else (lambda r, c: g.standard_normal((r, c)))
    X, Y = make(m, xc0 + nc + 2), make(m, yc0 + nc + 3)
    Xp, Xfull = _raw_with(ctx, X)
    Yp, Yfull = _raw_with(ctx, Y)
    return X, Y, Xp, Xfull, Yp, Yfull


@pytest.mark.parametrize("nc,xc0,yc0", BLAS1_WINDOWS)
def test_blas1_on_windows_is_exact(ctx, nc, xc0, yc0):
    lib, m = ctx.lib, 257
    g = np.random.default_rng(10 * nc + xc0)
    # copy: bits, specials included
    X, Y, Xp, Xfull, Yp, Yfull = _blas1_panels(ctx, g, m, nc, xc0, yc0, True)
    assert lib.rails_panel_copy(ctx.h, Xp.h, xc0, nc, Yp.h, yc0) == 0
    Yfull[:, yc0:yc0 + nc] = X[:, xc0:xc0 + nc]
    assert _same(Yp.raw(), Yfull) and _same(Xp.raw(), Xfull)
    # fill
    for v in (-0.0, 3.5, float("inf")):
        Yp.fill(yc0, nc, v)
        Yfull[:, yc0:yc0 + nc] = v
        assert _same(Yp.raw(), Yfull), v
    Xp.destroy()
    Yp.destroy()
    # scale and axpy: one rounding per element
    X, Y, Xp, Xfull, Yp, Yfull = _blas1_panels(ctx, g, m, nc, xc0, yc0, False)
    for s in (2.5, 1.0 / 13.0, -3.0):
        assert lib.rails_panel_scale(ctx.h, Yp.h, yc0, nc, s) == 0
        Yfull[:, yc0:yc0 + nc] = Yfull[:, yc0:yc0 + nc] * s
        assert _same(Yp.raw(), Yfull), s
    for alpha in (1.0, -1.0):
        assert lib.rails_panel_axpy(ctx.h, alpha, Xp.h, xc0, nc, Yp.h, yc0) == 0
        Yfull[:, yc0:yc0 + nc] = Yfull[:, yc0:yc0 + nc] + alpha * X[:, xc0:xc0 + nc]
        assert _same(Yp.raw(), Yfull), alpha
    Xp.destroy()
    X32 = X.astype(np.float32).astype(np.float64)
    Xp, Xfull = _raw_with(ctx, X32)
    for alpha in (float(np.float32(1.0 / 3.0)), float(np.float32(-2.7))):
        assert lib.rails_panel_axpy(ctx.h, alpha, Xp.h, xc0, nc, Yp.h, yc0) == 0
        prod = alpha * X32[:, xc0:xc0 + nc]
        assert np.array_equal(np.asarray(prod, dtype=np.longdouble), np.longdouble(alpha) * X32[:, xc0:xc0 + nc].astype(np.longdouble))  # exact
        Yfull[:, yc0:yc0 + nc] = Yfull[:, yc0:yc0 + nc] + prod
        assert _same(Yp.raw(), Yfull), alpha
    assert _same(Xp.raw(), Xfull)
    Xp.destroy()
    Yp.destroy()


def test_copy_within_one_panel(ctx):
    g = np.random.default_rng(12)
    A = R.special_data(g, 33, 20)
    P, full = _raw_with(ctx, A)
    lib = ctx.lib
    for xc0, nc, yc0 in ((0, 6, 5), (5, 6, 0), (3, 10, 10), (12, 8, 5)):
        assert lib.rails_panel_copy(ctx.h, P.h, xc0, nc, P.h, yc0) != 0, (xc0, nc, yc0)  # overlapping windows
    assert lib.rails_panel_copy(ctx.h, P.h, 0, 6, P.h, 15) != 0  # [15, 21) leaves the capacity
    assert lib.rails_panel_copy(ctx.h, P.h, 4, 6, P.h, 4) == 0  # onto itself: nothing to do
    assert _same(P.raw(), full)
    assert lib.rails_panel_copy(ctx.h, P.h, 1, 7, P.h, 8) == 0  # disjoint windows of one panel
    full[:, 8:15] = full[:, 1:8]
    assert _same(P.raw(), full)
    Q = Panel(ctx, 32, 20)
    assert lib.rails_panel_copy(ctx.h, P.h, 0, 6, Q.h, 0) != 0 and lib.rails_panel_axpy(ctx.h, 1.0, P.h, 0, 6, Q.h, 0) != 0  # row mismatch
    Q.destroy()
    P.destroy()


def test_grid_stride_loops(ctx, oracle):
    """more elements than the grid cap num_cu * 8 blocks of 256 threads: every thread of copy, fill, scale, axpy and random goes round its
    grid-stride loop more than once"""
    lib = ctx.lib
    num_cu = lib.rails_ctx_num_cu(ctx.h)
    assert num_cu > 0
    nc, xc0, yc0 = 16, 3, 1
    m = (num_cu * 8 * 256) // nc + 777
    assert m * nc > num_cu * 8 * 256 and m * 32 * 8 < 16 << 20  # (33545 rows on 256 CUs: a padded panel of 8.6 MB)
    g = np.random.default_rng(13)
    X, Y = g.standard_normal((m, xc0 + nc + 1)), g.standard_normal((m, yc0 + nc + 2))
    Xp, Xfull = _raw_with(ctx, X)
    Yp, Yfull = _raw_with(ctx, Y)
    assert lib.rails_panel_copy(ctx.h, Xp.h, xc0, nc, Yp.h, yc0) == 0
    Yfull[:, yc0:yc0 + nc] = X[:, xc0:xc0 + nc]
    assert _same(Yp.raw(), Yfull)
    assert lib.rails_panel_scale(ctx.h, Yp.h, yc0, nc, 1.0 / 13.0) == 0
    Yfull[:, yc0:yc0 + nc] = Yfull[:, yc0:yc0 + nc] * (1.0 / 13.0)
    assert _same(Yp.raw(), Yfull)
    assert lib.rails_panel_axpy(ctx.h, -1.0, Xp.h, xc0, nc, Yp.h, yc0) == 0
    Yfull[:, yc0:yc0 + nc] = Yfull[:, yc0:yc0 + nc] - X[:, xc0:xc0 + nc]
    assert _same(Yp.raw(), Yfull)
    Yp.fill(yc0, nc, 3.5)
    Yfull[:, yc0:yc0 + nc] = 3.5
    assert _same(Yp.raw(), Yfull)
    ctx.set_seed(99, 5)
    assert lib.rails_panel_random(ctx.h, Yp.h, yc0, nc) == 0
    Yfull[:, yc0:yc0 + nc] = oracle.random(m, nc, mode=1, seed=99, stream=5)
    assert _same(Yp.raw(), Yfull) and _same(Xp.raw(), Xfull)
    Xp.destroy()
    Yp.destroy()


def test_reserve_keeps_every_column(ctx):
    g = np.random.default_rng(14)
    m = 257
    A = R.special_data(g, m, 17)
    P = Panel(ctx, m, 17)
    assert P.upload(0, A) == 0 and P.ld == 32
    ptr = P.ptr
    assert ctx.lib.rails_panel_reserve(ctx.h, P.h, 30) == 0
    assert (P.cap, P.ld) == (30, 32) and P.ptr == ptr  # growth inside the leading dimension does not move the buffer
    want = np.zeros((m, 32))
    want[:, :17] = A
    assert _same(P.raw(), want)
    assert ctx.lib.rails_panel_reserve(ctx.h, P.h, 12) == 0 and P.cap == 30  # never shrinks
    assert ctx.lib.rails_panel_reserve(ctx.h, P.h, 60) == 0
    assert (P.cap, P.ld, P.m) == (60, 64, m)
    want = np.zeros((m, 64))
    want[:, :17] = A
    assert _same(P.raw(), want)  # all 17 old columns bit for bit, the new columns and the padding zero
    H = np.full((m, 60), SENTINEL, order="F")
    assert P.download(0, H) == 0 and _same(H, want[:, :60])
    P.destroy()


@pytest.mark.parametrize("m,cap,ld", [(257, 17, None), (100, 5, 5), (1, 1, None)])
def test_a_recycled_buffer_is_zeroed(m, cap, ld):
    """"padding columns are read by vectorised kernels: keep them finite" (rails_panel_create_ld): a destroyed panel's buffer, full of NaN,
    padding included, is handed to the next panel of the same size and must be all zeros there"""
    import rails_amd

    fresh = rails_amd.Context(device=0, seed=1)
    P = Panel(fresh, m, cap, ld)
    ptr, pld = P.ptr, P.ld
    assert np.all(R.bits(P.raw()) == 0)
    P.set_raw(np.full((m, pld), np.nan))
    assert np.isnan(P.raw()).all()
    P.destroy()
    Q = Panel(fresh, m, cap, ld)
    assert Q.ptr == ptr  # the same buffer: the test cannot pass on a fresh allocation
    assert Q.ld == pld and np.all(R.bits(Q.raw()) == 0)
    Q.destroy()
    fresh.close()
