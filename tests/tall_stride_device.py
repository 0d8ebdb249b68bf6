"""Tall panels for the device tests of windows that cross 2 GiB and 4 GiB (test_gpu_tall_stride_*.py; the shapes: tall_stride_cases.py).
Not a test module.

A TallPanel is made by rails_panel_create_ld with rows `ld` doubles apart and is destroyed by the test that made it: panels over 2 GiB are
not kept in the context's re-use list, so destroy frees the memory.  Only windows are ever touched: window() is a HipMultiVectorWrapper
over a few columns; guarded() first fills the GUARD columns on either side of it with NaN through views of their own, and intact() says
afterwards whether they still hold nothing else."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import tall_stride_cases as T

RAILS_ENOMEM = -3
NAN = float("nan")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@contextlib.contextmanager
def context(seed=1):
    import rails_amd

    ctx = rails_amd.Context(device=0, seed=seed)
    try:
        yield ctx
    finally:
        ctx.close()


def MV(ctx, **kw):
    import rails_amd

    return rails_amd.HipMultiVectorWrapper(ctx, **kw)


class TallPanel:
    def __init__(self, ctx, m, ld, cap=T.CAP):
        from rails_amd._lib import check

        self.ctx, self.m, self.ld, self.cap, self.h = ctx, int(m), int(ld), int(cap), C.c_void_p()
        self.guards = []
        rc = ctx.lib.rails_panel_create_ld(ctx.h, self.m, self.cap, self.ld, C.byref(self.h))
        if rc == RAILS_ENOMEM:
            self.h = None
            pytest.skip("no device memory for a panel of %d rows x %d doubles (%.2f GB)" % (m, ld, T.panel_bytes(m, ld) / 1e9))
        check(rc, "rails_panel_create_ld")
        assert ctx.lib.rails_panel_ld(self.h) == self.ld and ctx.lib.rails_panel_rows(self.h) == self.m

    def window(self, c0, nc):
        import rails_amd

        assert 0 <= c0 and c0 + nc <= self.cap
        return rails_amd.HipMultiVectorWrapper._borrow(self.ctx, self.h, c0, nc, self.m)

    def guarded(self, c0, nc, data=None):
        """the window [c0, c0 + nc) with NaN in the columns beside it; data, if given, is uploaded into it.  One window per panel at a
        time: the guards of the window before it go back to zero"""
        for g0, n in self.guards:
            self.window(g0, n).assign(0.0)
        self.guards = []
        for g0, g1 in ((max(0, c0 - T.GUARD), c0), (c0 + nc, c0 + nc + T.GUARD)):
            if g1 > g0:
                self.window(g0, g1 - g0).assign(NAN)
                self.guards.append((g0, g1 - g0))
        w = self.window(c0, nc)
        if data is not None:
            w.from_host(data)
        return w

    def intact(self):
        """every guard column still holds NaN in every row"""
        return all(np.isnan(self.window(g0, n).to_host()).all() for g0, n in self.guards)

    def destroy(self):
        if self.h:
            assert self.ctx.lib.rails_panel_destroy(self.h) == 0
            self.h = None


@contextlib.contextmanager
def tall(ctx, m, ld, cap=T.CAP):
    P = TallPanel(ctx, m, ld, cap)
    try:
        yield P
    finally:
        P.destroy()


class CompactOut:
    """a result window at column c0 of an ordinary panel full of NaN: the same interface as a guarded window of a TallPanel"""

    def __init__(self, ctx, m, c0, nc):
        self.c0, self.nc = c0, nc
        self.panel = MV(ctx, m=m, n=c0 + nc + T.GUARD, capacity=c0 + nc + T.GUARD)
        self.panel.assign(NAN)
        self.view = self.panel.view(c0, c0 + nc - 1)

    def intact(self):
        full = self.panel.to_host()
        return bool(np.isnan(np.delete(full, np.s_[self.c0:self.c0 + self.nc], axis=1)).all())
