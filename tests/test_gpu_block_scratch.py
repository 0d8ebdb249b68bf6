"""The block of an overlapped orthogonalisation in a compact scratch panel: the fused update + second projection
writes its result somewhere else than it reads (rails_update_gram_deferred_out), and the chain of the coordinate-space back end works in
that panel and writes the basis panel's tail once, at the end.  Nothing of this changes an operation or an order of summation, so
every comparison here is bit for bit: np.array_equal on the raw values, no tolerance."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rails_amd", "lib", "block_scratch_contract")
SENTINEL = -7.25  # what the output panel holds before the call


@pytest.fixture(scope="module")
def ctx():
    import rails_amd

    c = rails_amd.Context(device=0, seed=77)
    yield c
    c.close()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


class _PanelLd:
    """a device panel whose rows are exactly ld doubles apart, every column filled with the sentinel"""

    def __init__(self, ctx, m, ld):
        import rails_amd

        self.ctx, self.m, self.ld, self.chk = ctx, m, ld, rails_amd._lib.check
        self.h = C.c_void_p()
        self.chk(ctx.lib.rails_panel_create_ld(ctx.h, m, ld, ld, C.byref(self.h)), "rails_panel_create_ld")
        assert ctx.lib.rails_panel_ld(self.h) == ld and ctx.lib.rails_panel_capacity(self.h) == ld
        self.chk(ctx.lib.rails_panel_fill(ctx.h, self.h, 0, ld, SENTINEL), "rails_panel_fill")

    def to_host(self):
        out = np.zeros((self.m, self.ld), order="F")
        self.chk(self.ctx.lib.rails_panel_download(self.ctx.h, self.h, 0, self.ld, out.ctypes.data_as(C.POINTER(C.c_double)), self.m), "rails_panel_download")
        return out

    def close(self):
        if self.h:
            self.ctx.lib.rails_panel_destroy(self.h)
            self.h = None


# m = 4133: the fused kernel (from 4096 rows on), no multiple of 16 or 64; k covers NBW = 4, 6, 8 and k % 4 = 3, 0, 2, 2; (r, r2) the
# kernel with and without its 17th column; ld 18 as the back end allocates it and 17 (odd: the stores assume no alignment).
# m = 1000: the two separate kernels (Y is copied to the output panel first).
CASES = [(4133, k, r, r2, ld) for k in (35, 64, 258, 390) for (r, r2) in ((17, 16), (16, 7)) for ld in (18, 17)] + \
        [(1000, 35, r, r2, ld) for (r, r2) in ((17, 16), (16, 7)) for ld in (18, 17)]


@pytest.mark.parametrize("m,k,r,r2,ld", CASES)
def test_update_gram_output_elsewhere_equals_in_place(ctx, m, k, r, r2, ld):
    """rails_update_gram_deferred_out into another panel against rails_update_gram_deferred in place on a copy of the same panel: Y'
    and the slot bit for bit, the input Y untouched, the output panel's other columns untouched."""
    import rails_amd

    lib, chk = ctx.lib, rails_amd._lib.check
    dp = C.POINTER(C.c_double)
    g = np.random.default_rng(1000 * m + 10 * k + r)
    Xh = g.uniform(-1, 1, (m, k + r + 2))  # X = columns [0, k), Y right behind it, two more columns behind Y
    Ch = np.asfortranarray(g.uniform(-1, 1, (k + 3, r)))
    chk(lib.rails_deferred_reserve(ctx.h, 3, (k + 64) * 32), "rails_deferred_reserve")

    def fetch(slot):
        out = np.zeros((k, r2), order="F")
        chk(lib.rails_deferred_fetch(ctx.h, slot, k * r2, out.ctypes.data_as(dp)), "rails_deferred_fetch")
        return out

    fused0 = ctx.stats().get("update_gram_fused", 0)
    # in place, on a panel of its own
    Pin = rails_amd.HipMultiVectorWrapper(ctx, data=Xh)
    chk(lib.rails_update_gram_deferred(ctx.h, -1.0, Pin.panel.h, 0, k, Ch.ctypes.data_as(dp), k + 3, r, Pin.panel.h, k, r2, 1), "rails_update_gram_deferred")
    ctx.sync()
    want, want_slot = Pin.to_host(), fetch(1)
    # into another panel
    Pout = rails_amd.HipMultiVectorWrapper(ctx, data=Xh)
    S = _PanelLd(ctx, m, ld)
    try:
        chk(lib.rails_update_gram_deferred_out(ctx.h, -1.0, Pout.panel.h, 0, k, Ch.ctypes.data_as(dp), k + 3, r, Pout.panel.h, k, S.h, 0, r2, 2),
            "rails_update_gram_deferred_out")
        ctx.sync()
        got, got_slot, left = S.to_host(), fetch(2), Pout.to_host()
    finally:
        S.close()
    assert ctx.stats().get("update_gram_fused", 0) - fused0 == (2 if m >= 4096 else 0)
    assert not _same_bits(want[:, k:k + r], Xh[:, k:k + r])  # (the update did something)
    assert _same_bits(got[:, :r], want[:, k:k + r])
    assert _same_bits(got_slot, want_slot)
    assert _same_bits(left, Xh)  # the input Y, X and the columns behind them
    assert _same_bits(want[:, :k], Xh[:, :k]) and _same_bits(want[:, k + r:], Xh[:, k + r:])
    assert got.shape[1] == ld >= r and np.all(got[:, r:] == SENTINEL)  # (r = 17 fills the panel of 17 columns: nothing beyond)
    # against numpy, loosely: the bits above are the bits of the right thing (bound: k products of magnitude <= 1 per entry)
    ref = Xh[:, k:k + r] - Xh[:, :k] @ Ch[:k]
    assert np.abs(got[:, :r] - ref).max() <= 1e-13 * k


def test_update_gram_out_refuses_overlapping_windows(ctx):
    """windows of one panel that overlap are refused as by the other entry points, and so is an output window past the capacity"""
    import rails_amd

    lib = ctx.lib
    dp = C.POINTER(C.c_double)
    m, k, r = 64, 8, 4
    P = rails_amd.HipMultiVectorWrapper(ctx, data=np.zeros((m, k + 2 * r)))
    Ch = np.zeros((k, r), order="F")
    assert lib.rails_deferred_reserve(ctx.h, 3, 1024) == 0
    h = P.panel.h
    args = lambda yc0, out, oc0: (ctx.h, -1.0, h, 0, k, Ch.ctypes.data_as(dp), k, r, h, yc0, out, oc0, r, 0)
    assert lib.rails_update_gram_deferred_out(*args(k, h, k + 2)) != 0  # output partly over the input
    assert lib.rails_update_gram_deferred_out(*args(k, h, k - 1)) != 0  # output over X
    assert lib.rails_update_gram_deferred_out(*args(k - 1, h, k + r)) != 0  # input over X
    S = _PanelLd(ctx, m, 6)
    try:
        assert lib.rails_update_gram_deferred_out(*args(k, S.h, 3)) != 0  # [3, 7) of 6 columns
        assert lib.rails_update_gram_deferred_out(*args(k, S.h, 2)) == 0
        assert lib.rails_update_gram_deferred_out(*args(k, h, k + r)) == 0  # disjoint windows of the same panel
        ctx.sync()
    finally:
        S.close()


def test_chain_scratch_on_equals_scratch_off(monkeypatch):
    """Two solves of a small banded problem on the coordinate-space back end, the switch read per basis: the early blocks (fewer than 32
    basis columns) take the two separate kernels, later ones the fused pass, and the space is restarted at least once.  history(), V and
    T bit for bit; every overlapped block went through the scratch panel with the switch on, none with it off."""
    import rails_amd
    from rails_amd import problems as P

    m = 6000
    A = P.banded_random(m, nnz_row=9, bandwidth=64, seed=3)
    B = P.rhs(m, 4, seed=5)
    params = {"Restart size": 40, "Reduced size": 24, "Expand size": 4, "Lanczos iterations": 8, "Tolerance": 1e-30, "Maximum iterations": 100000}
    runs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("RAILS_SUBSPACE_BLOCK_SCRATCH", mode)
        c = rails_amd.Context(device=0, seed=1)
        c.set_seed(9, 0)
        op = rails_amd.HipOperatorWrapper(c, *A)
        s = rails_amd.Solver(c, op, B)
        assert s.set_parameters(params) == 0
        s.set_option("verbose", 0)
        s.set_option("subspace", 1)
        s.set_option("max_trips", 25)
        code, V, T = s.solve()
        runs[mode] = (code, s.trips(), np.array(s.history()), V, T, s.backend_stats(), c.stats().get("update_gram_fused", 0))
        s.close()
        c.close()
    (c0, t0, h0, V0, T0, st0, f0), (c1, t1, h1, V1, T1, st1, f1) = runs["0"], runs["1"]
    print({k: st1[k] for k in ("dim", "absorb", "overlapped_blocks", "scratch_blocks", "second_rounds", "compress")}, "fused passes", f1)
    assert t0 == t1 == 25 and c0 == c1
    assert st1["overlapped_blocks"] > 0 and st1["second_rounds"] > 0 and st1["compress"] >= 1
    assert st1["scratch_blocks"] == st1["overlapped_blocks"] and st0["scratch_blocks"] == 0
    assert 0 < f1 < st1["second_rounds"] and f0 == f1  # both forms of the first update were taken
    assert _same_bits(h1, h0) and _same_bits(V1, V0) and _same_bits(T1, T0)
    drop = ("seconds", "scratch_blocks")
    assert {k: v for k, v in st1.items() if k not in drop} == {k: v for k, v in st0.items() if k not in drop}


def test_chain_without_second_round_and_forced_shapes():
    """The branch without a second round (no fused pass: the first scaling moves the block) cannot be asked for through the solver --
    the DGKS rule decides per block -- so it is forced on the basis object itself, in C++ (tests/cpp/block_scratch_contract.cpp):
    scratch on against scratch off, basis panel and coordinates bit for bit, for that branch, for both forms of the first update, and
    for a scratch panel that grows."""
    if not os.path.exists(EXE):
        import rails_amd.build

        rails_amd.build.build()
    p = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("ALL PASSED"), p.stdout[-4000:]
    assert p.stdout.count("bit for bit") == 5 and "DIFFER" not in p.stdout, p.stdout[-4000:]
