"""Every form of the LDS-staged SpMM (rails_amd/csrc/spmm_tiled.hip: k_spmm_tiled, k_spmm_tiled_pipe, k_spmm_tiled_reg<KC, NNZ, NL, V2, NS>)
against the host references of tests/spmm_reference.py.

Each case runs a product through operator variant 2 (8-column chunks) or 6 (16-column chunks where they apply), asserts through
tile_stats() WHICH kernel and instantiation ran -- derived below from the dispatcher (rails_spmm_tiled; the plan itself is host code,
rails_amd/csrc/tile_plan.cpp, checked without a GPU by test_tile_plan_host.py), so a moved threshold fails here instead of
silently taking the coverage away -- and checks the result

  exactly   integer val in [-8, 8] \\ {0} and X in [-16, 16]: every partial sum is an exact double, Y must equal the int64 product;
  bounded   val, X uniform on (-1, 1): |Y - ref| <= 2 n_i 2^-53 (|A||X|)_ij per entry against a longdouble reference (derivation in
            spmm_reference.py);
  outside   Y is a window of a panel prefilled with a sentinel: every other column of the panel must still hold it;
  empty     rows without entries come back as exactly 0.

The form follows from the plan (tiles of 64 rows, or 4 x 4 x 4 / 4 x 16 x 1 boxes of a grid) like this, fp the largest footprint:
register kernel if the padded X row has room for the rounded-up last chunk (and ghost rows are whole chunks), the longest row has at most
32 entries and ceil(fp * KC/2 / 256) <= 8 staging slots suffice -- NNZ = 8 / 16 / 28 / 32 by the longest row, NL = 4 up to four slots,
else 8, NS = 2 unless V2 = 2 and 2 NNZ + 8 NL > 100; else the pipelined kernel if ceil(fp * 4 / 256) <= 8 (NL likewise); else the plain
one.  The references are computed once per matrix at the widest panel (130 columns); narrower cases use its leading columns."""
import functools
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import spmm_reference as R

pytestmark = pytest.mark.gpu

LD = np.longdouble
WMAX = 130
SENTINEL = -7.0e77
REG, PIPE, PLAIN = "k_spmm_tiled_reg", "k_spmm_tiled_pipe", "k_spmm_tiled"
# (nc, xoff, yoff): widths below, at and above one chunk, odd widths (single-column store), windows inside wider panels
WINDOWS = ((8, 0, 0), (9, 0, 0), (15, 0, 2), (16, 16, 0), (17, 0, 2), (24, 0, 0), (64, 2, 0), (130, 0, 0))
# the padded X row (a multiple of 16 columns) has no room for the rounded-up last chunk behind the window: never the register kernel
NO_ROOM = ((14, 2, 0), (126, 2, 0))


@pytest.fixture(scope="module")
def ctx():
    import rails_amd

    c = rails_amd.Context(device=0, seed=1234)
    yield c
    c.close()


def MV(ctx, **kw):
    import rails_amd

    return rails_amd.HipMultiVectorWrapper(ctx, **kw)


class Case:
    """a pattern with its two sets of values, the two panels at WMAX columns and the references (computed once, never modified).
    col indexes the rows of the panels (x_rows of them: more than the matrix has rows for a row block with ghost columns)."""

    def __init__(self, rowptr, col, x_rows=None):
        self.rowptr = np.asarray(rowptr, dtype=np.int64)
        self.col = np.asarray(col, dtype=np.int64)
        self.m = self.rowptr.size - 1
        self.x_rows = self.m if x_rows is None else x_rows
        self.empty = np.diff(self.rowptr) == 0
        self.val = {"int": R.int_values(self.col.size, seed=7), "uni": R.uniform_values(self.col.size, seed=8)}
        self.X = {"int": R.int_panel(self.x_rows, WMAX), "uni": R.uniform_panel(self.x_rows, WMAX, seed=9)}
        self.ref_int = R.spmm_exact_int(self.rowptr, self.col, self.val["int"], self.X["int"])
        self.ref, B = R.spmm_longdouble(self.rowptr, self.col, self.val["uni"], self.X["uni"])
        self.bound = R.spmm_bound(self.rowptr, B)
        for a in (self.ref_int, self.ref, self.bound, self.X["int"], self.X["uni"]):
            a.setflags(write=False)


def _box_fail_grid():
    """7-point pattern of a 16 x 24 x 24 grid (m = 9216: the grid detection samples every second row, the even ones).  On the odd rows
    with x = 1 mod 4, y even, z mod 8 < 4 the x+1 neighbour is replaced by the column 4003 rows on: the sampled rows still say `grid`,
    but the tiles of every other layer of boxes have eight columns outside their halo box."""
    from rails_amd import problems as P

    nx, ny, nz = 16, 24, 24
    rowptr, col, _ = P.laplace7(nx, ny, nz)
    m = nx * ny * nz
    col = col.astype(np.int64).copy()
    r = np.arange(m)
    x, y, z = r % nx, (r // nx) % ny, r // (nx * ny)
    changed = np.flatnonzero((x % 4 == 1) & (y % 2 == 0) & (z % 8 < 4))
    assert (changed % 2 == 1).all() and m // 4096 == 2
    for i in changed:
        seg = col[rowptr[i]:rowptr[i + 1]]
        seg[seg == i + 1] = (i + 4003) % m
        seg.sort()
        assert np.unique(seg).size == seg.size
    return rowptr, col, changed


@functools.lru_cache(maxsize=None)
def case(name):
    from rails_amd import problems as P

    if name.startswith("banded"):  # banded_<nnz per row>_<bandwidth>
        _, n, bw = name.split("_")
        rowptr, col, _ = P.banded_random(3000, int(n), int(bw), seed=1)
    elif name == "grid9_2d":
        rowptr, col, _ = P.stencil27(50, 61, 1)
    elif name == "grid5_2d":
        rowptr, col, _ = P.laplace7(50, 61, 1)
    elif name == "grid27":
        rowptr, col, _ = P.stencil27(9, 8, 7)
    elif name == "grid7":
        rowptr, col, _ = P.laplace7(23, 11, 9)
    elif name == "ragged":
        rowptr, col = R.ragged_banded(2990)
    elif name == "ragged_long_row":
        rowptr, col = R.ragged_banded(2990, long_row=(1500, 40))
    elif name == "ragged_empty_tail":  # the whole last tile (rows 2944..2989) without entries
        rowptr, col = R.ragged_banded(2990, empty_tail=46)
    elif name == "box_fail":
        rowptr, col, _ = _box_fail_grid()
    else:
        raise KeyError(name)
    return Case(rowptr, col)


def make_ops(ctx, c, variant, col=None, ncols_ext=None):
    import rails_amd

    ops = {}
    for kind in ("int", "uni"):
        ops[kind] = rails_amd.HipOperatorWrapper(ctx, c.rowptr, c.col if col is None else col, c.val[kind], ncols_ext=ncols_ext)
        ops[kind].set_variant(variant)
    return ops


def product(ctx, op, Xh, xoff, yoff):
    """Y = A Xh with X a window at column xoff and Y a window at column yoff of a panel full of SENTINEL; returns Y after checking that
    the rest of the panel, up to its capacity, was left alone"""
    m, nc = Xh.shape
    big = MV(ctx, m=m, n=nc + xoff, capacity=nc + xoff)
    X = big.view(xoff, xoff + nc - 1)
    X.from_host(Xh)
    cap = yoff + nc + 3
    outp = MV(ctx, m=op.M(), n=cap, capacity=cap)
    outp.assign(SENTINEL)
    op.apply(X, outp.view(yoff, yoff + nc - 1))
    full = outp.to_host()
    outside = np.delete(full, np.s_[yoff:yoff + nc], axis=1)
    assert outside.shape[1] == yoff + 3 and (outside == SENTINEL).all(), "columns outside the Y window were written"
    return full[:, yoff:yoff + nc]


def form_of(op):
    st = op.tile_stats()
    assert st["built"] and st["accepted"] and op.last_kernel() == st["kernel"], (st, op.last_kernel())
    return (st["kernel"], st["KC"], st["NNZ"], st["NL"], st["V2"], st["NS"])


def check(ctx, c, ops, nc, xoff, yoff, want, before=None):
    """both checks of one window; before(kind, nc) runs ahead of each product (the ghost rows' hook needs to know the panel)"""
    for kind in ("int", "uni"):
        if before:
            before(kind, nc)
        Y = product(ctx, ops[kind], c.X[kind][:c.m, :nc], xoff, yoff)
        got = form_of(ops[kind])
        print("FORM", got, "window", (nc, xoff, yoff), kind)
        assert got == want, (got, want, ops[kind].tile_stats())
        if kind == "int":
            bad = np.argwhere(Y != c.ref_int[:, :nc])
            assert bad.size == 0, "%d entries differ from the exact product, first at %s" % (len(bad), bad[0])
        else:
            err, bound = np.abs(Y.astype(LD) - c.ref[:, :nc]), c.bound[:, :nc]
            ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
            print("max |Y - ref| / bound = %.3f" % ratio)
            assert (err <= bound).all(), ratio
        assert (Y[c.empty] == 0).all()


# --------------------------------------------------------------------------------------------------- runs of consecutive rows
# max row nnz, max footprint and reuse of these are asserted on the host in test_spmm_reference_host.py
BANDED = {
    "banded_12_40": ((REG, 8, 16, 4, 1, 2), (PIPE, 8, 0, 4, 0, 0)),    # 12 per row, footprint 136
    "banded_31_40": ((REG, 8, 32, 4, 1, 2), (PIPE, 8, 0, 4, 0, 0)),    # 31 per row, footprint 143
    "banded_27_150": ((REG, 8, 28, 8, 1, 2), (PIPE, 8, 0, 8, 0, 0)),   # footprint 349: 6 staging slots
    "banded_40_60": ((PIPE, 8, 0, 4, 0, 0), (PIPE, 8, 0, 4, 0, 0)),    # 40 per row: beyond the register kernel
    "banded_32_400": ((PLAIN, 8, 0, 0, 0, 0), (PLAIN, 8, 0, 0, 0, 0)),  # footprint 778: 13 staging slots, beyond both
}


@pytest.mark.parametrize("name", sorted(BANDED))
def test_banded_forms_and_windows(ctx, name):
    c = case(name)
    ops = make_ops(ctx, c, 2)
    want, want_no_room = BANDED[name]
    for nc, xoff, yoff in WINDOWS:
        check(ctx, c, ops, nc, xoff, yoff, want)
    for nc, xoff, yoff in NO_ROOM:
        check(ctx, c, ops, nc, xoff, yoff, want_no_room)
    st = ops["int"].tile_stats()
    host = R.tile_stats_host(c.rowptr, c.col)
    assert not st["grid"] and st["tile_rows"] == 64 and st["n_tiles"] == 47 and st["max_fp"] == host["max_fp"] == st["max_pos"]
    assert st["max_row_nnz"] == host["max_row_nnz"] and abs(st["reuse"] - host["reuse"]) < 1e-12


# ------------------------------------------------------------------------------------------------------------------- box plans
GRIDS = {
    # 50 x 61 x 1: 4 x 16 x 1 boxes (neither extent a multiple of the box), halo box 8 x 18 x 3 = 432 LDS rows
    "grid9_2d": ((REG, 8, 16, 4, 1, 2), 432),
    "grid5_2d": ((REG, 8, 8, 4, 1, 2), 432),
    # 4 x 4 x 4 boxes, halo box 8 x 6 x 6 = 288 LDS rows, partial boxes at the far faces.  9 x 8 x 7 has no box away from every face: the
    # largest footprint is 6 x 5 x 5; 23 x 11 x 9 has interior boxes: 64 + 6 x 16 columns of the 7-point pattern
    "grid27": ((REG, 8, 28, 4, 1, 2), 288),
    "grid7": ((REG, 8, 8, 4, 1, 2), 288),
}


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_grid_forms_and_windows(ctx, name):
    c = case(name)
    ops = make_ops(ctx, c, 2)
    want, max_pos = GRIDS[name]
    for nc, xoff, yoff in WINDOWS:
        check(ctx, c, ops, nc, xoff, yoff, want)
    for nc, xoff, yoff in NO_ROOM:
        check(ctx, c, ops, nc, xoff, yoff, (PIPE, 8, 0, 4, 0, 0))
    st = ops["int"].tile_stats()
    assert st["grid"] and st["tile_rows"] == 64 and st["max_pos"] == max_pos, st
    if name == "grid27":
        assert st["max_fp"] == 150
    if name == "grid7":
        assert st["max_fp"] == 160


def test_grid_whose_tiles_fail_the_box_layout(ctx):
    """the grid detection looks at a sample of rows; tiles whose columns do not fit the halo box fall back to consecutive LDS rows"""
    c = case("box_fail")
    ops = make_ops(ctx, c, 2)
    for nc, xoff, yoff in ((8, 0, 0), (17, 0, 2), (64, 2, 0)):
        check(ctx, c, ops, nc, xoff, yoff, (REG, 8, 8, 4, 1, 2))
    st = ops["int"].tile_stats()
    # detected as a grid; the largest footprint is the 160 of the 7-point box and the 8 far columns
    assert st["grid"] and st["tile_rows"] == 64 and st["n_tiles"] == 4 * 6 * 6 and st["max_fp"] == 168 and st["max_pos"] == 288, st
    check(ctx, c, ops, 14, 2, 0, (PIPE, 8, 0, 4, 0, 0))


# ---------------------------------------------------------------------------------------------------------------- ragged rows
@pytest.mark.parametrize("name,want", [("ragged", (REG, 8, 32, 4, 1, 2)), ("ragged_long_row", (PIPE, 8, 0, 4, 0, 0)),
                                       ("ragged_empty_tail", (REG, 8, 32, 4, 1, 2))])
def test_ragged_rows_empty_rows_and_a_short_last_tile(ctx, name, want):
    """rows of 0..30 entries, every 37th and the last one empty, 2990 = 46 x 64 + 46 rows.  The empty last row (and, in
    ragged_empty_tail, a last tile with no footprint at all) is where the register kernel's unconditional loads of entry 0 used to
    reach one element past the plan's arrays."""
    c = case(name)
    assert c.empty[-1] and c.empty[::37].all() and c.m % 64 == 46 and np.diff(c.rowptr).max() == (40 if name == "ragged_long_row" else 30)
    ops = make_ops(ctx, c, 2)
    for nc, xoff, yoff in ((8, 0, 0), (17, 0, 2), (24, 0, 0), (130, 0, 0)):
        check(ctx, c, ops, nc, xoff, yoff, want)
    check(ctx, c, ops, 14, 2, 0, (PIPE, 8, 0, 4, 0, 0))
    st = ops["int"].tile_stats()
    assert st["n_tiles"] == 47 and st["reuse"] >= 1.8


# ------------------------------------------------------------------------------------------------------- non-finite isolation
@pytest.mark.parametrize("name,want", [("banded_12_40", (REG, 8, 16, 4, 1, 2)), ("banded_40_60", (PIPE, 8, 0, 4, 0, 0)),
                                       ("banded_32_400", (PLAIN, 8, 0, 0, 0, 0)), ("ragged", (REG, 8, 32, 4, 1, 2))])
def test_rows_that_do_not_reference_a_non_finite_x_row_stay_finite(ctx, name, want):
    """inf in one X row: the rows of A that reference it come out non-finite, all others exactly as clean as before -- the padded
    coefficients alias the row's own first entry, idle slots shadow row 0 of their tile and spare staging slots duplicate footprint
    row 0, so a stray inf * 0 would show as NaN in rows that have nothing to do with it"""
    import rails_amd

    c = case(name)
    op = rails_amd.HipOperatorWrapper(ctx, c.rowptr, c.col, c.val["uni"])
    op.set_variant(2)
    nc = 24
    rows_of = np.repeat(np.arange(c.m), np.diff(c.rowptr))
    last_tile = c.col[c.rowptr[c.m // 64 * 64]:]
    targets = [0, 1500, c.m - 1, int(c.col[c.rowptr[1472]])] + ([int(last_tile.min())] if last_tile.size else [])
    for r in targets:
        Xh = np.array(c.X["uni"][:, :nc])
        Xh[r] = np.inf
        Y = product(ctx, op, Xh, 0, 0)
        assert form_of(op) == want
        hit = np.zeros(c.m, dtype=bool)
        hit[rows_of[c.col == r]] = True
        assert hit.any() or name == "ragged"
        assert not np.isfinite(Y[hit]).any(), "a row that references X row %d came out finite" % r
        clean = Y[~hit]
        assert np.isfinite(clean).all(), "X row %d leaked into rows %s" % (r, np.flatnonzero(~hit)[~np.isfinite(clean).all(1)][:5])
        assert (np.abs(clean.astype(LD) - c.ref[~hit, :nc]) <= c.bound[~hit, :nc]).all()


# ------------------------------------------------------------------------------------------------------------ odd offsets
def test_odd_offsets_are_refused_by_variant_2_and_computed_by_the_automatic_choice(ctx):
    import rails_amd

    c = case("banded_12_40")
    ops2, ops0 = make_ops(ctx, c, 2), make_ops(ctx, c, 0)
    for nc, xoff, yoff in ((16, 1, 0), (16, 0, 1), (17, 1, 3), (64, 3, 0), (130, 0, 5)):
        with pytest.raises(rails_amd.RailsError):
            product(ctx, ops2["int"], c.X["int"][:, :nc], xoff, yoff)
        Y = product(ctx, ops0["int"], c.X["int"][:, :nc], xoff, yoff)
        assert not ops0["int"].last_kernel().startswith("k_spmm_tiled"), ops0["int"].last_kernel()
        assert np.array_equal(Y, c.ref_int[:, :nc])
        Yu = product(ctx, ops0["uni"], c.X["uni"][:, :nc], xoff, yoff)
        assert (np.abs(Yu.astype(LD) - c.ref[:, :nc]) <= c.bound[:, :nc]).all()


# ------------------------------------------------------------------------------------------------------------- variant 6
WIDE_WINDOWS = ((32, 0, 0), (33, 0, 2), (64, 2, 0), (130, 0, 0))


@pytest.mark.parametrize("name,want", [
    ("grid27", (REG, 16, 28, 8, 2, 1)),         # footprint 150 x 8 pieces: 5 staging slots; 2 * 28 + 8 * 8 > 100: one chunk in flight
    ("banded_12_30", (REG, 16, 16, 4, 2, 2)),   # footprint <= 128 (asserted on the host): 4 staging slots
    ("banded_27_150", (PIPE, 8, 0, 8, 0, 0)),   # footprint 349 x 8 pieces: 11 staging slots, no wide form; back to 8-column chunks
])
def test_variant_6_wide_chunks(ctx, name, want):
    c = case(name)
    ops = make_ops(ctx, c, 6)
    for nc, xoff, yoff in WIDE_WINDOWS:
        check(ctx, c, ops, nc, xoff, yoff, want)
    if name == "banded_12_30":
        assert ops["int"].tile_stats()["max_fp"] <= 128
        # below 32 columns, and where the padded row has no room for a 16-column last chunk: the 8-column forms
        check(ctx, c, ops, 24, 0, 0, (REG, 8, 16, 4, 1, 2))
        check(ctx, c, ops, 126, 2, 0, (PIPE, 8, 0, 4, 0, 0))


# ----------------------------------------------------------------------------------------------------------- ghost columns
def _ghost_block(kind):
    """rows [r0, r1) of a matrix, columns global -> (Case over the global panel, local column indices, ghost rows' global indices)"""
    from rails_amd import problems as P

    if kind == "banded":
        r0, r1, mg = 700, 2100, 3000
        rowptr, colg, _ = P.csr_rows(P.banded_random(mg, 27, 40, seed=1), r0, r1)
    else:
        nx, ny, nz, z0, z1 = 10, 9, 12, 3, 9
        r0, r1, mg = z0 * nx * ny, z1 * nx * ny, nx * ny * nz
        rowptr, colg, _ = P.stencil27_block(nx, ny, nz, z0, z1)
    colg = np.asarray(colg, dtype=np.int64)
    own = (colg >= r0) & (colg < r1)
    ghosts = np.unique(colg[~own])
    ml = r1 - r0
    col_local = np.where(own, colg - r0, ml + np.searchsorted(ghosts, colg)).astype(np.int32)
    c = Case(rowptr, colg, x_rows=mg)
    c.r0 = r0
    return c, col_local, ghosts


@pytest.mark.parametrize("kind", ["banded", "stencil27"])
def test_ghost_columns_on_one_rank(ctx, kind):
    """a row block with its ghost columns numbered behind the local ones, nothing to send, and a hook that puts the ghost rows of the
    known panel into the receive buffer (stored with ld = nc): the `c >= m` path of all three kernels' staging, which no other test
    drives through a tiled kernel.  Ghost rows must be whole chunks for the register kernel: 20 columns take the pipelined one."""
    import ctypes as C

    import rails_amd

    rails_amd.load()
    hip_memcpy = C.CDLL(None).hipMemcpy  # the HIP runtime the library brought in
    hip_memcpy.restype, hip_memcpy.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    c, col_local, ghosts = _ghost_block(kind)
    ng = int(ghosts.size)
    assert ng > 0 and (col_local >= c.m).any()
    plan = types.SimpleNamespace(send_rows=np.zeros(0, dtype=np.int64), n_send=0, n_ghost=ng, nranks=1, send_counts=[0], recv_counts=[ng])
    state = {}

    def hook(send_ptr, recv_ptr, ncols, stream):
        ctx.sync()  # the product before this one has read the buffer
        G = np.ascontiguousarray(state["X"][ghosts, :ncols])
        return hip_memcpy(recv_ptr, G.ctypes.data, G.nbytes, 1)  # host to device, done when it returns

    ops = make_ops(ctx, c, 2, col=col_local, ncols_ext=c.m + ng)
    for op in ops.values():
        op.set_halo(plan, hook)
    local = Case.__new__(Case)  # the same references, the panels cut to the block's own rows
    local.__dict__.update(c.__dict__)
    local.X = {k: v[c.r0:c.r0 + c.m] for k, v in c.X.items()}

    def before(k, nc):
        state["X"] = c.X[k]

    nnz_slots = 28  # 27 per row in both
    for nc in (64, 16, 24):
        check(ctx, local, ops, nc, 0, 0, (REG, 8, nnz_slots, 4, 1, 2), before=before)
    check(ctx, local, ops, 20, 0, 0, (PIPE, 8, 0, 4, 0, 0), before=before)
    assert ops["int"].tile_stats()["grid"] == (kind == "stencil27")


# -------------------------------------------------------------------------------------------------------- shipped switches
CHILD = r"""
import json
import numpy as np
import rails_amd
from rails_amd import problems as P
import spmm_reference as R

ctx = rails_amd.Context(device=0, seed=1)
out = []
for name, A in (("banded", P.banded_random(3000, 27, 40, seed=1)), ("stencil27", P.stencil27(20, 12, 9))):
    rowptr, col = A[0], A[1]
    m = rowptr.size - 1
    val = R.int_values(col.size, seed=7)
    op = rails_amd.HipOperatorWrapper(ctx, rowptr, col, val)
    op.set_variant(2)
    for nc in (16, 130):
        X = R.int_panel(m, nc)
        Y = op.apply(rails_amd.HipMultiVectorWrapper(ctx, data=X)).to_host()
        st = op.tile_stats()
        st.update(matrix=name, nc=nc, exact=bool(np.array_equal(Y, R.spmm_exact_int(rowptr, col, val, X))), last_kernel=op.last_kernel())
        out.append(st)
print("TILE_STATS " + json.dumps(out))
"""

# setting -> form on banded_random(3000, 27, 40) (footprint <= 144 at 64 rows, 336 at 256, <= 112 at 32), form on stencil27(20, 12, 9)
# (footprint 216 in 4 x 4 x 4 boxes, 600 in 8 x 8 x 4 ones)
SWITCHES = [
    # 16-column chunks, one 16-byte vector per lane: 8 lanes per row leave 32 row slots, so 64-row tiles take the pipelined kernel
    ({"RAILS_SPMM_TILE_KC": "16"}, (PIPE, 16, 0, 8, 0, 0), (PIPE, 16, 0, 8, 0, 0)),
    ({"RAILS_SPMM_TILE_NS": "1"}, (REG, 8, 28, 4, 1, 1), (REG, 8, 28, 4, 1, 1)),
    ({"RAILS_SPMM_TILE_NS": "3"}, (REG, 8, 28, 4, 1, 3), (REG, 8, 28, 4, 1, 3)),
    ({"RAILS_SPMM_TILE_REG": "0"}, (PIPE, 8, 0, 4, 0, 0), (PIPE, 8, 0, 4, 0, 0)),
    ({"RAILS_SPMM_TILE_REG": "0", "RAILS_SPMM_TILE_PIPE": "0"}, (PLAIN, 8, 0, 0, 0, 0), (PLAIN, 8, 0, 0, 0, 0)),
    # 256-row tiles: too many rows for the register kernel; the 8 x 8 x 4 boxes' 600 columns need 10 staging slots
    ({"RAILS_SPMM_TILE_ROWS": "256"}, (PIPE, 8, 0, 8, 0, 0), (PLAIN, 8, 0, 0, 0, 0)),
    # ... and with 32-row tiles the register kernel at 16-column chunks, V2 = 1 (boxes stay 4 x 4 x 4)
    ({"RAILS_SPMM_TILE_KC": "16", "RAILS_SPMM_TILE_ROWS": "32"}, (REG, 16, 28, 4, 1, 2), (PIPE, 16, 0, 8, 0, 0)),
]


@pytest.mark.parametrize("setting,want_banded,want_grid", SWITCHES, ids=["+".join("%s=%s" % (k[11:], v) for k, v in s[0].items()) for s in SWITCHES])
def test_shipped_switches_in_a_child_process(setting, want_banded, want_grid):
    """the switches are read once per process: one child per setting computes the exact check on a banded and a 27-point matrix at 16
    and 130 columns and reports what ran"""
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    env = {k: v for k, v in os.environ.items() if not k.startswith("RAILS_SPMM_")}
    env.update(setting, PYTHONPATH=os.pathsep.join([root, here]))
    out = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True, timeout=240, cwd=root)
    assert out.returncode == 0, out.stdout + out.stderr
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("TILE_STATS ")]
    assert len(line) == 1, out.stdout + out.stderr
    stats = json.loads(line[0][len("TILE_STATS "):])
    assert [(s["matrix"], s["nc"]) for s in stats] == [("banded", 16), ("banded", 130), ("stencil27", 16), ("stencil27", 130)]
    for s in stats:
        got = (s["kernel"], s["KC"], s["NNZ"], s["NL"], s["V2"], s["NS"])
        print("FORM", got, "switch", setting, s["matrix"], s["nc"])
        assert s["exact"], s
        assert s["accepted"] and s["last_kernel"] == s["kernel"]
        assert got == (want_banded if s["matrix"] == "banded" else want_grid), s
