"""The plane-sweep SpMM (rails_amd/csrc/spmm_planes.hip; `A_ * W`, src/LyapunovSolver.hpp:146) in its steady state: z segments long
enough that the loop stores a plane while the next ones are in flight and both buffer rings wrap, with coefficients that can be told
apart -- the 27-point stencil with random values and the complete 7-point stencil with random values (planes_reference.cross7_random),
the only unsymmetric operator the kernel's 7-point form meets in the suite.

How long a segment is follows from the grid, the panel's width and the device's CU count (planes_launch's rule).  The grids come
from planes_reference.find_grid at the CU count of the device the tests run on, and every case asserts that the launch the library
reports (rails_csr_planes_stats) is the one the restated plan (planes_reference.plan) expects: a case that was meant to run a
segment of seven planes or more (nine steps of the loop) and did not is a failure, on any device.

Bounds, those of tests/test_gpu_planes.py: bit for bit the row-gather kernel (the same chain of fused multiply-adds per row, up to the
sign of an exact zero), and the CPU oracle (separate multiply and add) within 4e-14 sqrt(27) max(1, |Y|max)."""
import functools

import numpy as np
import pytest

import planes_reference as PR

pytestmark = pytest.mark.gpu

MULTI, SINGLE = (7, True), (9, False)  # (shortest segment, more than one segment) asked of find_grid


@pytest.fixture(scope="module")
def ctx():
    import rails_amd

    c = rails_amd.Context(device=0, seed=78)
    yield c
    c.close()


def _num_cu(ctx):
    return int(ctx.lib.rails_ctx_num_cu(ctx.h))


def _grid(nc, num_cu, mode):
    g = PR.find_grid(nc, num_cu, *mode)
    if g is None:
        pytest.fail("no grid of at most 400000 rows runs %d columns at seglen >= %d (%s) on %d CUs" % (nc, mode[0], "several segments" if mode[1] else "one segment", num_cu))
    return g


@functools.lru_cache(maxsize=4)
def _matrix(kind, grid):
    from rails_amd import problems as P

    if kind == "stencil27":
        return P.stencil27(*grid, random_values=True, seed=sum(grid))
    return PR.cross7_random(*grid, seed=sum(grid) + 1)


def _expected(grid, nc, num_cu, kind, z_lo=0, z_hi=None, interior=False):
    p = PR.plan(grid, nc, num_cu, z_lo, z_hi)
    want = {k: p[k] for k in ("LPR", "RW", "WX", "WY", "seglen", "nseg", "chunks")}
    want.update(built=True, accepted=True, cross=(kind == "cross7"), grid=tuple(grid), z_lo=z_lo, z_hi=grid[2] if z_hi is None else z_hi, interior=interior)
    return want


def _stats(op):
    st = op.planes_stats()
    y_vec = st.pop("y_vec")
    return st, y_vec


def _panels(ctx, m, nc, xoff, yoff, pad, seed):
    """X and Y as windows [xoff, xoff + nc) and [yoff, yoff + nc) of wider panels; Y's panel, two columns wider than the window's end, is
    filled with NaN"""
    import rails_amd

    Xh = np.random.default_rng(seed).uniform(-1, 1, (m, nc))
    big = rails_amd.HipMultiVectorWrapper(ctx, m=m, n=nc + xoff, capacity=nc + xoff + pad)
    X = big.view(xoff, xoff + nc - 1)
    X.from_host(Xh)
    outp = rails_amd.HipMultiVectorWrapper(ctx, m=m, n=nc + yoff + 2, capacity=nc + yoff + 2 + pad)
    outp.assign(float("nan"))
    Y = outp.view(yoff, yoff + nc - 1)
    return Xh, X, Y, outp


def _check(ctx, oracle, kind, nc, mode, xoff=0, yoff=0, pad=0, want_y_vec=1):
    import rails_amd

    num_cu = _num_cu(ctx)
    grid = _grid(nc, num_cu, mode)
    A = _matrix(kind, grid)
    m = A[0].size - 1
    op = rails_amd.HipOperatorWrapper(ctx, *A)
    Xh, X, Y, outp = _panels(ctx, m, nc, xoff, yoff, pad, seed=nc + m % 5)
    before = outp.to_host().view(np.uint64)
    assert np.isnan(outp.to_host()).all()
    op.set_variant(9)
    op.apply(X, Y)
    assert op.last_kernel() == "k_spmm_planes"
    st, y_vec = _stats(op)
    want = _expected(grid, nc, num_cu, kind)
    print("%s %d columns on %d CUs: grid %s, %d rows, seglen %d x %d segments, %d chunk(s), y_vec %d" % (kind, nc, num_cu, grid, m, st["seglen"], st["nseg"], st["chunks"], y_vec))
    assert st == want, (st, want)
    assert st["seglen"] >= mode[0] and (st["nseg"] >= 2) == mode[1]
    assert y_vec == want_y_vec
    Yp = Y.to_host()
    after = outp.to_host().view(np.uint64)
    assert np.array_equal(after[:, :yoff], before[:, :yoff]) and np.array_equal(after[:, yoff + nc:], before[:, yoff + nc:])  # outside the window: untouched
    op.set_variant(3)
    op.apply(X, Y)
    assert op.last_kernel() == "k_spmm_rowgather"
    Yr = Y.to_host()
    assert np.isfinite(Yp).all()
    assert np.array_equal(Yp, Yr), np.abs(Yp - Yr).max()
    Yo = oracle.csr_spmm(*A, Xh)
    assert np.abs(Yp - Yo).max() <= 4e-14 * np.sqrt(27) * max(1.0, np.abs(Yo).max())


@pytest.mark.parametrize("mode", [MULTI, SINGLE], ids=["segments", "one_segment"])
@pytest.mark.parametrize("kind", ["stencil27", "cross7"])
@pytest.mark.parametrize("nc", [16, 32, 64, 128, 256])
def test_long_segments_at_every_lane_shape(ctx, oracle, nc, kind, mode):
    """The four instantiations by width (and two column chunks at 256) on segments of at least 7 planes -- several of them, the last one
    shorter -- and on one segment of at least 9."""
    _check(ctx, oracle, kind, nc, mode)


@pytest.mark.parametrize("kind", ["stencil27", "cross7"])
@pytest.mark.parametrize("nc", [2, 18, 48, 200])
def test_long_segments_at_widths_that_do_not_fill_the_lanes(ctx, oracle, nc, kind):
    """Lanes beyond the panel's width (2 of 16 columns, 18 of 32, 48 of 64) and a ragged second chunk (200 = 128 + 72)."""
    _check(ctx, oracle, kind, nc, MULTI)


@pytest.mark.parametrize("xoff,yoff,pad,y_vec", [(2, 3, 0, 0), (2, 4, 5, 1)], ids=["odd_y_offset", "even_y_offset_padded"])
@pytest.mark.parametrize("kind", ["stencil27", "cross7"])
@pytest.mark.parametrize("nc", [16, 128])
def test_windows_in_the_steady_state(ctx, oracle, nc, kind, xoff, yoff, pad, y_vec):
    """Y's window on an odd column takes two 8-byte stores per row between the LDS-DMA requests the kernel's waits count: here in steps
    that store while planes are in flight.  The panel is NaN before the product; the columns before and after the window keep their bits."""
    _check(ctx, oracle, kind, nc, MULTI, xoff=xoff, yoff=yoff, pad=pad, want_y_vec=y_vec)


@pytest.mark.parametrize("kind,nc", [("stencil27", 128), ("cross7", 16), ("stencil27", 32)])
def test_the_same_product_three_times_gives_the_same_bits(ctx, kind, nc):
    """A missing wait or barrier shows as run-to-run differences before it shows as a large error."""
    import rails_amd

    num_cu = _num_cu(ctx)
    grid = _grid(nc, num_cu, MULTI)
    A = _matrix(kind, grid)
    m = A[0].size - 1
    op = rails_amd.HipOperatorWrapper(ctx, *A)
    _, X, Y, outp = _panels(ctx, m, nc, 0, 0, 0, seed=nc)
    op.set_variant(9)
    runs = []
    for _ in range(3):
        outp.assign(float("nan"))
        op.apply(X, Y)
        runs.append(Y.to_host().view(np.uint64))
    st, _ = _stats(op)
    assert st == _expected(grid, nc, num_cu, kind) and st["seglen"] >= 7
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])


@pytest.mark.parametrize("kind", ["stencil27", "cross7"])
@pytest.mark.parametrize("nc", [128, 16])
def test_z_slabs_run_long_interior_segments_bitwise_the_serial_product(ctx, oracle, monkeypatch, kind, nc):
    """Two ranks, each a z-slab of gz + 1 planes whose gz planes without ghost columns go to the plane kernel beside the halo exchange
    (rails_spmm_planes_interior): segments of at least 7 planes by the restated plan with the rank's z range, asserted from the stats.
    Bit for bit the serial product on the row kernels, and the oracle within the bound."""
    import partition_ranks
    from rails_amd import partition
    from rails_amd.wrappers import HipMultiVectorWrapper as MV
    from test_gpu_partition import _rank_setup

    num_cu = _num_cu(ctx)
    gx, gy, gz = _grid(nc, num_cu, MULTI)
    local = (gx, gy, gz + 1)
    A = _matrix(kind, (gx, gy, 2 * (gz + 1)))
    m = A[0].size - 1
    Xh = np.random.default_rng(7).uniform(-1, 1, (m, nc))
    starts = partition.row_ranges(m, 2)
    assert int(starts[1]) == gx * gy * (gz + 1)
    z_range = [(0, gz), (1, gz + 1)]  # rank 0's last plane and rank 1's first have ghost columns
    results = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("RAILS_SPMM_HALO_OVERLAP", mode)
        ranks = partition_ranks.MailboxRanks(2)

        def work(r):
            c, op, plan = _rank_setup(ranks, r, starts, A, seed=5)
            r0, r1 = int(starts[r]), int(starts[r + 1])
            if mode == "0":
                op.set_variant(1)  # the serial order on the row kernels
            Y = op.apply(MV(c, data=Xh[r0:r1]))
            out = dict(Y=Y.to_host(), kernel=op.last_kernel(), planes=op.planes_stats())
            c.close()
            return out

        results[mode] = ranks.run(work)
    for r in range(2):
        assert "k_spmm_planes" in results["1"][r]["kernel"] and "halo overlapped" in results["1"][r]["kernel"]
        assert "k_spmm_planes" not in results["0"][r]["kernel"]
        st = results["1"][r]["planes"]
        assert st.pop("y_vec") == 1
        want = _expected(local, nc, num_cu, kind, *z_range[r], interior=True)
        assert st == want, (r, st, want)
        assert st["seglen"] >= 7 and st["nseg"] >= 2
    Yo = np.vstack([results["1"][r]["Y"] for r in range(2)])
    Ys = np.vstack([results["0"][r]["Y"] for r in range(2)])
    assert np.array_equal(Yo, Ys), np.abs(Yo - Ys).max()
    ref = oracle.csr_spmm(*A, Xh)
    assert np.abs(Yo - ref).max() <= 4e-14 * np.sqrt(27) * max(1.0, np.abs(ref).max())
