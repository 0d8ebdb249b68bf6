"""tests/planes_reference.py on the host: the restated launch plan of the plane-sweep SpMM on the shapes whose plans follow from the
source (rails_amd/csrc/spmm_planes.hip: planes_dispatch, planes_launch) by hand, the grid search on the CU counts and widths the GPU
tests may meet, and the 7-point stencil with coefficients that can be told apart.  No GPU."""
import numpy as np
import pytest

import planes_reference as PR

WIDTHS = (2, 16, 18, 32, 48, 64, 128, 200, 256)  # every lane shape, widths just past a threshold, a ragged second chunk
MODES = ((7, True), (9, False))


def test_shape_table_and_patches():
    got = {nc: (PR.shape(nc)["LPR"], PR.shape(nc)["PX"], PR.shape(nc)["PY"]) for nc in (2, 16, 18, 32, 34, 64, 66, 128, 256)}
    assert got == {2: (8, 8, 16), 16: (8, 8, 16), 18: (16, 8, 12), 32: (16, 8, 12), 34: (32, 8, 8), 64: (32, 8, 8), 66: (64, 8, 4),
                   128: (64, 8, 4), 256: (64, 8, 4)}
    assert PR.plan((24, 21, 6), 256, 256)["chunks"] == 2 and PR.plan((11, 10, 4), 200, 256)["chunks"] == 2
    assert PR.plan((9, 19, 6), 48, 256)["chunks"] == 1 and PR.plan((5, 3, 40), 2, 256)["chunks"] == 1


@pytest.mark.parametrize("grid,nc,seglen,nseg", [((100, 100, 100), 128, 34, 3), ((100, 100, 100), 32, 50, 2), ((50, 50, 8), 128, 4, 2),
                                                 ((20, 12, 9), 128, 1, 9)])
def test_plan_on_shapes_worked_out_by_hand(grid, nc, seglen, nseg):
    """At 256 CUs.  100^3 at 128 columns: 13 x 25 = 325 patches; 1, 2, 3, 4 segments take 2, 3, 4, 6 rounds of 104, 54, 38, 29 steps:
    208, 162, 152, 174.  At 32 columns: 13 x 9 = 117 patches; 1 segment 104, 2 segments 1 round of 54, 3 segments 2 rounds of 38.
    50 x 50 x 8: 7 x 13 = 91 patches; 2 segments fit one round of 8 steps, 3 take 2 rounds of 7.  20 x 12 x 9: 9 patches, every
    plane its own segment in one round of 5."""
    p = PR.plan(grid, nc, 256)
    assert (p["seglen"], p["nseg"]) == (seglen, nseg), p


def test_plan_of_a_slab_depends_on_its_interior_planes_only():
    a = PR.plan((20, 18, 13), 128, 256, z_lo=0, z_hi=12)
    b = PR.plan((20, 18, 13), 128, 256, z_lo=1, z_hi=13)
    c = PR.plan((20, 18, 12), 128, 256)
    assert a == b == c


@pytest.mark.parametrize("num_cu", [64, 120, 256, 304])
@pytest.mark.parametrize("nc", WIDTHS)
@pytest.mark.parametrize("min_seglen,multi", MODES)
def test_find_grid_succeeds_within_the_row_cap(num_cu, nc, min_seglen, multi):
    g = PR.find_grid(nc, num_cu, min_seglen, multi)
    assert g is not None, "no grid of at most 400000 rows"
    gx, gy, gz = g
    p = PR.plan(g, nc, num_cu)
    assert gx * gy * gz <= 400_000 and gx > p["PX"] and gy > p["PY"] and gz >= 3
    assert p["seglen"] >= min_seglen and (p["nseg"] >= 2 if multi else p["nseg"] == 1)
    assert gx % p["PX"] != 0 and gy % p["PY"] != 0
    assert PR.find_grid(nc, num_cu, min_seglen, multi) == g  # deterministic
    assert gx * gy * gz <= 160_000, g  # what the GPU tests' run time is sized for


def test_find_grid_reports_failure():
    assert PR.find_grid(128, 256, 9, False, max_rows=100) is None


@pytest.mark.parametrize("shape", [(5, 4, 3), (9, 8, 7), (3, 3, 12)])
def test_cross7_random_is_the_complete_stencil_with_distinct_values(shape):
    gx, gy, gz = shape
    rp, col, val = PR.cross7_random(gx, gy, gz, seed=3)
    m = gx * gy * gz
    assert rp.size == m + 1 and rp[-1] == col.size == val.size
    idx = np.arange(m)
    x, y, z = idx % gx, (idx // gx) % gy, idx // (gx * gy)
    want = (1 + (x > 0) + (x < gx - 1)) + (1 + (y > 0) + (y < gy - 1)) + (1 + (z > 0) + (z < gz - 1)) - 2
    assert np.array_equal(np.diff(rp), want)
    dense = {}
    for r in range(m):
        c, v = col[rp[r]:rp[r + 1]].astype(np.int64), val[rp[r]:rp[r + 1]]
        assert np.all(np.diff(c) > 0)
        d = np.stack([c % gx - x[r], (c // gx) % gy - y[r], c // (gx * gy) - z[r]])
        assert np.abs(d).max() <= 1 and np.all((d != 0).sum(0) <= 1)
        assert np.unique(v).size == v.size
        for cc, vv in zip(c, v):
            dense[(r, int(cc))] = vv
    assert all((c, r) in dense for (r, c) in dense)                          # the pattern is symmetric ...
    assert all(dense[(c, r)] != v for (r, c), v in dense.items() if r != c)  # ... the values are not
