"""The host references of tests/spmm_reference.py against a dense longdouble product, and the tile statistics that
tests/test_gpu_spmm_tiled.py relies on to reach every form of the LDS-staged kernel.  No GPU."""
import numpy as np
import pytest

import spmm_reference as R

LD = np.longdouble


def _small_cases():
    g = np.random.default_rng(3)
    cases = {}
    # ragged: rows of 0..9 entries, rows 0, 5 and the last empty, duplicate columns (drawn with replacement), 23 x 31 (rectangular)
    m, n = 23, 31
    cnt = g.integers(0, 10, m)
    cnt[[0, 5, m - 1]] = 0
    rowptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    col = np.concatenate([np.sort(g.integers(0, n, c)) for c in cnt]).astype(np.int32)
    cases["ragged_rect_dups"] = (rowptr, col, n)
    # every row the same column four times
    m = 9
    cases["all_dups"] = (np.arange(m + 1, dtype=np.int64) * 4, np.repeat(g.integers(0, m, m), 4).astype(np.int32), m)
    # no entries at all
    cases["empty"] = (np.zeros(6, dtype=np.int64), np.zeros(0, dtype=np.int32), 4)
    # more rows than columns
    m, n = 40, 7
    cases["tall"] = (np.arange(m + 1, dtype=np.int64) * 3, g.integers(0, n, 3 * m).astype(np.int32), n)
    return cases


@pytest.mark.parametrize("name", ["ragged_rect_dups", "all_dups", "empty", "tall"])
def test_exact_reference_is_the_dense_product(name):
    rowptr, col, n = _small_cases()[name]
    if name == "ragged_rect_dups":
        assert any(np.unique(col[rowptr[i]:rowptr[i + 1]]).size < rowptr[i + 1] - rowptr[i] for i in range(rowptr.size - 1)), "no duplicate"
    val = R.int_values(col.size, seed=1)
    assert val.size == 0 or (np.abs(val).min() >= 1 and np.abs(val).max() <= 8)
    X = R.int_panel(n, 11)
    assert np.abs(X).max() <= 16 and (np.diff(X, axis=0) != 0).all() and (np.diff(X, axis=1) != 0).all()
    D, _ = R.dense_longdouble(rowptr, col, val, n)
    ref = D @ X.astype(LD)
    Y = R.spmm_exact_int(rowptr, col, val, X)
    assert Y.dtype == np.int64 and np.array_equal(Y.astype(LD), ref)
    empty = np.diff(rowptr) == 0
    assert (Y[empty] == 0).all()


@pytest.mark.parametrize("name", ["ragged_rect_dups", "all_dups", "empty", "tall"])
def test_longdouble_reference_is_the_dense_product(name):
    rowptr, col, n = _small_cases()[name]
    val = R.uniform_values(col.size, seed=2)
    X = R.uniform_panel(n, 11, seed=4)
    D, Dabs = R.dense_longdouble(rowptr, col, val, n)
    ref, refabs = D @ X.astype(LD), Dabs @ np.abs(X).astype(LD)
    Y, B = R.spmm_longdouble(rowptr, col, val, X)
    assert Y.dtype == LD and B.dtype == LD
    # the two differ by the order of at most n_i + n longdouble additions: (n_i + n) eps_ld |A||X|, far below the double bound
    nrow = np.diff(rowptr).astype(LD)[:, None]
    tol = (nrow + n) * np.finfo(LD).eps * refabs
    assert (np.abs(Y - ref) <= tol).all() and (np.abs(B - refabs) <= tol).all()
    empty = np.diff(rowptr) == 0
    assert (Y[empty] == 0).all() and (B[empty] == 0).all() and (R.spmm_bound(rowptr, B)[empty] == 0).all()


def test_exact_reference_refuses_non_integers():
    rowptr, col, n = _small_cases()["tall"]
    with pytest.raises(AssertionError):
        R.spmm_exact_int(rowptr, col, R.uniform_values(col.size, 1), R.int_panel(n, 3))


def test_a_double_product_meets_the_bound_and_a_dropped_term_does_not():
    """the derived bound holds for a plain double accumulation (np.add.reduceat in float64) and is tight enough to see one term of a
    row go missing"""
    from rails_amd import problems as P

    rowptr, col, _ = P.banded_random(600, 27, 40, seed=1)
    val = R.uniform_values(col.size, seed=2)
    X = R.uniform_panel(600, 9, seed=4)
    ref, B = R.spmm_longdouble(rowptr, col, val, X)
    bound = R.spmm_bound(rowptr, B)
    Yd = R._segment_sums(val[:, None] * X[col], rowptr, 600)
    assert (np.abs(Yd.astype(LD) - ref) <= bound).all()
    v2 = val.copy()
    v2[rowptr[1:] - 1] = 0.0  # the last entry of every row
    Ym = R._segment_sums(v2[:, None] * X[col], rowptr, 600)
    assert (np.abs(Ym.astype(LD) - ref) > bound).mean() > 0.99


def test_tile_statistics_of_the_device_cases():
    """what decides the form of the LDS-staged kernel for the matrices of tests/test_gpu_spmm_tiled.py, recomputed here for runs of 64
    rows: the longest row picks NNZ (<= 8, 16, 28, 32; more: no register kernel), the largest footprint picks NL (4 staging slots of
    256 threads x 4 pieces hold 256 rows of 8 columns, 8 hold 512) and the reuse must reach 1.8 for the plan to be accepted"""
    from rails_amd import problems as P

    want = {(12, 40): (12, 136, 5.9), (31, 40): (31, 143, 14.4), (27, 150): (27, 349, 5.2), (40, 60): (40, 182, 14.5), (32, 400): (32, 778, 2.9)}
    for (nnz, bw), (mr, fp, reuse) in want.items():
        rowptr, col, _ = P.banded_random(3000, nnz, bw, seed=1)
        st = R.tile_stats_host(rowptr, col)
        print(nnz, bw, st)
        assert st["max_row_nnz"] == mr and st["max_fp"] == fp and abs(st["reuse"] - reuse) < 0.06, ((nnz, bw), st)
    # variant 6 (16-column chunks: 8 pieces per row): NL = 4 needs a footprint of at most 128
    st = R.tile_stats_host(*P.banded_random(3000, 12, 30, seed=1)[:2])
    assert st["max_fp"] <= 128 and st["reuse"] >= 1.8, st
    # the ragged matrix: rows of 0..30 entries, accepted by the plan
    rowptr, col = R.ragged_banded(2990)
    cnt = np.diff(rowptr)
    assert 2990 % 64 and cnt[-1] == 0 and (cnt[::37] == 0).all() and cnt.max() <= 30 and cnt.max() > 16
    st = R.tile_stats_host(rowptr, col)
    assert st["reuse"] >= 1.8 and st["max_fp"] <= 256, st
    rowptr, col = R.ragged_banded(2990, long_row=(1500, 40))
    assert np.diff(rowptr).max() == 40 and R.tile_stats_host(rowptr, col)["reuse"] >= 1.8
