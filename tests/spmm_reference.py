"""Host references, derived bounds and input generators for the CSR x panel product Y = A X (rails_amd/csrc/spmm.hip, spmm_tiled.hip;
the tile plan: tile_plan.cpp).  numpy only,
no project imports: a host test and a device test can share everything in here.

Two references, for two kinds of input.

  exact    val integers in [-8, 8] without 0, X integers in [-16, 16].  A row of n <= 40 entries sums products of magnitude <= 128:
           every partial sum is an integer below 2^13, an exact double whatever the order and whether or not the multiply-adds are
           fused.  A correct kernel therefore returns spmm_exact_int() bit for bit; one wrong, missing or doubled term shows as a
           difference of at least 1.
  bounded  val and X uniform on (-1, 1).  spmm_longdouble() returns the product and B = |A| |X|, both accumulated in np.longdouble
           (64-bit significand: its own error is 2^-11 of a double's).  A chain of n fused multiply-adds in any order has
           |fl(y) - y| <= gamma(n) sum |a||x| with gamma(n) = n u / (1 - n u), u = 2^-53 (Higham, Accuracy and Stability of Numerical
           Algorithms, section 3.1; a fused multiply-add rounds once, so n roundings).  spmm_bound() is 2 n_i u B_ij: the factor 2 is
           slack for gamma(n) against n u and for the reference.  Entries with a zero coefficient (padding) add exact zeros.  Rows
           without entries have B = 0: they must come back as exactly 0.

tile_stats_host() recomputes on the host what the LDS-staged kernel's plan finds for runs of consecutive rows: the footprint of a
tile is the number of distinct columns its rows touch, the reuse nonzeros per footprint entry."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53


def _rows_of(rowptr):
    rowptr = np.asarray(rowptr, dtype=np.int64)
    cnt = np.diff(rowptr)
    return rowptr, cnt, np.flatnonzero(cnt > 0)


def _segment_sums(prod, rowptr, m):
    """row sums of prod (nnz x nc, rows of A consecutive) -> m x nc; rows without entries stay 0"""
    rowptr, cnt, nonempty = _rows_of(rowptr)
    Y = np.zeros((m, prod.shape[1]), dtype=prod.dtype)
    if nonempty.size:
        Y[nonempty] = np.add.reduceat(prod, rowptr[:-1][nonempty], axis=0)
    return Y


def spmm_exact_int(rowptr, col, val, X):
    """A X in int64 for integer-valued val and X (checked)."""
    vi = np.rint(np.asarray(val)).astype(np.int64)
    Xi = np.rint(np.asarray(X)).astype(np.int64)
    assert np.array_equal(vi, np.asarray(val)) and np.array_equal(Xi, np.asarray(X)), "spmm_exact_int: inputs are not integers"
    m = len(rowptr) - 1
    col = np.asarray(col, dtype=np.int64)
    Y = np.zeros((m, Xi.shape[1]), dtype=np.int64)
    for c0 in range(0, Xi.shape[1], 32):
        Y[:, c0:c0 + 32] = _segment_sums(vi[:, None] * Xi[col, c0:c0 + 32], rowptr, m)
    return Y


def spmm_longdouble(rowptr, col, val, X):
    """(A X, |A| |X|), both accumulated in np.longdouble."""
    m = len(rowptr) - 1
    col = np.asarray(col, dtype=np.int64)
    v = np.asarray(val, dtype=LD)
    Xl = np.asarray(X, dtype=LD)
    Y = np.zeros((m, Xl.shape[1]), dtype=LD)
    B = np.zeros((m, Xl.shape[1]), dtype=LD)
    for c0 in range(0, Xl.shape[1], 32):
        g = Xl[col, c0:c0 + 32]
        Y[:, c0:c0 + 32] = _segment_sums(v[:, None] * g, rowptr, m)
        B[:, c0:c0 + 32] = _segment_sums(np.abs(v)[:, None] * np.abs(g), rowptr, m)
    return Y, B


def spmm_bound(rowptr, B):
    """2 n_i u B_ij (module docstring)"""
    n = np.diff(np.asarray(rowptr, dtype=np.int64)).astype(LD)
    return 2.0 * n[:, None] * LD(U) * B


def dense_longdouble(rowptr, col, val, ncols):
    """A and |A| (entry by entry: duplicates of a column add up in both) as dense longdouble matrices"""
    rowptr, cnt, _ = _rows_of(rowptr)
    m = rowptr.size - 1
    rows = np.repeat(np.arange(m), cnt)
    D = np.zeros((m, ncols), dtype=LD)
    Dabs = np.zeros((m, ncols), dtype=LD)
    np.add.at(D, (rows, np.asarray(col, dtype=np.int64)), np.asarray(val, dtype=LD))
    np.add.at(Dabs, (rows, np.asarray(col, dtype=np.int64)), np.abs(np.asarray(val, dtype=LD)))
    return D, Dabs


# ------------------------------------------------------------------------------------------------------------------ inputs
def int_values(n, seed):
    """n integers in [-8, 8] without 0"""
    g = np.random.default_rng(seed)
    v = g.integers(1, 9, n) * g.choice(np.array([-1, 1]), n)
    return v.astype(np.float64)


def int_panel(rows, nc):
    """rows x nc integers in [-16, 16]; entries next to each other in a row or a column differ (by 3..11 down a column, 9..17 along a
    row, modulo 33), so a kernel that reads the neighbouring X row or column cannot get the sum right by accident"""
    i = np.arange(rows, dtype=np.int64)[:, None]
    j = np.arange(nc, dtype=np.int64)[None, :]
    return (((7 * i + 13 * j + (i * j) % 5) % 33) - 16).astype(np.float64)


def uniform_values(n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n)


def uniform_panel(rows, nc, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (rows, nc))


def ragged_banded(m, band=60, max_len=30, every=37, seed=5, long_row=None, empty_tail=1):
    """Rows of 0..max_len entries with columns in |j - i| <= band (sorted, no duplicates inside a row); every `every`-th row and the
    last empty_tail rows are empty.  long_row = (row, n): that row gets n entries instead."""
    g = np.random.default_rng(seed)
    rowptr = [0]
    cols = []
    for i in range(m):
        n = int(g.integers(0, max_len + 1))
        if i % every == 0 or i >= m - empty_tail:
            n = 0
        if long_row is not None and i == long_row[0]:
            n = long_row[1]
        lo, hi = max(0, i - band), min(m - 1, i + band)
        c = np.sort(g.choice(np.arange(lo, hi + 1), size=n, replace=False))
        cols.append(c)
        rowptr.append(rowptr[-1] + n)
    return np.asarray(rowptr, dtype=np.int64), np.concatenate(cols).astype(np.int32)


def tile_stats_host(rowptr, col, rows=64):
    """what the tile plan finds for runs of `rows` consecutive rows: dict(max_row_nnz, max_fp, reuse)"""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    m = rowptr.size - 1
    fp_total, max_fp = 0, 0
    for r0 in range(0, m, rows):
        f = np.unique(col[rowptr[r0]:rowptr[min(m, r0 + rows)]]).size
        fp_total += f
        max_fp = max(max_fp, f)
    return {"max_row_nnz": int(np.diff(rowptr).max()), "max_fp": max_fp, "reuse": float(rowptr[-1]) / max(1, fp_total)}
