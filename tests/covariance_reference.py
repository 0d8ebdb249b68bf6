"""What the pair and map entries of the solution object X = U S U' compute (include/rails_solution.h: rails_panel_rowpair,
rails_solution_pairs, rails_solution_maps), restated in numpy longdouble, with the componentwise bounds and the case lists the tests share.
Not a test module: tests/test_covariance_host.py checks that the bounds can be met (numpy in plain double stays inside them) and runs the
C++ fallback against it; the GPU tests compare the device against it.  tests/solution_reference.py has the slice rule, the exact integer
cases and the bit helpers; this module builds on it.

Bounds, derived and not tuned.  eps = 2^-52, tau = 8 k eps.
  pairs, covariance maps   X[a, b] is an inner product of 2k terms, as the variance is: gamma_2k (|U_a||S||U_b|'); tau leaves the factor 4 of
                           solution_reference.rowquad_bound for the MFMA's internal order and the reference's own error.  The maps' U (S U_r')
                           is the same inner product bracketed the other way; the bound does not depend on the bracketing.
  correlation maps         c = C / sqrt(v_i v_j) with computed C = C (1 + d_C), v = v (1 + d_v), |d_C| <= tau Cbar / |C|, |d_v| <= tau Vbar / v
                           (Cbar, Vbar: the forms on |U|, |S|).  To first order  dc = c (d_C - d_vi / 2 - d_vj / 2), so
                             |dc| <= tau [ Cbar / sqrt(v_i v_j) + |c| (Vbar_i / v_i + Vbar_j / v_j) / 2 ],
                           doubled for the second-order terms (valid while tau Vbar / v < 1e-6, which corr_problem's S = L L' + I gives and
                           test_covariance_host.py checks), plus 4 eps |c| for two roots, their product and the quotient (half an ulp each =
                           eps / 2 each, doubled).  Where a variance is not > 0 the entry is 0; at the reference unknown itself it is 1.
Exact cases: solution_reference.exact_case's integer U and S with index patterns: every partial sum of U_a S U_b' is an integer below 2^53
whatever the rows are, so the device must EQUAL the int64 result."""
import functools

import numpy as np

import solution_reference as R

EPS = R.EPS
LD = R.LD

PAIR_MS = (1, 15, 16, 17, 127, 128, 129)  # the 16-row wave tile and the 128-row workgroup, either side
PATTERNS = ("identity", "reversed", "last", "repeats", "differ", "ia_null", "ib_null")
MAP_Q = (1, 16, 17, 64)
MAP_M = (1, 129, 4097)
MAP_K = (1, 33, 257)


def pair_ns(m):
    return (0, 1, 16, 17, 129, 2 * m)


def pattern(name, m, n, seed=0):
    """(ia, ib, n) for an index pattern on m rows; None = the identity (a NULL array in the call), which caps n at m"""
    g = np.random.default_rng(1000003 * m + 101 * n + seed)
    i = np.arange(n, dtype=np.int64)
    if name == "identity":
        ia = ib = i % m
    elif name == "reversed":
        ia = ib = (m - 1 - i) % m
    elif name == "last":
        ia = ib = np.full(n, m - 1, dtype=np.int64)
    elif name == "repeats":
        ia = ib = (i // 3) % m
    elif name == "differ":
        ia, ib = g.integers(0, m, n), g.integers(0, m, n)
        if n and m > 1:
            ib[0] = (ia[0] + 1) % m  # at least one pair off the diagonal
    elif name in ("ia_null", "ib_null"):
        n = min(n, m)
        idx = g.integers(0, m, n)
        ia, ib = (None, idx) if name == "ia_null" else (idx, None)
    else:
        raise ValueError(name)
    as32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32)
    return as32(ia), as32(ib), n


def _rows(idx, n):
    return np.arange(n) if idx is None else np.asarray(idx, dtype=np.int64)


def exact_pairs(U, S, ia, ib, n):
    """the int64 result for integer-valued U and S"""
    Ui, Si = U.astype(np.int64), S.astype(np.int64)
    return np.einsum("ij,jl,il->i", Ui[_rows(ia, n)], Si, Ui[_rows(ib, n)]) if n else np.zeros(0, dtype=np.int64)


# ---- the operations in longdouble ------------------------------------------------------------------------------------------------------
def _ld(a):
    return np.asarray(a, dtype=LD)


def pairs(U, S, ia, ib, n=None):
    n = n if n is not None else (ia if ia is not None else ib).size
    U, S = _ld(U), _ld(S)
    return ((U[_rows(ia, n)] @ S) * U[_rows(ib, n)]).sum(axis=1) if U.shape[1] else np.zeros(n, dtype=LD)


def maps(U, S, rows):
    U, S = _ld(U), _ld(S)
    return U @ (S @ U[np.asarray(rows, dtype=np.int64)].T)


def correlations(U, S, rows):
    """longdouble correlation maps with the zero rule and the unit rule of rails_solution_maps"""
    rows = np.asarray(rows, dtype=np.int64)
    C, v = maps(U, S, rows), R.rowquad(U, S)
    ok = (v[:, None] > 0) & (v[rows][None, :] > 0)
    den = np.sqrt(np.where(ok, v[:, None] * v[rows][None, :], LD(1)))
    out = np.where(ok, C / den, LD(0))
    for j, r in enumerate(rows):
        if v[r] > 0:
            out[r, j] = LD(1)
    return out


# ---- the bounds (double) -----------------------------------------------------------------------------------------------------------------
def tau(k):
    return 8 * k * EPS


def pairs_bound(U, S, ia, ib, n=None):
    return np.asarray(tau(U.shape[1]) * pairs(np.abs(U), np.abs(S), ia, ib, n), dtype=np.float64)


def maps_bound(U, S, rows):
    return np.asarray(tau(U.shape[1]) * maps(np.abs(U), np.abs(S), rows), dtype=np.float64)


def variance_ratio(U, S):
    """tau Vbar / v per row (0 where v is not > 0): the relative error bound of a computed variance"""
    v, vbar = R.rowquad(U, S), R.rowquad(np.abs(U), np.abs(S))
    return np.asarray(np.where(v > 0, tau(U.shape[1]) * vbar / np.where(v > 0, v, LD(1)), LD(0)), dtype=np.float64)


def correlations_bound(U, S, rows):
    rows = np.asarray(rows, dtype=np.int64)
    k = U.shape[1]
    c = np.abs(correlations(U, S, rows))
    v, vbar = R.rowquad(U, S), R.rowquad(np.abs(U), np.abs(S))
    cbar = maps(np.abs(U), np.abs(S), rows)
    ok = (v[:, None] > 0) & (v[rows][None, :] > 0)
    safe = np.where(v > 0, v, LD(1))
    rel = vbar / safe
    first = cbar / np.sqrt(safe[:, None] * safe[rows][None, :]) + c * (rel[:, None] + rel[rows][None, :]) / 2
    return np.asarray(np.where(ok, 2 * tau(k) * first + 4 * EPS * c, LD(0)), dtype=np.float64)


# ---- the same in plain double, as numpy does it (the host test: the bounds can be met) --------------------------------------------------
def pairs_double(U, S, ia, ib, n=None):
    n = n if n is not None else (ia if ia is not None else ib).size
    return np.einsum("ij,ij->i", U[_rows(ia, n)] @ S, U[_rows(ib, n)])


def maps_double(U, S, rows):
    return U @ (S @ U[np.asarray(rows, dtype=np.int64)].T)


def correlations_double(U, S, rows):
    rows = np.asarray(rows, dtype=np.int64)
    C, v = maps_double(U, S, rows), R.rowquad_double(U, S)
    ok = (v[:, None] > 0) & (v[rows][None, :] > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where(ok, C / (np.sqrt(np.where(v > 0, v, 1.0))[:, None] * np.sqrt(np.where(v > 0, v, 1.0))[rows][None, :]), 0.0)
    for j, r in enumerate(rows):
        if v[r] > 0:
            out[r, j] = 1.0
    return out


# ---- shared problems ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pair_problem(m, k):
    """random real U (rows scaled over six decades) and a NON-symmetric S: read-only"""
    g = np.random.default_rng(31 * k + m)
    U = g.standard_normal((m, k)) * 10.0 ** g.uniform(-3, 3, (m, 1))
    S = g.standard_normal((k, k))
    U.setflags(write=False)
    S.setflags(write=False)
    return U, S


def map_rows(m, q, seed=0):
    """q reference unknowns of m rows: the first, the last, then random ones (with repeats when q > m)"""
    g = np.random.default_rng(77 * m + q + seed)
    rows = np.concatenate([[0, m - 1], g.integers(0, m, max(0, q - 2))])[:q]
    return np.ascontiguousarray(rows, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def corr_problem(m, k, zero_row=None):
    """U random, S = L L' + I with integer L in [-2, 2] (positive definite: variances well away from cancellation); zero_row: that row of
    U is all zero.  Read-only."""
    g = np.random.default_rng(5 * m + 13 * k)
    U = g.standard_normal((m, k))
    if zero_row is not None:
        U[zero_row] = 0.0
    L = g.integers(-2, 3, (k, k)).astype(np.float64)
    S = L @ L.T + np.eye(k)
    U.setflags(write=False)
    S.setflags(write=False)
    return U, S
