"""What the solution object X = U S U' (include/rails_solution.h) computes, restated in numpy longdouble, the slice rule of
rails_panel_rowquad (rails_amd/csrc/solution.hip) restated on the host, the componentwise bounds and the case lists the GPU tests share.
Not a test module: tests/test_solution_reference_host.py checks the lists and that the bounds can be met (numpy in plain double stays
inside them); tests/test_gpu_rowquad.py and tests/test_gpu_solution.py compare the device against it.

Bounds, derived and not tuned (gamma_n = n eps / (1 - n eps) bounds the error of an inner product of n terms in any order):
  rowquad / variance   an inner product of 2k terms per row: gamma_2k (|U||S||U|')_ii; 8 k eps leaves a factor 4 for the MFMA's internal
                       order and the reference's own error
  block                the same inner product for a pair of rows: 8 k eps (|U_r||S||U_c|')
  apply                U (S (U'W)): three factors with inner lengths m, k, k, gamma_(m+2k) (|U||S||U|'|W|)_ij; 4 (m + 2k) eps
  trace                sum_ij S_ij (U'U)_ji: k^2 terms, each an inner product of m: 4 (m + k^2) eps sum_ij |S_ij| (|U|'|U|)_ji

Exact cases: U and S integer-valued in [-3, 3], k <= 512.  |(U S)_ij| <= 9 k <= 4608, a term of the second reduction is at most 3 * 4608
and the whole sum at most 512 * 13824 = 7077888 < 2^53: every partial sum, in whatever order and fused or not, is an integer that a double
holds, so the device result must EQUAL the int64 einsum."""
import functools

import numpy as np

EPS = 2.0 ** -52
LD = np.longdouble
TRS = (2, 4, 8, 12, 16)  # the instantiations of k_panel_rowquad<TR>

# the k of the kernel tests: 0, the chunk edges (32 rows of S per LDS chunk) 31/32/33/64, every TR in one slice (1: 2, 33: 4, 128: 8,
# 129 and 192: 12, 193 and 256: 16), the slice edges 256/257/512 and the two-slice cases
K_LIST = (0, 1, 3, 4, 5, 31, 32, 33, 64, 128, 129, 192, 193, 256, 257, 270, 300, 384, 385, 512)
M_LIST = (1, 15, 16, 17, 127, 128, 129, 300)  # the 16-row wave tile and the 128-row workgroup, either side
K_SMALL_MAX = 64  # k above this is paired with m = 129 and m = 300 only
WINDOW_C0 = (0, 2, 3, 7, 16)
WINDOW_CASES = ((129, 5), (129, 45), (129, 257))  # (m, k) of the window / poison tests: vector head + scalar tail, one slice, two slices
BOUNDED_M = 129  # two workgroups, the second with one row
STALE_SEQUENCE = (500, 33, 300, 5)
OBJECT_M, OBJECT_K = 300, 40
APPLY_NC = (1, 16, 257)  # 257 > 256 takes rails_panel_gemm_wide


def slice_rule(k):
    """k -> [(j0, nc, TR), ...]: slices of equal width (a multiple of 16, at most 256 columns of S), TR the smallest instantiation that
    holds the slice's column tiles.  The first slice is never narrower than a later one, so TR never increases along the list."""
    if k == 0:
        return []
    nslices = (k + 255) // 256
    width = ((k + nslices - 1) // nslices + 15) // 16 * 16
    out = []
    for j0 in range(0, k, width):
        nc = min(width, k - j0)
        tiles = (nc + 15) // 16
        out.append((j0, nc, min(t for t in TRS if t >= tiles)))
    return out


def exact_ms(k):
    return M_LIST if k <= K_SMALL_MAX else (129, 300)


def exact_case(m, k):
    """integer-valued U (m x k) and S (k x k, not symmetric) in [-3, 3] and the int64 result"""
    g = np.random.default_rng(7919 * k + m)
    U = g.integers(-3, 4, (m, k))
    S = g.integers(-3, 4, (k, k))
    if k > 1 and np.array_equal(S, S.T):
        S[0, 1] = S[1, 0] + 1 if S[1, 0] < 3 else S[1, 0] - 1
    want = np.einsum("ij,jl,il->i", U.astype(np.int64), S.astype(np.int64), U.astype(np.int64))
    return U.astype(np.float64), S.astype(np.float64), want


def exact_partial_sum_limit(k):
    """the largest modulus a partial sum of an exact case can reach"""
    return k * 3 * (k * 9)


SINGLE_ENTRY_K = (33, 257, 300, 512)


def single_entry_pairs(k):
    """(a, b) with S[a, b] = 1 the only entry: either side of the tile edge 15|16, of the chunk edge 31|32 and of the slice edge, both
    orders, the corners and the last diagonal entry"""
    edges = [15, 31] + [s[0] - 1 for s in slice_rule(k)[1:]]
    pairs = []
    for e in edges:
        if e + 1 < k:
            pairs += [(e, e + 1), (e + 1, e)]
    return pairs + [(0, k - 1), (k - 1, 0), (k - 1, k - 1)]


def kernel_case(g, m, k):
    """the inputs of tests/test_gpu_solution.py::_kernel_case: rows scaled over six decades, S symmetric indefinite"""
    U = g.standard_normal((m, k)) * 10.0 ** g.uniform(-3, 3, (m, 1))
    S = g.standard_normal((k, k))
    return U, S + S.T


@functools.lru_cache(maxsize=None)
def bounded_case(m, k):
    """(U, S, the longdouble reference, the bound): computed once, shared by the tests that need it, read-only"""
    U, S = kernel_case(np.random.default_rng(1000 * k + m), m, k)
    for a in (U, S):
        a.setflags(write=False)
    want, bound = rowquad(U, S), rowquad_bound(U, S)
    want.setflags(write=False)
    bound.setflags(write=False)
    return U, S, want, bound


@functools.lru_cache(maxsize=None)
def object_problem(m=OBJECT_M, k=OBJECT_K):
    """as tests/test_gpu_solution.py::_object_problem at m rows: U of condition 1e2, not orthonormal; S symmetric"""
    g = np.random.default_rng(41)
    Q1 = np.linalg.qr(g.standard_normal((m, k)))[0]
    Q2 = np.linalg.qr(g.standard_normal((k, k)))[0]
    U = (Q1 * np.logspace(0, 2, k)) @ Q2.T
    S = g.standard_normal((k, k))
    S = S + S.T
    U.setflags(write=False)
    S.setflags(write=False)
    return U, S


def apply_rhs(m, nc):
    return np.random.default_rng(500 + nc).standard_normal((m, nc))


# rows with repeats and out of order, the first and the last row, single-element blocks
def block_cases(m):
    return (([0, 7, m - 1, 7, 150], [m - 1, 2, 3]), ([m - 1, 0], [0, m - 1]), ([0], [0]), ([m - 1], [m - 1]), ([17], [m - 1]), ([5, 5, 5], [9]))


# ---- the operations in longdouble ------------------------------------------------------------------------------------------------------
def _ld(a):
    return np.asarray(a, dtype=LD)


def rowquad(U, S):
    U, S = _ld(U), _ld(S)
    return ((U @ S) * U).sum(axis=1) if U.shape[1] else np.zeros(U.shape[0], dtype=LD)


def apply(U, S, W):
    U, S, W = _ld(U), _ld(S), _ld(W)
    return U @ (S @ (U.T @ W))


def trace(U, S):
    U, S = _ld(U), _ld(S)
    return (S * (U.T @ U).T).sum()


def block(U, S, rows, cols):
    U, S = _ld(U), _ld(S)
    return U[np.asarray(rows)] @ S @ U[np.asarray(cols)].T


# ---- the bounds (double) -----------------------------------------------------------------------------------------------------------------
def rowquad_bound(U, S):
    k = U.shape[1]
    return np.asarray(8 * k * EPS * rowquad(np.abs(U), np.abs(S)), dtype=np.float64)


def block_bound(U, S, rows, cols):
    return np.asarray(8 * U.shape[1] * EPS * block(np.abs(U), np.abs(S), rows, cols), dtype=np.float64)


def apply_bound(U, S, W):
    m, k = U.shape
    return np.asarray(4 * (m + 2 * k) * EPS * apply(np.abs(U), np.abs(S), np.abs(W)), dtype=np.float64)


def trace_bound(U, S):
    m, k = U.shape
    return float(4 * (m + k * k) * EPS * trace(np.abs(U), np.abs(S)))


# ---- the same in plain double, as numpy does it (the host test: the bounds can be met) --------------------------------------------------
def rowquad_double(U, S):
    return np.einsum("ij,ij->i", U @ S, U)


def apply_double(U, S, W):
    return U @ (S @ (U.T @ W))


def trace_double(U, S):
    return float((S * (U.T @ U).T).sum())


def block_double(U, S, rows, cols):
    return U[np.asarray(rows)] @ S @ U[np.asarray(cols)].T


# ---- bit patterns ------------------------------------------------------------------------------------------------------------------------
def bits(a):
    """the uint64 bit patterns of a float64 array (a copy in the array's own layout)"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def special_data(g, m, n):
    """m x n doubles (column-major) of every kind a row move or a transfer must carry unchanged: normal numbers, -0.0, +-inf, quiet NaNs with
    distinct payloads and either sign, subnormals"""
    X = g.standard_normal((m, n))
    u = np.ascontiguousarray(X).view(np.uint64).ravel()
    pos = g.permutation(u.size)
    kinds = (lambda q: 0x8000000000000000, lambda q: 0x7FF0000000000000, lambda q: 0xFFF0000000000000,
             lambda q: 0x7FF8000000000000 | (0x1234500 + q), lambda q: 0xFFF8000000000000 | (0xABC00 + 3 * q),
             lambda q: 1 + q, lambda q: 0x800FFFFFFFFFFFFF - q)
    for q, p in enumerate(pos[:max(1, u.size // 3)]):
        u[p] = kinds[q % len(kinds)](q)
    return np.asfortranarray(u.view(np.float64).reshape(m, n))
