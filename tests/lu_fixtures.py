"""Factors with a known level structure for the tests of the device LU solves (rails_amd/csrc/splu.hip, sptrsv.hip), a restatement
of the host level analysis and launch plan of splu.hip, and a level-by-level substitution on the host in any floating-point type:
the reference of tests/test_gpu_lu_levels.py.  Nothing here calls the library.

Conventions (scipy's SuperLU object): Pr A Pc = L U with Pr[perm_r[i], i] = 1 and Pc[i, perm_c[i]] = 1, that is
A[i, j] = (L U)[perm_r[i], perm_c[j]].  So A x = b is  L U y = c  with c[perm_r[i]] = b[i], x[j] = y[perm_c[j]],  and A' x = b is
U' L' y = c  with c[perm_c[j]] = b[j], x[i] = y[perm_r[i]]."""
import collections

import numpy as np
import scipy.sparse as sp

NARROW = 1024  # RAILS_LU_NARROW of splu.hip: a level of more rows than this gets a launch of its own
SPTRSV_WORK = 1024  # sptrsv.hip: a level goes to k_sptrsv_level when rows * columns exceed this

LevelPlan = collections.namedtuple("LevelPlan", "widths pattern launches order")


def _strict(T):
    """CSR arrays of a triangle without its diagonal, columns sorted (stored zeros stay: the library keeps them too), and the diagonal"""
    C = sp.coo_matrix(T)
    off = C.row != C.col
    n = C.shape[0]
    d = np.zeros(n)
    np.add.at(d, C.row[~off], C.data[~off])
    rows, cols, data = C.row[off], C.col[off], C.data[off]
    o = np.lexsort((cols, rows))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64)
    return rp, cols[o].astype(np.int64), data[o].astype(np.float64), d


def level_plan(T, lower):
    """The level analysis and the segment plan of splu.hip's tri_create for the triangle T (its diagonal is ignored): level(i) = 1 +
    the largest level among the rows that row i's off-diagonal entries name.  widths: rows per level; pattern: 'W' for a level of
    more than 1024 rows (one k_lu_level launch), 'r' for a maximal run of narrower levels (one k_lu_run launch); launches =
    len(pattern), what one sweep over the triangle launches; order: the rows of each level, ascending."""
    rp, ci, _, _ = _strict(T)
    n = rp.size - 1
    level = np.zeros(n, dtype=np.int64)
    for i in (range(n) if lower else range(n - 1, -1, -1)):
        c = ci[rp[i]:rp[i + 1]]
        assert np.all(c < i) if lower else np.all(c > i), "not a %s triangle" % ("lower" if lower else "upper")
        level[i] = level[c].max() + 1 if c.size else 0
    widths = np.bincount(level)
    pattern = ""
    for w in widths:
        if w > NARROW:
            pattern += "W"
        elif not pattern.endswith("r"):
            pattern += "r"
    order = [np.flatnonzero(level == l) for l in range(widths.size)]
    return LevelPlan([int(w) for w in widths], pattern, len(pattern), order)


def sptrsv_plan(T, lower, nc):
    """the same for sptrsv.hip's rails_sptrsv_solve at nc columns: 'W' a k_sptrsv_level launch (rows * nc > 1024), 'r' a chain"""
    pattern = ""
    for w in level_plan(T, lower).widths:
        if w * nc > SPTRSV_WORK:
            pattern += "W"
        elif not pattern.endswith("r"):
            pattern += "r"
    return pattern


class Factors:
    """What SparseLU(ctx, F.A, lu=F) and DeviceLU(ctx, F) read of a SuperLU object -- L (unit lower, its ones stored), U, perm_r,
    perm_c, shape -- plus the matrix A itself."""

    def __init__(self, L, U, perm_r, perm_c, A=None):
        self.L, self.U = sp.csc_matrix(L), sp.csc_matrix(U)
        self.perm_r, self.perm_c = np.asarray(perm_r, dtype=np.int32), np.asarray(perm_c, dtype=np.int32)
        self.shape = self.L.shape
        self.n = self.shape[0]
        if A is None:  # A[i, j] = (L U)[perm_r[i], perm_c[j]]
            A = sp.csr_matrix(self.L @ self.U)[self.perm_r][:, self.perm_c]
        self.A = sp.csr_matrix(A)
        self._tri = {}

    def triangles(self, trans):
        """the two triangles of a solve in sweep order, as (T, lower): L, U for A^-1; U', L' for A^-T"""
        return ((self.U.T, True), (self.L.T, False)) if trans else ((self.L, True), (self.U, False))

    def plans(self, trans):
        return [level_plan(T, lower) for T, lower in self.triangles(trans)]

    def launches(self, trans):
        """launches of one rails_lu_solve"""
        return sum(p.launches for p in self.plans(trans))

    def _host_tri(self, trans, k):
        key = (bool(trans), k)
        if key not in self._tri:
            T, lower = self.triangles(trans)[k]
            rp, ci, va, d = _strict(T)
            levels = []
            for rows in level_plan(T, lower).order:
                cnt = rp[rows + 1] - rp[rows]
                q = np.concatenate([np.arange(rp[r], rp[r + 1]) for r in rows]) if cnt.sum() else np.zeros(0, dtype=np.int64)
                levels.append((rows, q, np.repeat(np.arange(rows.size), cnt)))
            self._tri[key] = (ci, va, d, levels)
        return self._tri[key]

    def solve(self, X, trans=False, rows=None, dtype=np.longdouble, reverse=False):
        """(A^-1 E X)[rows] (trans: A^-T), E putting X on `rows` and zeros elsewhere (rows None: all), by level-by-level substitution
        in `dtype`: every product and every sum is rounded to dtype, a row's products are summed first, in the order of its columns
        (reverse: in the opposite order), and taken from the right-hand side then.  Returns an array of dtype."""
        X = np.asarray(X)
        n, nc = self.n, X.shape[1]
        E = np.zeros((n, nc), dtype=dtype)
        E[np.arange(n) if rows is None else rows] = X
        pin, pout = (self.perm_c, self.perm_r) if trans else (self.perm_r, self.perm_c)
        W = np.zeros((n, nc), dtype=dtype)
        W[pin] = E
        for k in (0, 1):
            ci, va, d, levels = self._host_tri(trans, k)
            va, d = va.astype(dtype), d.astype(dtype)
            for lrows, q, rid in levels:
                part = np.zeros((lrows.size, nc), dtype=dtype)
                if q.size:
                    if reverse:
                        q, rid = q[::-1], rid[::-1]
                    np.add.at(part, rid, va[q, None] * W[ci[q]])
                W[lrows] = (W[lrows] - part) / d[lrows, None]
        Y = W[pout]
        return Y if rows is None else Y[rows]


def _perms(n, seed):
    g = np.random.default_rng([seed, 7, n])
    return g.permutation(n), g.permutation(n)


def _blocks(nb, bs, seed):
    """nb diagonally dominant bs x bs blocks (off the diagonal uniform in (-1, 1), on it +-4) and their unpivoted Doolittle factors;
    the first blocks of a longer sequence with the same seed are the same blocks"""
    B = np.random.default_rng([seed, 1]).uniform(-1.0, 1.0, (nb, bs, bs))
    sign = np.where(np.random.default_rng([seed, 2]).random((nb, bs)) < 0.5, -1.0, 1.0)
    k = np.arange(bs)
    B[:, k, k] = 4.0 * sign
    L, U = np.zeros_like(B), B.copy()
    L[:, k, k] = 1.0
    for j in range(bs - 1):  # Doolittle: eliminate column j of every block at once
        L[:, j + 1:, j] = U[:, j + 1:, j] / U[:, j, j][:, None]
        U[:, j + 1:, :] -= L[:, j + 1:, j][:, :, None] * U[:, j, :][:, None, :]
        U[:, j + 1:, j] = 0.0
    return B, L, U


def block_factors(nb, bs, seed):
    """Factors of a block-diagonal matrix of nb bs x bs blocks, made here (no library factorises anything), with random perm_r and
    perm_c folded into the matrix so that Pr A Pc = L U.  Every triangle has bs levels of nb rows."""
    _, L, U = _blocks(nb, bs, seed)
    perm_r, perm_c = _perms(nb * bs, seed)
    Ls, Us = sp.block_diag(list(L), format="csc"), sp.block_diag(list(U), format="csc")
    Ls.eliminate_zeros()  # block_diag stores the zeros of the dense blocks
    Us.eliminate_zeros()
    return Factors(Ls, Us, perm_r, perm_c)


def bordered_blocks(nb=1100, bs=3, border=6, seed=3, density=0.3):
    """The same blocks with `border` more rows and columns, each coupled to a random `density` of the block rows, factored by scipy's
    SuperLU.  L and U' keep the blocks' levels of nb rows and add one level per border row; in U and L' a block row waits for the
    first border column it is coupled to, which spreads the rows over the levels: one wide level between two runs at the default
    sizes."""
    import scipy.sparse.linalg as spla

    B, _, _ = _blocks(nb, bs, seed)
    g = np.random.default_rng([seed, 3])
    n0 = nb * bs
    E = np.where(g.random((n0, border)) < density, g.uniform(-1.0, 1.0, (n0, border)), 0.0)
    F = np.where(g.random((border, n0)) < density, g.uniform(-1.0, 1.0, (border, n0)), 0.0)
    G = g.uniform(-1.0, 1.0, (border, border)) + np.diag(np.abs(F).sum(axis=1) + border)
    A = sp.bmat([[sp.block_diag(list(B), format="csr"), sp.csr_matrix(E)], [sp.csr_matrix(F), sp.csr_matrix(G)]], format="csc")
    lu = spla.splu(A)
    return Factors(lu.L, lu.U, lu.perm_r, lu.perm_c, A=A)


def dyadic_factors(n=3400, seed=1, sizes_L=(1500, 900, 1000), sizes_U=(900, 1500, 1000)):
    """Hand-built factors on which a solve with small integer right-hand sides is exact in fp64 in any summation order: L unit
    lower, U upper with a diagonal of +-0.5, 1, 2, 4, entries off the diagonals +-0.5 or +-0.25, three levels per triangle
    (sizes_L: rows of L's levels 0, 1, 2 from the top; sizes_U: rows of U's levels 0, 1, 2 from the bottom), every row of a level
    named by a row of the next one, so that the transposes have the same three levels in the opposite order.  Most rows and
    columns hold 1 to 6 entries.  Every 37th row of the second and third level draws 17 to 40, every 41st draws 16, and every 53rd
    column is named by 17 to 40 more rows: several lanes of a row's group and the whole butterfly take part, in the transposed
    solve too.  With right-hand sides in [-8, 8] every intermediate is below 2^25 and a multiple of 2^-14."""
    assert sum(sizes_L) == n and sum(sizes_U) == n
    g = np.random.default_rng([seed, 5])
    vals = np.array([0.5, -0.5, 0.25, -0.25])

    def strict_lower(sizes):
        """rows, columns of a strictly lower pattern with levels of the given sizes from the top"""
        b = np.concatenate([[0], np.cumsum(sizes)])
        rr, cc = [], []
        for lv in (1, 2):
            lo, hi = b[lv], b[lv + 1]  # rows of this level; they name rows of the level before, [b[lv - 1], lo), and any earlier
            prev = np.arange(b[lv - 1], lo)
            for j in prev:  # every row of the level before is named by a row of this one
                rr.append(lo + (j - b[lv - 1]) % (hi - lo))
                cc.append(j)
            for i in range(lo, hi):
                k = i - lo
                cnt = int(g.integers(17, 41)) if k % 37 == 5 else 16 if k % 41 == 7 else int(g.integers(1, 7))
                cols = set(g.choice(prev, size=min(cnt, prev.size), replace=False).tolist())
                if lv == 2 and k % 3 == 0:  # and some of level 0 directly
                    cols |= set(g.choice(np.arange(0, b[1]), size=2, replace=False).tolist())
                rr += [i] * len(cols)
                cc += sorted(cols)
            for j in prev[3::53]:  # and some rows are named by 17 to 40 rows: long rows for the transposed triangle
                hub = g.choice(np.arange(lo, hi), size=int(g.integers(17, 41)), replace=False)
                rr += hub.tolist()
                cc += [j] * hub.size
        M = sp.coo_matrix((np.ones(len(rr)), (rr, cc)), shape=(n, n)).tocsr()  # duplicates add up
        M.data = g.choice(vals, M.nnz)
        return M

    L = strict_lower(sizes_L) + sp.identity(n, format="csr")
    # U: the mirror image of such a pattern (row i <-> n - 1 - i), so its levels count from the bottom
    S = strict_lower(sizes_U).tocoo()
    U = sp.coo_matrix((S.data, (n - 1 - S.row, n - 1 - S.col)), shape=(n, n)).tocsr()
    U = U + sp.diags(g.choice(np.array([0.5, -0.5, 1.0, -1.0, 2.0, -2.0, 4.0, -4.0]), n))
    perm_r, perm_c = _perms(n, seed)
    return Factors(L, U, perm_r, perm_c)


def permutation_matrices(F):
    """Pr, Pc as scipy's documentation of SuperLU writes them"""
    n = F.n
    Pr = sp.csc_matrix((np.ones(n), (F.perm_r, np.arange(n))), shape=(n, n))
    Pc = sp.csc_matrix((np.ones(n), (np.arange(n), F.perm_c)), shape=(n, n))
    return Pr, Pc
