"""Row partitions whose ghost-row plans are not the neighbour-to-neighbour plans of a balanced banded block: a rank that only sends and
one that only receives, an empty rank the exchange jumps over, every rank exchanging with every other, boundary rows in the middle of a
block, a rank of one row.  Not a test module and no GPU in here (numpy, scipy, rails_amd.partition): tests/test_partition_plans_host.py
pins the plans on the CPU, tests/test_gpu_partition_plans.py runs them.

A problem is the CSR triple (rowptr, col_global, val) of the undivided matrix plus `starts`.  The values are integers in [-8, 8] without 0
(spmm_reference.int_values) and the panels are spmm_reference.int_panel, so spmm_reference.spmm_exact_int is the bit-for-bit reference of
every product whatever the order of a row's terms -- on a partition that order changes, the ghost columns are numbered behind the local
ones.  The two problems the solves run on also carry a float matrix (`matrix`).

plans(p) makes every rank's HaloPlan without threads: every rank's requests first, then HaloPlan with them as its all_gather_object.
interior(...) restates rails_csr_set_halo's walk, overlaps(...) the condition of rails_halo_order (op_choice.h)."""
import numpy as np

import spmm_reference as R

NAMES = ("one_way", "wrap_skip", "all_to_all", "scattered", "unequal")
ONE_WAY_SEED = 449  # with this seed 36 of the 40 rows above a cut are referenced from below it, the last time from the cut's 39th and 40th row


class Problem:
    def __init__(self, name, starts, rowptr, col, val, matrix=None):
        self.name = name
        self.starts = np.asarray(starts, dtype=np.int64)
        self.rowptr = np.asarray(rowptr, dtype=np.int64)
        self.col = np.asarray(col, dtype=np.int64)
        self.val = np.asarray(val, dtype=np.float64)
        self.matrix = matrix  # scipy CSR with float values on the same pattern, where a solve runs on the problem
        self.m = int(self.starts[-1])
        self.nranks = self.starts.size - 1
        assert self.rowptr.size == self.m + 1 and self.col.size == self.val.size == self.rowptr[-1]
        for a in (self.starts, self.rowptr, self.col, self.val):
            a.setflags(write=False)

    @property
    def triple(self):
        return self.rowptr, self.col, self.val

    def block(self, r):
        """rows of rank r, global columns (rails_amd.problems.csr_rows)"""
        r0, r1 = int(self.starts[r]), int(self.starts[r + 1])
        p0, p1 = self.rowptr[r0], self.rowptr[r1]
        return self.rowptr[r0:r1 + 1] - p0, self.col[p0:p1], self.val[p0:p1]


def _from_rows(rows):
    """rows: per row a sorted array of columns -> rowptr, col"""
    rowptr = np.zeros(len(rows) + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum([len(r) for r in rows])
    return rowptr, np.concatenate(rows).astype(np.int64)


def _pattern_matrix(rowptr, col, val):
    import scipy.sparse as sp

    m = rowptr.size - 1
    A = sp.csr_matrix((val, col, rowptr), shape=(m, m))
    A.sort_indices()
    return A


def _one_way(seed=ONE_WAY_SEED):
    """3 x 2048 rows; row i has the diagonal and eight columns drawn from [i - 40, i] (below 0 dropped, repeats merged): nothing points
    to a later row, so rank 0 only sends and rank 2 only receives.  The float matrix: the integer values off the diagonal, 1 + the sum of
    their magnitudes on it (strictly diagonally dominant, lower triangular)."""
    m = 3 * 2048
    g = np.random.default_rng(seed)
    off = g.integers(0, 41, size=(m, 8))
    rows = []
    for i in range(m):
        c = np.unique(np.concatenate([i - off[i], [i]]))
        rows.append(c[c >= 0])
    rowptr, col = _from_rows(rows)
    val = R.int_values(col.size, seed=11)
    fv = val.copy()
    row_of = np.repeat(np.arange(m), np.diff(rowptr))
    diag = col == row_of
    fv[diag] = 0.0
    fv[diag] = 1.0 + np.add.reduceat(np.abs(fv), rowptr[:-1])
    return Problem("one_way", (0, 2048, 4096, 6144), rowptr, col, val, _pattern_matrix(rowptr, col, fv))


def _wrap_skip():
    """5300 rows in blocks of 2400, 500, 2400, each tridiagonal on its own; row i < 60 is coupled with row 5299 - i.  Symmetric.  The float
    matrix has 4 on the diagonal and -1 beside it (at most three off-diagonal entries in a row)."""
    import scipy.sparse as sp

    starts = (0, 2400, 2900, 5300)
    m = starts[-1]
    i = np.arange(m - 1)
    inside = ~np.isin(i + 1, starts)  # i and i + 1 in the same block
    lo, hi = i[inside], i[inside] + 1
    w = np.arange(60)
    r = np.concatenate([lo, hi, w, m - 1 - w, np.arange(m)])
    c = np.concatenate([hi, lo, m - 1 - w, w, np.arange(m)])
    v = np.concatenate([-np.ones(2 * lo.size + 2 * w.size), 4.0 * np.ones(m)])
    A = sp.csr_matrix((v, (r, c)), shape=(m, m))
    A.sort_indices()
    rowptr, col = A.indptr.astype(np.int64), A.indices.astype(np.int64)
    return Problem("wrap_skip", starts, rowptr, col, R.int_values(col.size, seed=12), A)


def _all_to_all():
    """uniform_random(900, 5, seed=2) on three balanced ranks: columns anywhere, more ghost rows than local rows, no interior"""
    from rails_amd import partition
    from rails_amd import problems as P

    rowptr, col, _ = P.uniform_random(900, 5, seed=2)
    return Problem("all_to_all", partition.row_ranges(900, 3), rowptr, col, R.int_values(col.size, seed=13))


def _scattered():
    """banded_random(3 * 4096, 9, 64, seed=4) on three balanced ranks; rows 4096 + 700 and 4096 + 3500 of the middle rank reference
    columns 5 and 3 * 4096 - 7 as well: boundary rows in the middle of its block"""
    from rails_amd import partition
    from rails_amd import problems as P

    m = 3 * 4096
    rowptr, col, _ = P.banded_random(m, 9, 64, seed=4)
    rows = [np.asarray(col[rowptr[i]:rowptr[i + 1]], dtype=np.int64) for i in range(m)]
    for i in (4096 + 700, 4096 + 3500):
        rows[i] = np.sort(np.concatenate([rows[i], [5, m - 7]]))
    rowptr, col = _from_rows(rows)
    return Problem("scattered", partition.row_ranges(m, 3), rowptr, col, R.int_values(col.size, seed=14))


def _unequal():
    """tridiagonal, 700 rows in blocks of 333, 1 and 366: the middle rank is one row with two ghost rows and two rows to send"""
    m = 700
    rows = [np.arange(max(0, i - 1), min(m, i + 2)) for i in range(m)]
    rowptr, col = _from_rows(rows)
    return Problem("unequal", (0, 333, 334, 700), rowptr, col, R.int_values(col.size, seed=15))


_make = {"one_way": _one_way, "wrap_skip": _wrap_skip, "all_to_all": _all_to_all, "scattered": _scattered, "unequal": _unequal}
_problems, _plans = {}, {}


def problem(name):
    if name not in _problems:
        _problems[name] = _make[name]()
    return _problems[name]


def requests(starts, colg, q):
    """what rank q asks of every rank: its ghost rows by owner (HaloPlan's own first step)"""
    colg = np.asarray(colg, dtype=np.int64)
    ghosts = np.unique(colg[(colg < starts[q]) | (colg >= starts[q + 1])])
    owner = np.searchsorted(starts, ghosts, side="right") - 1
    return [ghosts[owner == d] for d in range(len(starts) - 1)]


def plans_of(starts, blocks):
    """the HaloPlan of every rank, from every rank's row block (rowptr, col_global, val), without threads"""
    from rails_amd import partition

    n = len(blocks)
    gathered = [requests(starts, blocks[q][1], q) for q in range(n)]
    return [partition.HaloPlan(starts, r, blocks[r][1], lambda mine: gathered) for r in range(n)]


def plans(p):
    if p.name not in _plans:
        _plans[p.name] = plans_of(p.starts, [p.block(r) for r in range(p.nranks)])
    return _plans[p.name]


def interior(rowptr, col_local, m_local, n_ghost):
    """[int_lo, int_hi) as rails_csr_set_halo finds it: walking the rows upwards, a boundary row of the lower half moves int_lo behind
    it, the first boundary row of the upper half ends the range"""
    lo, hi = 0, m_local
    if n_ghost > 0:
        boundary = np.zeros(m_local, dtype=bool)
        cnt = np.diff(rowptr)
        np.logical_or.at(boundary, np.repeat(np.arange(m_local), cnt), np.asarray(col_local) >= m_local)
        mid = m_local // 2
        low = np.flatnonzero(boundary[:mid])
        high = np.flatnonzero(boundary[mid:])
        if low.size:
            lo = int(low.max()) + 1
        if high.size:
            hi = mid + int(high.min())
    return lo, hi


def overlaps(m_local, n_ghost, lo, hi, variant=1):
    """rails_halo_order's condition with RAILS_SPMM_HALO_OVERLAP on (op_choice.h), for a square operator"""
    return n_ghost > 0 and variant in (0, 1, 3) and hi - lo >= m_local // 2 and hi - lo >= 1024


def rank_facts(p):
    """per rank: dict(m_local, n_ghost, n_send, recv_counts, send_counts, interior, overlaps)"""
    out = []
    for r, plan in enumerate(plans(p)):
        rowptr = p.block(r)[0]
        lo, hi = interior(rowptr, plan.col_local, plan.m_local, plan.n_ghost)
        out.append(dict(m_local=plan.m_local, n_ghost=plan.n_ghost, n_send=plan.n_send, recv_counts=[int(x) for x in plan.recv_counts],
                        send_counts=[int(x) for x in plan.send_counts], interior=(lo, hi), overlaps=overlaps(plan.m_local, plan.n_ghost, lo, hi)))
    return out
