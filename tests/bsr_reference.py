"""A numpy restatement of how a block-CSR product is launched (rails_amd/csrc/bsr_choice.h) and exact integer problems for the kernels on the
shared block-row body (rails_amd/csrc/bsr_row_gather.inc: k_spmm_bsr, k_cheb_step_bsr, k_amg_residual_bsr), written from the rules and not
by calling the library.  Not a test module: tests/test_bsr_reference_host.py checks it on the CPU, tests/test_gpu_bsr_rounds.py and
tests/test_gpu_block_amg.py hold the device to it.

The launch rule gives a lane group rpg = 2 or 4 block rows, one after the other, only from groups * rpg * (2 num_cu - 1) + 1 block rows on
(thousands at 256 compute units); shape_for names the smallest such shape of an instantiation and the longest block row the rule allows
there.  The problems are integers: block entries in [-3, 3], panel entries in [-4, 4], so every partial sum of a product is an integer far
below 2^53, the float64 product is exact in any order of summation, and the reference -- computed in int64 on the host -- is compared
with np.array_equal, without a tolerance."""
import numpy as np

LDS_DOUBLES = 4096
BS = tuple(range(2, 9))
LPRS = (8, 16, 32)
INSTANTIATIONS = tuple((b, lpr) for b in BS for lpr in LPRS)  # RAILS_BSR_TABLE
PAIRS = tuple((b, lpr, rpg) for b, lpr in INSTANTIATIONS for rpg in (2, 4))
# widths that pick an instantiation's lanes per block row: the full chunk, an odd width (its last lane loads the last pair and keeps .y), one
# column (8-byte loads), and 130: three chunks inside every round
WIDTHS = {8: (16, 15, 1), 16: (32, 17), 32: (64, 33, 130)}
ENTRY, PANEL = 3, 4  # |block entries| <= 3, |panel entries| <= 4


# ---------------------------------------------------------------------------------------------------------------- the launch decision
def threads(b):
    """rails_bsr_threads"""
    return 256 if b <= 4 else 128 if b <= 6 else 64


def lds_blocks(b):
    """rails_bsr_lds_blocks: the blocks a workgroup's staging buffer holds"""
    return LDS_DOUBLES // (b * b)


def lanes(nc):
    return 8 if nc <= 16 else 16 if nc <= 32 else 32


def bsr_choice(b, nc, mb, max_brow, num_cu=256):
    """bsr_choice.h: (lpr, threads, rpg, rows, bpx, grid, all_staged) or None"""
    if b < 2 or b > 8 or nc < 1 or mb < 1 or max_brow < 0:
        return None
    lpr = lanes(nc)
    groups, cap = threads(b) // lpr, lds_blocks(b)
    rpg = 1
    while rpg < 4 and groups * 2 * rpg * max(max_brow, 1) <= cap and (mb + groups * 2 * rpg - 1) // (groups * 2 * rpg) >= 2 * max(num_cu, 1):
        rpg *= 2
    rows = groups * rpg
    bpx = ((mb + rows - 1) // rows + 7) // 8
    if bpx * 8 > 0x7fffffff:
        return None
    return lpr, threads(b), rpg, rows, bpx, bpx * 8, rows * max_brow <= cap


def shape_for(b, lpr, rpg, num_cu=256):
    """(mb_min, kmax): the fewest block rows at which the rule gives k_spmm_bsr<b, lpr> exactly `rpg` block rows per lane group (with block
    rows short enough), and the longest block row it still allows there"""
    groups = threads(b) // lpr
    return groups * rpg * (2 * max(num_cu, 1) - 1) + 1, lds_blocks(b) // (groups * rpg)


def block_rows(b, lpr, rpg, num_cu=256):
    """the block-row counts a pair is tested at, by what the last workgroup holds: one block row (it breaks out of every round but the
    first); a full round and one block row of the second; a full round and two block rows -- with two lane groups (b = 7, 8 at 32 lanes)
    that is two full rounds, and at rpg = 2 a full workgroup"""
    mb_min = shape_for(b, lpr, rpg, num_cu)[0]
    groups = threads(b) // lpr
    return mb_min, mb_min + groups, mb_min + groups + 1


def predicted_stats(b, nc, mb, max_brow, num_cu):
    """what rails_csr_bsr_stats reports of a launch, from the rule"""
    lpr, nt, rpg, rows, bpx, grid, staged = bsr_choice(b, nc, mb, max_brow, num_cu)
    return {"B": b, "LPR": lpr, "threads": nt, "rpg": rpg, "grid": grid, "all_staged": staged}


# ---------------------------------------------------------------------------------------------------------------- block-row counts
def counts_full(mb, kmax):
    """(a) every block row holds kmax blocks: a full workgroup's run of rows * kmax blocks fills the staging buffer as far as it can --
    exactly where 4096 / b^2 is a power of two (b = 2, 4, 8)"""
    return np.full(mb, kmax, dtype=np.int64)


def forced_empty(mb, groups, rpg):
    """(block rows forced empty, the workgroup left without a block) of pattern (b): the first and the last block row of every round of the
    first, a middle and the last workgroup, and all block rows of one more workgroup"""
    rows = groups * rpg
    nwg = -(-mb // rows)
    empty = []
    for w in sorted({0, nwg // 2, nwg - 1}):
        for rr in range(rpg):
            lo, hi = w * rows + rr * groups, min(w * rows + (rr + 1) * groups, mb)
            if lo < hi:
                empty += [lo, hi - 1]
    bare = nwg // 3 if nwg // 3 not in (0, nwg // 2, nwg - 1) else None
    if bare is not None:
        empty += list(range(bare * rows, min((bare + 1) * rows, mb)))
    return np.unique(np.asarray(empty, dtype=np.int64)), bare


def counts_uniform(mb, kmax, groups, rpg, seed):
    """(b) counts uniform in 0 .. kmax with forced_empty's block rows emptied; one other block row holds kmax blocks whatever was drawn, so
    that the longest block row, which the rule looks at, is kmax"""
    g = np.random.default_rng(seed)
    counts = g.integers(0, kmax + 1, mb).astype(np.int64)
    empty = forced_empty(mb, groups, rpg)[0]
    counts[g.choice(np.setdiff1d(np.arange(mb), empty))] = kmax
    counts[empty] = 0
    return counts


def counts_one_longer(mb, kmax, seed):
    """(c) pattern (a) with one block row of kmax + 1 blocks: the rule steps back to rpg / 2"""
    counts = counts_full(mb, kmax)
    counts[int(np.random.default_rng(seed).integers(0, mb))] = kmax + 1
    return counts


# ---------------------------------------------------------------------------------------------------------------- integer problems
def pattern(counts, seed):
    """(indptr, indices): block row i holds counts[i] blocks at distinct ascending random block columns"""
    counts = np.asarray(counts, dtype=np.int64)
    mb, k = counts.size, int(counts.max()) if counts.size else 0
    assert k < mb, "a block row of %d blocks in %d block columns" % (k, mb)
    g = np.random.default_rng(seed)
    cols = np.sort(g.integers(0, mb - k + 1, (mb, max(k, 1))), axis=1) + np.arange(max(k, 1))[None, :]  # strictly ascending, below mb
    # every row keeps a random subset of its k columns, in order
    keep = np.argsort(g.random((mb, max(k, 1))), axis=1) < counts[:, None]
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return indptr, cols[keep].astype(np.int32)


def integer_blocks(nnzb, b, seed, nonzero=False):
    """block entries: integers in [-3, 3] as float64 (nonzero: none of them 0)"""
    g = np.random.default_rng(seed)
    if nonzero:
        return (g.integers(1, ENTRY + 1, (nnzb, b, b)) * (2 * g.integers(0, 2, (nnzb, b, b)) - 1)).astype(np.float64)
    return g.integers(-ENTRY, ENTRY + 1, (nnzb, b, b)).astype(np.float64)


def integer_problem(counts, b, seed, nonzero=False):
    """(indptr, indices, data) of an integer block matrix with the given block-row counts"""
    indptr, indices = pattern(counts, seed)
    return indptr, indices, integer_blocks(indices.size, b, seed + 1, nonzero)


def integer_panel(m, nc, seed):
    """panel entries: integers in [-4, 4] as float64"""
    return np.random.default_rng(seed).integers(-PANEL, PANEL + 1, (m, nc)).astype(np.float64)


def with_shared_column(indptr, indices, data, rows, col):
    """the same matrix with the last block of each of `rows` moved to block column `col` (the largest: rows stay ascending), so that one
    block column is referenced by len(rows) block rows and the transposed matrix has a block row that long"""
    assert col == indptr.size - 2 and np.all(np.diff(indptr)[rows] > 0)
    indices = indices.copy()
    indices[indptr[np.asarray(rows) + 1] - 1] = col
    return indptr, indices, data


def transposed(indptr, indices, data):
    """the block arrays of A^T, block columns ascending (a stable counting sort by block column, every block transposed)"""
    mb = indptr.size - 1
    brow = np.repeat(np.arange(mb), np.diff(indptr))
    order = np.argsort(indices, kind="stable")
    tptr = np.concatenate([[0], np.cumsum(np.bincount(indices, minlength=mb))]).astype(np.int64)
    return tptr, brow[order].astype(np.int32), np.ascontiguousarray(data[order].transpose(0, 2, 1))


def product_int64(indptr, indices, data, X):
    """(A X in int64, by scipy's block product on int64 arrays; a bound no partial sum of it exceeds in any order of summation: the entries
    of the longest scalar row times the largest |a| |x|)"""
    import scipy.sparse as sp

    nnzb, b, _ = data.shape
    mb = indptr.size - 1
    Ai = np.rint(data).astype(np.int64)
    Xi = np.rint(X).astype(np.int64)
    assert np.array_equal(Ai, data) and np.array_equal(Xi, X), "not an integer problem"
    Y = sp.bsr_matrix((Ai, indices, indptr), shape=(mb * b, mb * b)) @ Xi
    assert Y.dtype == np.int64
    bound = int(np.diff(indptr).max() if mb else 0) * b * int(np.abs(Ai).max() if nnzb else 0) * int(np.abs(Xi).max() if Xi.size else 0)
    return Y, bound


def reference(indptr, indices, data, X):
    """the exact product as float64"""
    Y, bound = product_int64(indptr, indices, data, X)
    assert bound < 2 ** 53
    return Y.astype(np.float64)


def uniform_like(indptr, indices, data, seed):
    """the same pattern with entries U(-1, 1), for the bit-for-bit comparison with the row-gather kernel"""
    return indptr, indices, np.random.default_rng(seed).uniform(-1.0, 1.0, data.shape)
