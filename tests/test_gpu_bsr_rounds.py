"""k_spmm_bsr (rails_amd/csrc/spmm_bsr.hip on bsr_row_gather.inc) at the launches that give a lane group 2 and 4 block rows, one after the
other: every instantiation of bsr_choice.h at the smallest shapes of tests/bsr_reference.py::shape_for for the context's compute units,
where tests/test_gpu_bsr.py stays at one round.  What runs only there: rounds 2 to 4 of the body, the break of the last workgroup out of
its dead rounds, its partly live round, a staged run shared by several rounds, and a run that fills the LDS buffer exactly.

The reference is the int64 product of an integer problem (bsr_reference.reference: numpy alone), compared with np.array_equal; every case
first holds rails_csr_bsr_stats to the restated rule, which proves that the launch had the rounds the case is about.  The row-gather kernel
is a second witness, bit for bit on U(-1, 1) data, not the reference.  Non-finite rows of X show that what a lane loads beyond its own
block row -- the first block of its row or of the workgroup's run again, the neighbouring column of its pair -- stays out of the result."""
import numpy as np
import pytest

import bsr_reference as K
from test_gpu_bsr import Pair, product

pytestmark = pytest.mark.gpu

WINDOWS = ((0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 3, 2), (1, 1, 0, 0), (2, 3, 3, 2), (3, 2, 3, 2), (0, 0, 3, 2), (1, 1, 3, 2))  # xoff, yoff, xtail, ytail


@pytest.fixture(scope="module")
def ctx():
    import rails_amd

    c = rails_amd.Context(device=0, seed=77)
    yield c
    c.close()


def compute_units(ctx):
    n = ctx.lib.rails_ctx_num_cu(ctx.h)
    assert n > 0
    return n


def operator(ctx, triple):
    import rails_amd

    return rails_amd.HipOperatorWrapper.from_bsr(ctx, *triple)


def launched_as_the_rule_says(ctx, op, nc, rpg):
    """rails_csr_bsr_stats of the last launch against the restatement at the context's compute units, and rpg the wanted one"""
    st = op.bsr_stats()
    mb = (op.M() // st["b"])
    want = K.predicted_stats(st["b"], nc, mb, st["max_block_row"], compute_units(ctx))
    assert {k: st[k] for k in want} == want, (st, want)
    assert st["rpg"] == rpg, (st, rpg)
    return st


def exact(got, want, what):
    assert np.array_equal(got, want), "%s: %d entries differ from the int64 product" % (what, int((got != want).sum()))
    assert not np.any(np.signbit(got) & (got == 0.0)), "%s: a negative zero" % (what,)


@pytest.mark.parametrize("b,lpr,rpg", K.PAIRS)
def test_every_round_against_the_int64_product(ctx, b, lpr, rpg):
    """patterns (a) and (b) at the three block-row counts of bsr_reference.block_rows (the middle one with (a) alone), every width of the
    instantiation; pattern (c), one block row a block longer, steps back to rpg / 2 on the same kind of data; on the last shape the
    row-gather kernel agrees bit for bit on U(-1, 1) data"""
    ncu = compute_units(ctx)
    mb_min, kmax = K.shape_for(b, lpr, rpg, ncu)
    groups = K.threads(b) // lpr
    widths = K.WIDTHS[lpr]
    sizes = K.block_rows(b, lpr, rpg, ncu)
    reported = set()
    for mb in sizes:
        Xw = K.integer_panel(mb * b, max(widths), seed=mb)
        for name in ("a", "b") if mb != sizes[1] else ("a",):
            counts = K.counts_full(mb, kmax) if name == "a" else K.counts_uniform(mb, kmax, groups, rpg, seed=mb + 1)
            triple = K.integer_problem(counts, b, seed=100 * b + lpr + rpg)
            op = operator(ctx, triple)
            want = K.reference(*triple, Xw)
            for nc in widths:
                got = product(ctx, op, np.ascontiguousarray(Xw[:, :nc]))
                assert op.last_kernel() == "k_spmm_bsr"
                st = launched_as_the_rule_says(ctx, op, nc, rpg)
                assert st["all_staged"] and st["max_block_row"] == kmax
                reported.add((st["rpg"], st["all_staged"]))
                exact(got, want[:, :nc], "k_spmm_bsr<%d, %d>, rpg %d, %d block rows, pattern (%s), %d columns" % (b, lpr, rpg, mb, name, nc))
            if name == "b" and mb == sizes[2]:
                pair = Pair(ctx, K.uniform_like(*triple, seed=mb))
                for nc in widths:
                    pair.check(nc, seed=nc)
                    launched_as_the_rule_says(ctx, pair.bsr, nc, rpg)
    # (c): the boundary of the rule on the device
    triple = K.integer_problem(K.counts_one_longer(mb_min, kmax, seed=b), b, seed=7 * b + lpr)
    op = operator(ctx, triple)
    Xh = K.integer_panel(mb_min * b, widths[1], seed=3)
    got = product(ctx, op, Xh)
    st = launched_as_the_rule_says(ctx, op, widths[1], rpg // 2)
    assert st["max_block_row"] == kmax + 1
    exact(got, K.reference(*triple, Xh), "k_spmm_bsr<%d, %d>, one block row of %d blocks" % (b, lpr, kmax + 1))
    print("k_spmm_bsr<%d, %d> at %d compute units, %d..%d block rows of at most %d blocks: reported (rpg, all_staged) %s; one block more: rpg %d, all_staged %s" % (
        b, lpr, ncu, sizes[0], sizes[2], kmax, sorted(reported), st["rpg"], st["all_staged"]))
    assert reported == {(rpg, True)}


@pytest.mark.parametrize("b,lpr", [(3, 8), (4, 16), (7, 32)])
def test_windows_in_poisoned_panels_at_four_rounds(ctx, b, lpr):
    """X and Y on odd and even columns of NaN-filled panels, with and without tails: both store forms of the epilogue (16-byte stores on
    an even column of Y, two 8-byte stores on an odd one) in rounds beyond the first, nothing written outside the window"""
    ncu = compute_units(ctx)
    rpg = 4
    groups = K.threads(b) // lpr
    mb, kmax = K.block_rows(b, lpr, rpg, ncu)[2], K.shape_for(b, lpr, rpg, ncu)[1]
    triple = K.integer_problem(K.counts_uniform(mb, kmax, groups, rpg, seed=b), b, seed=lpr)
    op = operator(ctx, triple)
    widths = K.WIDTHS[lpr][:2]
    Xw = K.integer_panel(mb * b, max(widths), seed=2)
    want = K.reference(*triple, Xw)
    for nc in widths:
        Xh = np.ascontiguousarray(Xw[:, :nc])
        for xoff, yoff, xtail, ytail in WINDOWS:
            got = product(ctx, op, Xh, xoff=xoff, yoff=yoff, xtail=xtail, ytail=ytail)  # (asserts that the rest of Y's panel is still NaN)
            launched_as_the_rule_says(ctx, op, nc, rpg)
            exact(got, want[:, :nc], "b %d, %d columns, X at %d (+%d), Y at %d (+%d)" % (b, nc, xoff, xtail, yoff, ytail))


@pytest.mark.parametrize("b,lpr", [(2, 8), (5, 16), (8, 32)])
def test_transposed_product_of_a_matrix_with_a_long_block_column(ctx, b, lpr):
    """pattern (a) with one block column referenced by 8 kmax block rows: forward four rounds; the transposed copy has a block row that
    long and takes fewer.  The same from the transposed data, whose transposed copy is the matrix itself and takes four rounds."""
    ncu = compute_units(ctx)
    mb, kmax = K.shape_for(b, lpr, 4, ncu)
    A = K.integer_problem(K.counts_full(mb, kmax), b, seed=b)
    A = K.with_shared_column(*A, rows=np.arange(3, 3 + 16 * kmax, 2), col=mb - 1)
    T = K.transposed(*A)
    long_row = int(np.diff(T[0]).max())
    assert long_row >= 8 * kmax and int(np.diff(A[0]).max()) == kmax
    fewer = K.predicted_stats(b, K.WIDTHS[lpr][0], mb, long_row, ncu)["rpg"]
    assert fewer < 4
    opA, opT = operator(ctx, A), operator(ctx, T)
    for nc in K.WIDTHS[lpr][:2]:
        Xh = K.integer_panel(mb * b, nc, seed=nc)
        AX, ATX = K.reference(*A, Xh), K.reference(*T, Xh)
        for op, fwd, fwd_rpg, rev, rev_rpg in ((opA, AX, 4, ATX, fewer), (opT, ATX, fewer, AX, 4)):
            got = product(ctx, op, Xh, xoff=1)
            assert op.last_kernel() == "k_spmm_bsr"
            launched_as_the_rule_says(ctx, op, nc, fwd_rpg)
            exact(got, fwd, "b %d, %d columns, forward at rpg %d" % (b, nc, fwd_rpg))
            got = product(ctx, op.transpose(), Xh, yoff=1)
            assert op.last_kernel() == "k_spmm_bsr (transposed copy)"
            # (the stats name the handle's own matrix and the last launch, here of the transposed copy)
            st = op.bsr_stats()
            want = K.predicted_stats(b, nc, mb, long_row if rev_rpg != 4 else kmax, ncu)
            assert {k: st[k] for k in want} == want and st["rpg"] == rev_rpg, (st, want)
            exact(got, rev, "b %d, %d columns, transposed copy at rpg %d" % (b, nc, rev_rpg))


@pytest.mark.parametrize("b,lpr,rpg", [(5, 16, 1), (6, 8, 2), (2, 32, 4)])
def test_non_finite_rows_of_x_reach_only_the_block_rows_that_reference_them(ctx, b, lpr, rpg):
    """Pattern (b), every stored entry non-zero.  X holds NaN in column j of the b rows of a few block columns, among them those of the
    first block of some workgroups' runs and of some block rows -- the blocks a lane past the end of its own block row loads again.
    Y[:, j] is NaN exactly in the block rows that store a block in one of these columns, and everything else is the int64 product with
    those entries of X at 0: neither the repeated loads nor the other column of a lane's pair reach an accumulator.  j even, j odd, and
    j = nc - 2 with nc odd, where the lane of the last column loads the pair (nc - 2, nc - 1) and keeps its second half."""
    ncu = compute_units(ctx)
    groups = K.threads(b) // lpr
    if rpg == 1:
        mb, kmax = 40 * groups + 3, 6
    else:
        mb, kmax = K.block_rows(b, lpr, rpg, ncu)[2], K.shape_for(b, lpr, rpg, ncu)[1]
    counts = K.counts_uniform(mb, kmax, groups, rpg, seed=b + rpg)
    indptr, indices, data = triple = K.integer_problem(counts, b, seed=rpg, nonzero=True)
    op = operator(ctx, triple)
    rows = groups * rpg
    nwg = -(-mb // rows)
    g = np.random.default_rng(rpg)
    first_of_runs = [int(indptr[w * rows]) for w in (0, 1, nwg // 2, nwg - 2) if indptr[w * rows] < indices.size]
    first_of_rows = indptr[g.choice(np.flatnonzero(counts > 0), 5, replace=False)].tolist()
    chosen = np.unique(np.concatenate([indices[first_of_runs + first_of_rows], g.integers(0, mb, 2)]))
    hit = np.zeros(mb, dtype=bool)
    hit[np.repeat(np.arange(mb), counts)[np.isin(indices, chosen)]] = True
    assert 0 < hit.sum() < mb // 2
    nc = K.WIDTHS[lpr][1]
    assert nc % 2 == 1
    clean = K.integer_panel(mb * b, nc, seed=9)
    xrows = (chosen[:, None] * b + np.arange(b)[None, :]).ravel()
    for j in (4, 7, nc - 2):
        Xh, zeroed = clean.copy(), clean.copy()
        Xh[xrows, j] = np.nan
        zeroed[xrows, j] = 0.0
        got = product(ctx, op, Xh, xoff=1)
        launched_as_the_rule_says(ctx, op, nc, rpg)
        want_nan = np.zeros((mb * b, nc), dtype=bool)
        want_nan[np.repeat(hit, b), j] = True
        assert np.array_equal(np.isnan(got), want_nan), "b %d, rpg %d, NaN in column %d of X: %d entries of Y are NaN, %d should be" % (
            b, rpg, j, int(np.isnan(got).sum()), int(want_nan.sum()))
        want = K.reference(*triple, zeroed)
        assert np.array_equal(got[~want_nan], want[~want_nan])
