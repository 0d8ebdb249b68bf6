"""tests/bsr_reference.py on the CPU: the restated launch rule against the stand-alone program of the rule (rails_amd/lib/bsr_host --table),
shape_for over every instantiation and three compute-unit counts, the integer reference against scipy.sparse.bsr_matrix, and the count
patterns against what tests/test_gpu_bsr_rounds.py relies on."""
import json
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import block_amg_reference as B
import bsr_reference as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rails_amd", "lib", "bsr_host")
NUM_CUS = (256, 304, 64)


def table():
    if not os.path.exists(EXE):
        import rails_amd.build

        rails_amd.build.build()
    p = subprocess.run([EXE, "--table"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:]
    return [json.loads(line) for line in p.stdout.splitlines()]


def test_the_restatement_is_the_one_copy_and_agrees_with_the_table_of_the_rule():
    assert B.bsr_choice is K.bsr_choice
    rows = table()
    assert sorted(tuple(r["inst"]) for r in rows) == sorted(K.INSTANTIATIONS)
    for r in rows:
        b, lpr = r["inst"]
        # the program walks its shapes with the longest block row ascending from 0 and the compute units from 1: the first shape that
        # reaches an instantiation has both at their smallest
        got = K.bsr_choice(r["b"], r["nc"], r["mb"], 0, 1)
        assert got[:4] == (lpr, r["threads"], 1, r["rows"]) and r["threads"] == K.threads(b), (r, got)
        assert K.lanes(r["nc"]) == lpr and K.lds_blocks(b) == 4096 // (b * b)
    for lpr, widths in K.WIDTHS.items():
        assert all(K.lanes(nc) == lpr for nc in widths)
    assert K.bsr_choice(1, 4, 10, 1) is None and K.bsr_choice(9, 4, 10, 1) is None and K.bsr_choice(4, 0, 10, 1) is None and K.bsr_choice(4, 4, 0, 1) is None


def test_the_table_of_the_issue_at_256_compute_units():
    want = {2: ((32705, 16353, 8177), (65409, 32705, 16353)), 5: ((16353, 8177, 4089), (32705, 16353, 8177)), 7: ((8177, 4089, 2045), (16353, 8177, 4089))}
    for b in K.BS:
        two, four = want[2 if b <= 4 else 5 if b <= 6 else 7]
        assert tuple(K.shape_for(b, lpr, 2)[0] for lpr in K.LPRS) == two and tuple(K.shape_for(b, lpr, 4)[0] for lpr in K.LPRS) == four


@pytest.mark.parametrize("num_cu", NUM_CUS)
def test_shape_for_is_the_boundary_of_the_rule(num_cu):
    assert len(K.PAIRS) == 42
    for b, lpr, rpg in K.PAIRS:
        mb, kmax = K.shape_for(b, lpr, rpg, num_cu)
        groups = K.threads(b) // lpr
        assert kmax >= 1, (b, lpr, rpg)
        for nc in K.WIDTHS[lpr]:
            assert K.block_rows(b, lpr, rpg, num_cu) == (mb, mb + groups, mb + groups + 1)
            for mbs in K.block_rows(b, lpr, rpg, num_cu):
                got = K.bsr_choice(b, nc, mbs, kmax, num_cu)
                assert got[0] == lpr and got[2] == rpg and got[3] == groups * rpg and got[6], (b, lpr, rpg, nc, mbs, got)
                # a full workgroup's run is as long as the buffer allows; exactly the buffer where 4096 / b^2 is a power of two
                assert got[3] * kmax <= K.lds_blocks(b) < got[3] * (kmax + 1)
                if b in (2, 4, 8):
                    assert got[3] * kmax == K.lds_blocks(b)
                # the block rows of the last workgroup: 1, groups + 1, groups + 2 (a full workgroup with two lane groups and two rounds)
                assert (mbs - 1) % got[3] + 1 == mbs - mb + 1
            # one block row fewer, or one block longer: half as many rounds
            assert K.bsr_choice(b, nc, mb - 1, kmax, num_cu)[2] == rpg // 2
            assert K.bsr_choice(b, nc, mb, kmax + 1, num_cu)[2] == rpg // 2
            if rpg == 2:  # and not yet four, however short the block rows
                assert K.bsr_choice(b, nc, mb + groups + 1, 1, num_cu)[2] == 2
        st = K.predicted_stats(b, K.WIDTHS[lpr][0], mb, kmax, num_cu)
        workgroups = -(-mb // (groups * rpg))
        assert workgroups == 2 * num_cu  # two per compute unit, the last with one block row
        assert st == {"B": b, "LPR": lpr, "threads": K.threads(b), "rpg": rpg, "grid": 8 * -(-workgroups // 8), "all_staged": True}


def scipy_of(triple):
    indptr, indices, data = triple
    mb, b = indptr.size - 1, data.shape[1]
    return sp.bsr_matrix((data, indices, indptr), shape=(mb * b, mb * b))


@pytest.mark.parametrize("b,lpr,rpg", [(2, 32, 2), (3, 8, 4), (6, 16, 4), (8, 8, 2)])
def test_patterns_and_the_integer_reference(b, lpr, rpg):
    num_cu = 4  # (the shapes of a small device: the same code as at 256)
    mb, kmax = K.shape_for(b, lpr, rpg, num_cu)
    mb += K.threads(b) // lpr + 1
    groups = K.threads(b) // lpr
    rows = groups * rpg
    nwg = -(-mb // rows)
    nc = K.WIDTHS[lpr][1]
    X = K.integer_panel(mb * b, nc, seed=5)
    assert X.min() == -4 and X.max() == 4 and np.array_equal(X, np.rint(X))
    for name, counts in (("a", K.counts_full(mb, kmax)), ("b", K.counts_uniform(mb, kmax, groups, rpg, seed=3)), ("c", K.counts_one_longer(mb, kmax, seed=4))):
        triple = K.integer_problem(counts, b, seed=11)
        indptr, indices, data = triple
        assert indptr.dtype == np.int64 and indices.dtype == np.int32 and data.dtype == np.float64 and data.shape == (indices.size, b, b)
        assert np.array_equal(np.diff(indptr), counts) and data.min() == -3 and data.max() == 3 and np.array_equal(data, np.rint(data))
        for i in (0, 1, mb // 2, mb - 1):  # distinct, ascending, in range
            c = indices[indptr[i]:indptr[i + 1]]
            assert np.all(np.diff(c) > 0) and (c.size == 0 or (c[0] >= 0 and c[-1] < mb))
        brow = np.repeat(np.arange(mb), counts)
        assert np.all((np.diff(indices.astype(np.int64)) > 0) | (np.diff(brow) > 0)) and indices.min() >= 0 and indices.max() < mb
        if name == "c":
            assert np.sort(counts)[-2:].tolist() == [kmax, kmax + 1] and K.bsr_choice(b, nc, mb, int(counts.max()), num_cu)[2] == rpg // 2
        else:
            assert counts.max() == kmax and K.bsr_choice(b, nc, mb, int(counts.max()), num_cu)[2] == rpg
        if name == "a":
            assert np.all(counts == kmax)
        if name == "b":
            empty, bare = K.forced_empty(mb, groups, rpg)
            assert bare is not None and np.all(counts[bare * rows:(bare + 1) * rows] == 0) and np.all(counts[empty] == 0)
            for w in (0, nwg // 2, nwg - 1):
                for rr in range(rpg):
                    lo, hi = w * rows + rr * groups, min(w * rows + (rr + 1) * groups, mb)
                    assert lo >= hi or (counts[lo] == 0 and counts[hi - 1] == 0)
            assert counts.min() == 0 and counts.max() == kmax and np.unique(counts).size >= min(kmax + 1, 8)
        Y, bound = K.product_int64(indptr, indices, data, X)
        assert Y.dtype == np.int64 and bound < 2 ** 53 and np.abs(Y).max() <= bound
        # against numpy alone: the dense int64 matrix, block by block, times the int64 panel
        dense = np.zeros((mb * b, mb * b), dtype=np.int64)
        for q, (i, c) in enumerate(zip(brow, indices)):
            dense[i * b:(i + 1) * b, c * b:(c + 1) * b] = data[q]
        assert np.array_equal(Y, dense @ X.astype(np.int64))
        assert np.array_equal(K.reference(indptr, indices, data, X), scipy_of(triple) @ X)
        # every block entry non-zero on request, the pattern the same
        nz = K.integer_problem(counts, b, seed=11, nonzero=True)
        assert np.array_equal(nz[1], indices) and np.all(nz[2] != 0) and np.abs(nz[2]).max() == 3
    with pytest.raises(AssertionError, match="not an integer problem"):
        K.product_int64(indptr, indices, data + 0.5, X)


def test_transposed_and_the_shared_block_column():
    b, lpr, num_cu = 3, 16, 8
    mb, kmax = K.shape_for(b, lpr, 4, num_cu)
    triple = K.integer_problem(K.counts_full(mb, kmax), b, seed=2)
    rows = np.arange(5, 5 + 8 * kmax)
    triple = K.with_shared_column(*triple, rows=rows, col=mb - 1)
    indptr, indices, data = triple
    brow = np.repeat(np.arange(mb), np.diff(indptr))
    assert np.all((np.diff(indices.astype(np.int64)) > 0) | (np.diff(brow) > 0)) and np.all(np.diff(indptr) == kmax)
    T = K.transposed(*triple)
    assert np.array_equal(scipy_of(T).toarray(), scipy_of(triple).toarray().T)
    tcounts = np.diff(T[0])
    assert tcounts[mb - 1] >= 8 * kmax and K.bsr_choice(b, 17, mb, int(np.diff(indptr).max()), num_cu)[2] == 4
    assert K.bsr_choice(b, 17, mb, int(tcounts.max()), num_cu)[2] < 4
    trow = np.repeat(np.arange(mb), tcounts)
    assert np.all((np.diff(T[1].astype(np.int64)) > 0) | (np.diff(trow) > 0))
    X = K.integer_panel(mb * b, 5, seed=1)
    assert np.array_equal(K.reference(*T, X), scipy_of(triple).T @ X)
    back = K.transposed(*T)
    assert all(np.array_equal(u, v) for u, v in zip(back, triple))
    U = K.uniform_like(*triple, seed=3)
    assert U[0] is indptr and U[1] is indices and U[2].shape == data.shape and np.abs(U[2]).max() < 1.0
