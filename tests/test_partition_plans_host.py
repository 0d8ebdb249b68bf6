"""The ghost-row plans of tests/partition_plans.py, on the CPU: the counts tests/test_gpu_partition_plans.py depends on (a rank that only
sends, one that only receives, an empty one, exchanges with every other rank, boundary rows in the middle of a block, a rank of one row),
the conditions of the exact reference (spmm_reference.spmm_exact_int) and those of the solves."""
import numpy as np
import pytest

import partition_plans as PP
import spmm_reference as R

# per rank: (m_local, n_ghost, n_send), recv_counts by owner, send_counts by destination, interior rows [int_lo, int_hi), overlapped order
EXPECTED = {
    "one_way": [((2048, 0, 36), [0, 0, 0], [0, 36, 0], (0, 2048), False),       # only sends
                ((2048, 36, 36), [36, 0, 0], [0, 0, 36], (39, 2048), True),
                ((2048, 36, 0), [0, 36, 0], [0, 0, 0], (40, 2048), True)],      # only receives
    "wrap_skip": [((2400, 60, 60), [0, 0, 60], [0, 0, 60], (60, 2400), True),
                  ((500, 0, 0), [0, 0, 0], [0, 0, 0], (0, 500), False),         # empty: the exchange jumps over it
                  ((2400, 60, 60), [60, 0, 0], [60, 0, 0], (0, 2340), True)],
    "all_to_all": [((300, 432, 437), [0, 218, 214], [0, 224, 213], (150, 150), False),  # more ghost rows than local rows, no interior
                   ((300, 444, 427), [224, 0, 220], [218, 0, 209], (150, 150), False),
                   ((300, 422, 434), [213, 209, 0], [214, 220, 0], (150, 150), False)],
    "scattered": [((4096, 50, 51), [0, 50, 0], [0, 51, 0], (0, 4035), True),
                  ((4096, 102, 101), [51, 0, 51], [50, 0, 51], (701, 3500), True),  # boundary spans of 701 and 596 rows
                  ((4096, 51, 51), [0, 51, 0], [0, 51, 0], (57, 4096), True)],
    "unequal": [((333, 1, 1), [0, 1, 0], [0, 1, 0], (0, 332), False),
                ((1, 2, 2), [1, 0, 1], [1, 0, 1], (0, 0), False),               # one row, two ghosts, two sends
                ((366, 1, 1), [0, 1, 0], [0, 1, 0], (1, 366), False)],
}


def test_every_problem_is_listed():
    assert set(EXPECTED) == set(PP.NAMES)


@pytest.mark.parametrize("name", PP.NAMES)
def test_plan_counts(name):
    p = PP.problem(name)
    facts = PP.rank_facts(p)
    assert len(facts) == len(EXPECTED[name]) == p.nranks
    for r, (f, (sizes, recv, send, interior, overlaps)) in enumerate(zip(facts, EXPECTED[name])):
        assert (f["m_local"], f["n_ghost"], f["n_send"]) == sizes, (name, r, f)
        assert f["recv_counts"] == recv and f["send_counts"] == send, (name, r, f)
        assert f["interior"] == interior and f["overlaps"] == overlaps, (name, r, f)
    # what one rank receives from another is what that one sends to it, row for row
    plans = PP.plans(p)
    for dst in range(p.nranks):
        at = 0
        for src in range(p.nranks):
            n = int(plans[dst].recv_counts[src])
            so = int(plans[src].send_counts[:dst].sum())
            assert int(plans[src].send_counts[dst]) == n
            assert np.array_equal(plans[src].send_rows[so:so + n] + p.starts[src], plans[dst].ghost_globals[at:at + n])
            at += n


@pytest.mark.parametrize("name", PP.NAMES)
def test_plans_of_matches_the_plans_rank_threads_make(name):
    """HaloPlan on threads that gather through a barrier (what the rank emulations do) gives the plans made here without threads"""
    import partition_ranks as PR
    from rails_amd import partition

    p = PP.problem(name)
    ranks = PR.MailboxRanks(p.nranks)
    got = ranks.run(lambda r: partition.HaloPlan(p.starts, r, p.block(r)[1], ranks.all_gather_object(r)))
    for a, b in zip(got, PP.plans(p)):
        for field in ("col_local", "ghost_globals", "recv_counts", "send_rows", "send_counts"):
            assert np.array_equal(getattr(a, field), getattr(b, field)), (name, field)


@pytest.mark.parametrize("name", PP.NAMES)
def test_conditions_of_the_exact_reference(name):
    p = PP.problem(name)
    assert np.array_equal(p.val, np.rint(p.val)) and np.abs(p.val).min() >= 1 and np.abs(p.val).max() <= 8
    assert np.diff(p.rowptr).max() <= 40 and np.diff(p.rowptr).min() >= 1
    X = R.int_panel(p.m, 130)
    assert np.array_equal(X, np.rint(X)) and np.abs(X).max() <= 16
    assert p.col.min() >= 0 and p.col.max() < p.m
    # a rank's block with its local numbering is a permutation of the row's terms: the same exact sums
    ref = R.spmm_exact_int(p.rowptr, p.col, p.val, X[:, :3])
    for r, plan in enumerate(PP.plans(p)):
        r0, r1 = int(p.starts[r]), int(p.starts[r + 1])
        rowptr, colg, val = p.block(r)
        ext = np.vstack([X[r0:r1, :3], X[plan.ghost_globals, :3]])
        assert np.array_equal(R.spmm_exact_int(rowptr, plan.col_local, val, ext), ref[r0:r1])


def test_wrap_skip_float_matrix_is_symmetric_and_strictly_diagonally_dominant():
    A = PP.problem("wrap_skip").matrix
    assert (A != A.T).nnz == 0
    d = A.diagonal()
    off = np.asarray(abs(A).sum(1)).ravel() - np.abs(d)
    assert np.all(d == 4.0) and np.all(off < d) and off.max() == 3.0
    p = PP.problem("wrap_skip")
    assert np.array_equal(A.indptr, p.rowptr) and np.array_equal(A.indices, p.col)  # the integer copy has the same pattern
    # each block tridiagonal on its own, row i < 60 coupled with row 5299 - i
    C = A.tocoo()
    far = np.abs(C.row - C.col) > 1
    assert sorted(zip(C.row[far], C.col[far])) == sorted([(i, 5299 - i) for i in range(60)] + [(5299 - i, i) for i in range(60)])
    assert A[2399, 2400] == 0 and A[2899, 2900] == 0 and A[2398, 2399] == -1


def test_one_way_float_matrix_is_lower_triangular_and_strictly_diagonally_dominant():
    p = PP.problem("one_way")
    A = p.matrix
    C = A.tocoo()
    assert np.all(C.col <= C.row) and np.all(C.row - C.col <= 40)
    d = A.diagonal()
    off = np.asarray(abs(A).sum(1)).ravel() - np.abs(d)
    assert np.array_equal(d, 1.0 + off)
    assert np.array_equal(A.indptr, p.rowptr) and np.array_equal(A.indices, p.col)
