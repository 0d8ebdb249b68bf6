"""The cases of the row-partitioned iterative A^-1 tests and the rank emulation they share.  Not a test module:
tests/test_iter_partition_host.py checks the step cases' conditions on the CPU, tests/test_gpu_iter_partition_steps.py,
test_gpu_iter_partition.py and test_gpu_iter_partition_solver.py run on the GPU.

A partition is one more order of summation of the inner products, so the step cases are those of tests/iter_steps_reference.py (its
matrices, right-hand sides, bounds and conditions) at the shapes at which a partition can go wrong.  The matrices are tridiagonal: every
rank has one or two ghost rows.  The rank emulation is that of tests/test_gpu_partition.py (rank threads in one process on device 0,
hooks that meet at a barrier)."""
import numpy as np

import iter_steps_reference as S

RANKS = (2, 3)
_VARIANT = {v[0]: v for v in S.VARIANTS}
# polynomial cases at widths that are not in S.CASES (ghost rows at odd widths through the fused step), with the steps of their shape
CONSTRUCTED = [S.Case(_VARIANT[name], 72, w, S.SHAPES[72][1]) for name in ("cg-poly-fused", "cg-poly-unfused") for w in (1, 17)]


def _listed(name, m, w):
    return S.case("%s-m%d-w%d" % (name, m, w))


def _step_cases():
    out = []
    # 3 + 2 and 2 + 2 + 1 rows: a one-row rank, fewer rows than row classes
    out += [(_listed(n, 5, w), RANKS) for n in ("cg-jacobi", "bicgstab-jacobi") for w in (2, 3)]
    # every tx_bits class, odd last columns, three groups with the scalar block at 32 and 64
    out += [(_listed(n, 72, w), RANKS) for n in ("cg-jacobi", "cg-plain", "bicgstab-jacobi", "bicgstab-plain") for w in (1, 3, 17, 32, 70)]
    out += [(_listed("cg-negated-plain", 72, 3), RANKS)]  # defsign -1 agreed over the ranks
    out += [(_listed(n, 72, w), RANKS) for n in ("cg-poly-fused", "cg-poly-unfused") for w in (3, 32)]
    out += [(c, RANKS) for c in CONSTRUCTED]
    # several slabs per rank; a group of 32, then a group of 1
    out += [(_listed(n, 2181, w), RANKS) for n in ("cg-jacobi", "bicgstab-jacobi") for w in (17, 33)]
    out += [(_listed("cg-poly-fused", 2181, w), (2,)) for w in (3, 32)]
    return out


STEP_CASES = _step_cases()
STEP_PARAMS = [(c.id, n) for c, ranks in STEP_CASES for n in ranks]
_by_id = {c.id: c for c, _ in STEP_CASES}


def step_case(case_id):
    return _by_id[case_id]


def csr_triple(A):
    """(rowptr, col, val) of a scipy matrix, as rails_amd.problems.csr_rows takes it"""
    import scipy.sparse as sp

    A = sp.csr_matrix(A)
    A.sort_indices()
    return A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data.astype(np.float64)


def run_ranks(nranks, A, work, seed=3, starts=None, ranks=None, every_rank_has_ghosts=True):
    """work(r, ctx, op, plan, r0, r1) -> result on every rank of a row partition of the CSR triple A, one thread per rank; the contexts
    are closed afterwards.  Returns the results in rank order.  starts: the row blocks (default: balanced).  ranks: the emulation
    (default: test_gpu_partition.Ranks; tests/partition_ranks.py's for plans in which not every rank exchanges -- those, and only those,
    pass every_rank_has_ghosts=False)."""
    from rails_amd import partition
    from test_gpu_partition import Ranks, _rank_setup

    m = A[0].size - 1
    if starts is None:
        starts = partition.row_ranges(m, nranks)
    assert len(starts) == nranks + 1 and int(starts[-1]) == m
    if ranks is None:
        ranks = Ranks(nranks)

    def body(r):
        ctx, op, plan = _rank_setup(ranks, r, starts, A, seed=seed)
        try:
            assert plan.n_ghost > 0 or not every_rank_has_ghosts  # rows really cross the partition, on every rank
            return work(r, ctx, op, plan, int(starts[r]), int(starts[r + 1]))
        finally:
            ctx.close()

    return ranks.run(body)
