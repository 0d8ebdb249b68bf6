"""The solution object on a row partition: two and three rank threads on ONE GPU, each with its own context and row block of U, the
all-reduce hook exchanging through host memory between the threads (the Ranks pattern of tests/test_gpu_partition.py).  trace, variance,
pairs and maps of the split U equal the single-rank results -- variance and pairs bit for bit (they are row-local), trace and maps within
their bounds (the sums are all-reduced in another order) -- with the reference unknowns of the maps on different ranks; a reference
unknown that no rank or two ranks claim is refused on every rank alike."""
import ctypes as C
import threading

import numpy as np
import pytest

import covariance_reference as CR
import solution_reference as R

pytestmark = pytest.mark.gpu

_i32p = C.POINTER(C.c_int32)
EINVAL = -1
M, K = 129, 33
SPLITS = {2: (0, 50, M), 3: (0, 40, 41, M)}  # a rank with a single row among three


class Ranks:
    """In-process stand-in for the collectives: rank threads meet at a barrier and exchange numpy arrays."""

    def __init__(self, n):
        self.n = n
        self.barrier = threading.Barrier(n, timeout=120)
        self.slots = [None] * n
        self.errors = []

    def allreduce(self, rank, ctx):
        import torch
        from rails_amd.partition import wrap_buffer

        def hook(ptr, n, stream):
            ctx.sync()  # the library's stream has produced the buffer
            t = wrap_buffer(ptr, n, True)
            self.slots[rank] = t.cpu().numpy().copy()
            self.barrier.wait()
            total = np.zeros(n)
            for r in range(self.n):  # fixed order: every rank gets the same bits
                total += self.slots[r]
            self.barrier.wait()
            t.copy_(torch.from_numpy(total))
            torch.cuda.synchronize()
            return 0
        return hook

    def run(self, target):
        """target(rank) -> result, one thread per rank; re-raises the first failure."""
        results = [None] * self.n

        def body(r):
            try:
                results[r] = target(r)
            except BaseException as e:  # noqa: BLE001 - reported to the main thread
                self.errors.append((r, e))
                self.barrier.abort()
        threads = [threading.Thread(target=body, args=(r,)) for r in range(self.n)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(600)
        if self.errors:
            real = [e for e in self.errors if not isinstance(e[1], threading.BrokenBarrierError)] or self.errors
            raise real[0][1]
        return results


def _problem():
    U, S = CR.corr_problem(M, K, 5)  # row 5 of U is zero
    ref = np.array([0, 5, 40, 45, 60, M - 1, 40], dtype=np.int64)  # on every rank of either split, one twice, the zero row
    g = np.random.default_rng(3)
    # random pairs, and a few that every rank of either split holds whole (the single row 40 of the three-rank split among them)
    ia = np.concatenate([[40, 0, 5, 60, M - 1, 45], g.integers(0, M, 400)])
    ib = np.concatenate([[40, 5, 0, M - 1, 60, 41], g.integers(0, M, 400)])
    return U, S, ref, ia, ib


@pytest.fixture(scope="module")
def single():
    import rails_amd

    U, S, ref, ia, ib = _problem()
    ctx = rails_amd.Context(device=0, seed=1)
    sol = rails_amd.Solution(ctx, U, S)
    out = dict(trace=sol.trace(), variance=sol.variance(), pairs=sol.covariance(ia.astype(np.int32), ib.astype(np.int32)),
               maps=sol.maps(ref.astype(np.int32)), corr=sol.maps(ref.astype(np.int32), correlation=True))
    sol.close()
    ctx.close()
    return out


def _local(ref, r0, r1):
    return np.where((ref >= r0) & (ref < r1), ref - r0, -1).astype(np.int32)


@pytest.mark.parametrize("nranks", [2, 3])
def test_row_split_equals_single_rank(single, nranks):
    import rails_amd

    U, S, ref, ia, ib = _problem()
    starts = SPLITS[nranks]
    ranks = Ranks(nranks)

    def target(r):
        r0, r1 = starts[r], starts[r + 1]
        ctx = rails_amd.Context(device=0, seed=1)
        ctx.set_partition(r, nranks, r0, M)
        ctx.set_allreduce(ranks.allreduce(r, ctx))
        sol = rails_amd.Solution(ctx, U[r0:r1], S)
        mine = (ia >= r0) & (ia < r1) & (ib >= r0) & (ib < r1)
        out = dict(trace=sol.trace(), variance=sol.variance(), mine=mine,
                   pairs=sol.covariance((ia[mine] - r0).astype(np.int32), (ib[mine] - r0).astype(np.int32)),
                   maps=sol.maps(_local(ref, r0, r1)), corr=sol.maps(_local(ref, r0, r1), correlation=True))
        sol.close()
        ctx.close()
        return out

    res = ranks.run(target)
    assert len({tuple(np.flatnonzero(_local(ref, starts[r], starts[r + 1]) >= 0)) for r in range(nranks)}) == nranks  # owners differ
    for r, out in enumerate(res):
        r0, r1 = starts[r], starts[r + 1]
        assert abs(out["trace"] - res[0]["trace"]) == 0.0  # every rank holds the same sum
        assert abs(out["trace"] - single["trace"]) <= 2 * R.trace_bound(U, S)
        assert np.array_equal(R.bits(out["variance"]), R.bits(single["variance"][r0:r1]))
        assert out["mine"].any() and np.array_equal(R.bits(out["pairs"]), R.bits(single["pairs"][out["mine"]]))
        mb = CR.maps_bound(U, S, ref)[r0:r1]
        assert np.all(np.abs(out["maps"] - single["maps"][r0:r1]) <= 2 * mb)
        assert np.all(np.abs(np.asarray(out["maps"] - CR.maps(U, S, ref)[r0:r1], dtype=np.float64)) <= mb)
        cb = CR.correlations_bound(U, S, ref)[r0:r1]
        assert np.all(np.abs(out["corr"] - single["corr"][r0:r1]) <= 2 * cb)
        assert np.all(np.abs(np.asarray(out["corr"] - CR.correlations(U, S, ref)[r0:r1], dtype=np.float64)) <= cb)
        assert np.all(out["corr"][:, 1] == 0.0)  # the zero row as a reference unknown, owned by rank 0
    assert np.all(res[0]["corr"][5] == 0.0)
    for j, g in enumerate(ref):
        if g != 5:
            r = max(q for q in range(nranks) if starts[q] <= g)
            assert res[r]["corr"][g - starts[r], j] == 1.0


@pytest.mark.parametrize("nranks", [2, 3])
def test_unowned_and_doubly_owned_reference_unknowns_are_refused_everywhere(nranks):
    import rails_amd

    U, S, _, _, _ = _problem()
    starts = SPLITS[nranks]
    ranks = Ranks(nranks)
    # local rows per rank: unknown 0 nobody's; unknown 1 claimed by ranks 0 and 1; an index outside rank 1's rows; then a good call
    cases = {
        "unowned": lambda r: np.array([-1, 3 if r == 0 else -1], dtype=np.int32),
        "twice": lambda r: np.array([3 if r == 0 else -1, 0 if r <= 1 else -1], dtype=np.int32),
        "outside": lambda r: np.array([3 if r == 0 else -1, (starts[2] - starts[1]) if r == 1 else -1], dtype=np.int32),
        "good": lambda r: np.array([3 if r == 0 else -1, 0 if r == 1 else -1], dtype=np.int32),
    }

    def target(r):
        r0, r1 = starts[r], starts[r + 1]
        ctx = rails_amd.Context(device=0, seed=1)
        ctx.set_partition(r, nranks, r0, M)
        ctx.set_allreduce(ranks.allreduce(r, ctx))
        sol = rails_amd.Solution(ctx, U[r0:r1], S)
        got = {}
        for corr in (0, 1):
            for name, rows in cases.items():
                out = rails_amd.HipMultiVectorWrapper(ctx, data=np.full((r1 - r0, 3), 7.0))
                idx = rows(r)
                rc = sol.lib.rails_solution_maps(sol.h, idx.ctypes.data_as(_i32p), 2, corr, out.panel.h, 0, -1)
                got[(corr, name)] = (rc, out.to_host())
        sol.close()
        ctx.close()
        return got

    res = ranks.run(target)
    want = CR.maps(U, S, np.array([3, starts[1]]))
    for r, got in enumerate(res):
        r0, r1 = starts[r], starts[r + 1]
        for corr in (0, 1):
            for name in ("unowned", "twice", "outside"):
                rc, host = got[(corr, name)]
                assert rc == EINVAL and np.all(host == 7.0), (r, corr, name)
            rc, host = got[(corr, "good")]
            assert rc == 0 and np.all(host[:, 2] == 7.0)
        err = np.abs(np.asarray(got[(0, "good")][1][:, :2] - want[r0:r1], dtype=np.float64))
        assert np.all(err <= CR.maps_bound(U, S, np.array([3, starts[1]]))[r0:r1])
