"""A rank emulation whose ghost-row exchange is point to point, as the real exchanges are (partition.make_halo, rails_rccl_halo): rank
threads in one process on device 0, the interface of tests/test_gpu_partition.py's Ranks (all_gather_object, allreduce, halo, run), so
that _rank_setup and iter_partition_cases.run_ranks take either.  Not a test module.

Ranks' halo hook meets all ranks at the barrier its all-reduce uses: a rank that rails_spmm does not send into the exchange (no ghost
rows and nothing to send) would trip the next all-reduce's barrier with mixed participants, so a plan in which only some ranks exchange
cannot be run there.  Here the all-reduce and the all-gather keep a barrier of their own over all ranks -- every rank takes part in
every one of those -- and the halo hook uses one mailbox per ordered pair (src, dst): a rank puts a copy of its slice for every
destination it sends to, then takes one message from every source it receives from, and nothing else happens.  A rank whose hook is
never called meets nobody.  Messages carry the sender's count of exchanges and the width, so an exchange that pairs up with the wrong
one fails instead of delivering.

A wait that times out, or an exception on one rank, aborts the other ranks' waits and is re-raised by run(): a test failure, and no wait
on the device (every hook has synchronised its context before it blocks)."""
import queue
import threading
import time

import numpy as np

WAIT = 60.0  # seconds a rank waits for a message before it gives up
POLL = 0.05


class Aborted(RuntimeError):
    """another rank failed while this one waited"""


class MailboxRanks:
    def __init__(self, n):
        self.n = n
        self.barrier = threading.Barrier(n, timeout=120)
        self.slots = [None] * n
        self.box = {(s, d): queue.Queue() for s in range(n) for d in range(n) if s != d}
        self.failed = threading.Event()
        self.errors = []
        self.exchanges = [0] * n  # halo hook calls per rank

    # ---- collectives of all ranks ---------------------------------------------------------------------------------------------
    def all_gather_object(self, rank):
        def fn(obj):
            self.slots[rank] = obj
            self.barrier.wait()
            out = list(self.slots)
            self.barrier.wait()
            return out
        return fn

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

    # ---- the point-to-point exchange ------------------------------------------------------------------------------------------
    def _take(self, src, dst):
        deadline = time.monotonic() + WAIT
        while True:
            if self.failed.is_set():
                raise Aborted("rank %d: another rank failed while this one waited for rank %d" % (dst, src))
            try:
                return self.box[(src, dst)].get(timeout=POLL)
            except queue.Empty:
                if time.monotonic() > deadline:
                    raise TimeoutError("rank %d: no ghost rows from rank %d within %g s" % (dst, src, WAIT)) from None

    def halo(self, rank, ctx, plan):
        import torch
        from rails_amd.partition import wrap_buffer

        def exchange(send_ptr, recv_ptr, ncols):
            ctx.sync()
            seq = self.exchanges[rank]
            self.exchanges[rank] += 1
            if plan.n_send:
                send = wrap_buffer(send_ptr, plan.n_send * ncols, True).cpu().numpy()
                so = 0
                for dst in range(self.n):  # the send buffer is grouped by destination, ranks ascending
                    ns = int(plan.send_counts[dst]) * ncols
                    if ns:
                        self.box[(rank, dst)].put((seq, ncols, send[so:so + ns].copy()))
                    so += ns
            if plan.n_ghost:
                recv = np.empty(plan.n_ghost * ncols)
                ro = 0
                for src in range(self.n):  # the ghost rows are grouped by owner, ranks ascending
                    nr = int(plan.recv_counts[src]) * ncols
                    if nr:
                        their_seq, their_ncols, piece = self._take(src, rank)
                        assert their_ncols == ncols and piece.size == nr, (rank, src, their_seq, their_ncols, ncols, piece.size, nr)
                        recv[ro:ro + nr] = piece
                    ro += nr
                wrap_buffer(recv_ptr, plan.n_ghost * ncols, True).copy_(torch.from_numpy(recv))
                torch.cuda.synchronize()
            return 0

        def hook(send_ptr, recv_ptr, ncols, stream):
            try:
                return exchange(send_ptr, recv_ptr, ncols)
            except BaseException as e:  # noqa: BLE001 - the library only sees a code: keep the reason for run()
                self._fail(rank, e)
                raise
        return hook

    # ---- the threads ----------------------------------------------------------------------------------------------------------
    def _fail(self, rank, e):
        self.errors.append((rank, e))
        self.failed.set()
        self.barrier.abort()

    def run(self, target):
        """target(rank) -> result, one thread per rank; re-raises the first failure that is not another rank's failure seen from here"""
        results = [None] * self.n

        def body(r):
            try:
                results[r] = target(r)
            except BaseException as e:  # noqa: BLE001 - reported to the main thread
                self._fail(r, e)
        threads = [threading.Thread(target=body, args=(r,)) for r in range(self.n)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(600)
        if self.errors:
            echo = (threading.BrokenBarrierError, Aborted)
            real = [e for e in self.errors if not isinstance(e[1], echo)] or self.errors
            raise real[0][1]
        left = {k: q.qsize() for k, q in self.box.items() if q.qsize()}
        assert not left, "messages nobody took (src, dst) -> count: %r" % left
        return results
