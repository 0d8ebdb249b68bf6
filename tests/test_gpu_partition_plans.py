"""Row-partitioned products and solves on the ghost-row plans of tests/partition_plans.py: a rank that only sends and one that only
receives (one_way), an empty rank the exchange jumps over (wrap_skip), every rank exchanging with every other and no interior rows
(all_to_all), boundary rows in the middle of a block (scattered), a rank of one row (unequal).  The other partition tests run balanced
banded, tridiagonal and grid-stencil blocks, where every rank sends to and receives from its neighbours only.

(a) One context plays one rank.  Its halo hook first compares the packed send buffer with the rows of X the plan lists, in plan order, bit
    for bit (k_pack_rows, the grouping by destination), then writes the ghost rows from the global X; on an empty plan it must not be
    called.  The product is spmm_reference.spmm_exact_int's bit for bit, into a window of a panel filled with a sentinel that must
    survive beside the window, with RAILS_SPMM_HALO_OVERLAP on and off; the kernel is the one KERNEL_TABLE lists, and the overlapped
    order is taken exactly on the ranks partition_plans.overlaps() names.
(b) The same plans on rank threads whose exchange is point to point (tests/partition_ranks.py): the stacked panel is exact.
(c) The iterative inverse where ranks take different forms of the fused Chebyshev step: conjugate gradients on wrap_skip (ranks 0 and 2
    exchange and run the ghost-row form, rank 1 the plain form without an exchange), BiCGStab on one_way, and `precondition` alone on
    both (one_way: a rank that only sends runs the ghost-row form against a ghost buffer of one row) against a longdouble evaluation.
    Bounds: those of tests/test_gpu_iter_partition.py and of test_gpu_iter_partition_steps.py::poly_expected.

The module reports, per plan and rank, the kernels reached and whether a product overlapped, and per `precondition` case the largest
error / bound with the bound.  Measured on MI355X, degree 2, ratio 30: wrap_skip 0.031 / 0.030 / 0.026 at 3 / 17 / 32 columns (bounds
1.16e-14, 1.37e-14, 1.39e-14: the floor of 64 eps |y|_inf), one_way 0.051 / 0.064 / 0.067 (3.47e-14, 3.09e-14, 3.49e-14), fused and
unfused alike."""
import numpy as np
import pytest

import cheb_reference as C
import iter_partition_cases as PC
import iter_reference as R
import iter_steps_reference as S
import partition_plans as PP
import partition_ranks as PR
import spmm_reference as SR

pytestmark = pytest.mark.gpu

SENTINEL = -777.25  # no product of integers
MAX_COLS = 130
RG, CC, NW = "k_spmm_rowgather", "k_spmm_rowgather_cc", "k_spmm_narrow"

# (variant, widths, X offset, Y offsets) -> the row kernel on a rank without an exchange / one that only sends / one with ghost rows in
# the serial order / the boundary rows of one with ghost rows in the overlapped order.  The rule is row_choice.h's ("Which row
# kernel runs"); every row has at most 11 entries and fewer than 2^24 columns.  With an exchange the ghost rows are packed with leading
# dimension nc (rails_spmm: p.ldg = nc), so an odd width makes x_vec2 false; without one "the ghost rows" are X itself.
KERNEL_TABLE = (
    # nc <= 8: narrow_width needs nc > 8 -- the plain kernel, 1 / 1 / 2 / 4 lanes per row (plain_lpr of need = ceil(nc / 2))
    (1, (1, 2, 3, 6), 0, (0, 1), RG, RG, RG, RG),
    # 8 < nc <= 16, x_vec2: lpr = 8 and nc <= 2 lpr -- the lean kernel; `flat` without ghost rows (n_ghost == 0, span_ghost == 0), else
    # its ghost form behind two bases (`small && !flat && !rect`); a Y window on an odd column only changes the stores (y_vec)
    (1, (12, 16), 0, (0, 1), NW, NW, NW, NW),
    # X rows that are only 8-byte aligned: `narrow_width && serial && !x_vec2 && nc <= 16` -- the lean kernel on the serial path only;
    # a span falls through to the plain kernel, 8 lanes per row
    (1, (12, 16), 1, (0, 1), NW, NW, NW, RG),
    # 17 columns: without an exchange ldg is X's own even leading dimension, x_vec2 holds, lpr = 16 -- the lean kernel.  With one the
    # packed ghost rows have an odd stride: x_vec2 fails, 17 > 16 -- the plain kernel, 16 lanes per row (need = 9)
    (1, (17,), 0, (0, 1), NW, RG, RG, RG),
    # 16 < nc <= 32, x_vec2: lpr = 16 -- the lean kernel's other lane count
    (1, (24, 32), 0, (0, 1), NW, NW, NW, NW),
    # wider than 32 on a variant without chunks: the plain kernel, 32 / 32 / 64 lanes per row
    (1, (33, 64, 130), 0, (0, 1), RG, RG, RG, RG),
    # variant 4: chunks of 32 columns for nc > 32 on the serial path between aligned windows (`serial && vec2`), and 48 > 2 lpr keeps the
    # lean kernel out -- the chunked kernel, ghost rows included; variant 4 never overlaps (rails_halo_order: variants 0 / 1 / 3)
    (4, (48, 130), 0, (0,), CC, CC, CC, CC),
    # ... a Y window on an odd column: vec2 fails, no chunks, nc > 32 -- the plain kernel
    (4, (48, 130), 0, (1,), RG, RG, RG, RG),
)
KINDS = ("empty", "send_only", "ghost", "ghost_overlapped")
PRODUCTS = {v: [(nc, xoff, yoff) for (var, widths, xoff, yoffs, *_k) in KERNEL_TABLE if var == v for nc in widths for yoff in yoffs] for v in (1, 4)}
KERNEL = {(var, nc, xoff, yoff): dict(zip(KINDS, names)) for (var, widths, xoff, yoffs, *names) in KERNEL_TABLE for nc in widths for yoff in yoffs}


def test_the_table_covers_what_it_should():
    widths = {nc for (nc, xoff, yoff) in PRODUCTS[1]}
    assert widths == {1, 2, 3, 6, 12, 16, 17, 24, 32, 33, 64, 130} and {nc for (nc, _, _) in PRODUCTS[4]} == {48, 130}
    assert {k["ghost"] for k in KERNEL.values()} == {RG, CC, NW}  # all three kernels run with ghost rows
    assert any(xoff == 1 and nc <= 16 for (nc, xoff, yoff) in PRODUCTS[1])
    assert {yoff for (_, _, yoff) in PRODUCTS[1]} == {0, 1}


_operands = {}


def operands(name):
    """the problem, its integer panel of 130 columns and the exact product, computed once"""
    if name not in _operands:
        p = PP.problem(name)
        X = SR.int_panel(p.m, MAX_COLS)
        ref = SR.spmm_exact_int(p.rowptr, p.col, p.val, X).astype(np.float64)
        for a in (X, ref):
            a.setflags(write=False)
        _operands[name] = (p, X, ref)
    return _operands[name]


class OneRank:
    """one context as rank r of problem p; the hook checks what was packed and supplies the ghost rows"""

    def __init__(self, name, rank):
        import rails_amd

        self.p, self.X, self.ref = operands(name)
        p = self.p
        self.rank, self.plan = rank, PP.plans(p)[rank]
        self.r0, self.r1 = int(p.starts[rank]), int(p.starts[rank + 1])
        rowptr, _, val = p.block(rank)
        self.rowptr = rowptr
        self.ctx = rails_amd.Context(device=0, seed=5)
        self.op = rails_amd.HipOperatorWrapper(self.ctx, rowptr, self.plan.col_local, val, ncols_ext=self.plan.m_local + self.plan.n_ghost)
        self.calls, self.problems, self.nc = 0, [], None
        self.op.set_halo(self.plan, self.hook)
        plan = self.plan
        self.kind = "empty" if plan.n_ghost == 0 and plan.n_send == 0 else "send_only" if plan.n_ghost == 0 else "ghost"
        self.interior = PP.interior(rowptr, plan.col_local, plan.m_local, plan.n_ghost)

    def hook(self, send_ptr, recv_ptr, ncols, stream):
        import torch
        from rails_amd.partition import wrap_buffer

        plan = self.plan
        self.calls += 1
        self.ctx.sync()
        if ncols != self.nc:
            self.problems.append("exchange of %d columns in a product of %d" % (ncols, self.nc))
            return 1
        if plan.n_send:
            packed = wrap_buffer(send_ptr, plan.n_send * ncols, True).cpu().numpy().reshape(plan.n_send, ncols)
            want = self.X[plan.send_rows + self.r0, :ncols]
            if not np.array_equal(packed, want):
                bad = np.flatnonzero((packed != want).any(1))
                self.problems.append("packed rows differ at %d columns: %d of %d, first at position %d" % (ncols, bad.size, plan.n_send, bad[0]))
        if plan.n_ghost:
            ghosts = np.ascontiguousarray(self.X[plan.ghost_globals, :ncols]).ravel()
            wrap_buffer(recv_ptr, plan.n_ghost * ncols, True).copy_(torch.from_numpy(ghosts))
            torch.cuda.synchronize()
        return 0

    def product(self, nc, xoff, yoff):
        """Y window <- A * X window: (last_kernel, whole Y panel on the host, hook calls, overlapped products counted)"""
        from rails_amd.wrappers import HipMultiVectorWrapper as MV

        ml = self.plan.m_local
        big = MV(self.ctx, m=ml, n=nc + xoff, capacity=nc + xoff)
        big.assign(SENTINEL)
        Xw = big.view(xoff, xoff + nc - 1)
        Xw.from_host(self.X[self.r0:self.r1, :nc])
        out = MV(self.ctx, m=ml, n=nc + yoff + 1, capacity=nc + yoff + 1)
        out.assign(SENTINEL)
        self.nc = nc
        calls0, over0 = self.calls, self.ctx.stats()["spmm_halo_overlapped"]
        self.op.apply(Xw, out.view(yoff, yoff + nc - 1))
        kernel = self.op.last_kernel()
        return kernel, out.to_host(), self.calls - calls0, self.ctx.stats()["spmm_halo_overlapped"] - over0

    def check(self, variant, nc, xoff, yoff, overlap_on, kernels=True):
        tag = (self.p.name, self.rank, variant, nc, xoff, yoff, overlap_on)
        kernel, H, calls, overlapped = self.product(nc, xoff, yoff)
        assert not self.problems, (tag, self.problems)
        assert calls == (0 if self.kind == "empty" else 1), (tag, calls)
        assert np.array_equal(H[:, yoff:yoff + nc], self.ref[self.r0:self.r1, :nc]), (tag, kernel, np.abs(H[:, yoff:yoff + nc] - self.ref[self.r0:self.r1, :nc]).max())
        assert np.all(H[:, :yoff] == SENTINEL) and np.all(H[:, yoff + nc:] == SENTINEL), tag
        lo, hi = self.interior
        want_overlap = overlap_on and PP.overlaps(self.plan.m_local, self.plan.n_ghost, lo, hi, variant)
        if kernels:
            assert overlapped == (1 if want_overlap else 0), (tag, overlapped)
            name = KERNEL[(variant, nc, xoff, yoff)]["ghost_overlapped" if want_overlap else self.kind]
            assert kernel == name + (" (halo overlapped)" if want_overlap else ""), (tag, kernel)
        return kernel, bool(overlapped)

    def close(self):
        self.ctx.close()


_reached = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for key in sorted(_reached):
        print("\n%s rank %d (%s): overlapped %s; kernels %s" % (key + (_reached[key]["overlapped"], ", ".join(sorted(_reached[key]["kernels"])))), end="")
    for key in sorted(_precondition_worst):
        print("\nprecondition on %s, %d columns, fused %d: largest error / bound %.3f, bound %.3e" % (key + _precondition_worst[key]), end="")
    print()


ALL_RANKS = [(name, r) for name in PP.NAMES for r in range(3)]


# ------------------------------------------------------------------------------------------------- (a) one context, one rank
@pytest.mark.parametrize("name,rank", ALL_RANKS)
def test_every_rank_of_every_plan_is_exact(monkeypatch, name, rank):
    one = OneRank(name, rank)
    try:
        seen = _reached.setdefault((name, rank, one.kind), dict(kernels=set(), overlapped=False))
        for variant in (1, 4):
            one.op.set_variant(variant)
            for nc, xoff, yoff in PRODUCTS[variant]:
                for mode in ("1", "0"):
                    monkeypatch.setenv("RAILS_SPMM_HALO_OVERLAP", mode)
                    kernel, overlapped = one.check(variant, nc, xoff, yoff, mode == "1")
                    seen["kernels"].add(kernel)
                    seen["overlapped"] = seen["overlapped"] or overlapped
        # the ranks listed as overlapping, and only those (tests/test_partition_plans_host.py pins which)
        assert seen["overlapped"] == PP.rank_facts(one.p)[rank]["overlaps"]
    finally:
        one.close()


@pytest.mark.parametrize("name,rank", [(name, r) for name in ("one_way", "scattered") for r in range(3)])
def test_automatic_variant_is_exact(monkeypatch, name, rank):
    """variant 0 at 16 and 128 columns: the serial automatic order may pick a whole-operator kernel (the send-only rank has no ghost rows),
    the overlapped one tries the plane and sweep kernels on the interior rows first -- whatever runs, the product is exact"""
    one = OneRank(name, rank)
    try:
        one.op.set_variant(0)
        for nc in (16, 128):
            for mode in ("1", "0"):
                monkeypatch.setenv("RAILS_SPMM_HALO_OVERLAP", mode)
                one.check(0, nc, 0, 0, mode == "1", kernels=False)
    finally:
        one.close()


# ------------------------------------------------------------------------------------------------- (b) rank threads, point to point
def _threads_product(ranks, starts, A, Xg, widths, extra=None):
    """every rank's A * X[:, :nc] for the widths, on rank threads: per rank a dict"""
    from rails_amd.wrappers import HipMultiVectorWrapper as MV
    from test_gpu_partition import _rank_setup

    def work(r):
        ctx, op, plan = _rank_setup(ranks, r, starts, A, seed=5)
        try:
            r0, r1 = int(starts[r]), int(starts[r + 1])
            out = {nc: op.apply(MV(ctx, data=Xg[r0:r1, :nc])).to_host() for nc in widths}
            out["plan"] = (plan.n_ghost, plan.n_send)
            if extra:
                out.update(extra(ctx, r0, r1))
            return out
        finally:
            ctx.close()

    return ranks.run(work)


def test_mailbox_ranks_give_the_bits_of_barrier_ranks():
    """tests/test_gpu_partition.py::test_partitioned_spmm_and_reductions' problem on both emulations: the same panels and the same
    all-reduced Gram block, bit for bit -- the point-to-point exchange is no weaker a stand-in than the barrier one"""
    from rails_amd import partition
    from rails_amd import problems as P
    from rails_amd.wrappers import HipMultiVectorWrapper as MV
    from test_gpu_partition import Ranks

    nranks, m = 3, 5000
    A = P.banded_random(m, 27, 300, seed=1)
    X = np.random.default_rng(3).uniform(-1, 1, (m, 24))
    starts = partition.row_ranges(m, nranks)

    def gram(ctx, r0, r1):
        Xl = MV(ctx, data=X[r0:r1])
        return {"gram": Xl.view(0, 7).dot(Xl.view(8, 23))}

    mail = PR.MailboxRanks(nranks)
    a = _threads_product(mail, starts, A, X, (24, 16, 3), gram)
    b = _threads_product(Ranks(nranks), starts, A, X, (24, 16, 3), gram)
    for nc in (24, 16, 3):
        assert np.array_equal(np.vstack([a[r][nc] for r in range(nranks)]), np.vstack([b[r][nc] for r in range(nranks)])), nc
    for r in range(nranks):
        assert a[r]["plan"][0] > 0 and mail.exchanges[r] == 3
        assert np.array_equal(a[r]["gram"], b[r]["gram"]) and np.array_equal(a[r]["gram"], a[0]["gram"])


@pytest.mark.parametrize("name", ["wrap_skip", "one_way", "all_to_all"])
def test_plans_on_rank_threads_are_exact(name):
    """the mailboxes route by owner: every ghost row arrives from the rank that owns it, in the order the receiver numbered it"""
    p, X, ref = operands(name)
    widths = (16, 33, 128)
    ranks = PR.MailboxRanks(p.nranks)
    res = _threads_product(ranks, p.starts, p.triple, X, widths)
    for nc in widths:
        Y = np.vstack([res[r][nc] for r in range(p.nranks)])
        assert np.array_equal(Y, ref[:, :nc]), (name, nc, np.abs(Y - ref[:, :nc]).max())
    for r, f in enumerate(PP.rank_facts(p)):
        assert res[r]["plan"] == (f["n_ghost"], f["n_send"])
        assert ranks.exchanges[r] == (len(widths) if f["n_ghost"] or f["n_send"] else 0), (name, r, ranks.exchanges)


# ------------------------------------------------------------------------------------------------- (c) the iterative inverse
TOL = 1e-10
_solve_reference = {}


def solve_reference(problem, K, nc):
    """the restatement's solve on the undivided float matrix (iter_reference.bicgstab; cheb_reference.pcg, which is iter_reference.cg at
    degree 0), computed once: (A, B, Columns)"""
    key = (problem, K, nc)
    if key not in _solve_reference:
        A = PP.problem(problem).matrix
        Bm = R.rhs(A.shape[0], nc)
        if problem == "one_way":
            _, c = R.bicgstab(A, Bm, tol=TOL, maxit=5000)
        else:
            _, c = C.pcg(A, Bm, K, ratio=S.POLY_RATIO, tol=TOL, maxit=5000)
        _solve_reference[key] = (A, Bm, c)
    return _solve_reference[key]


def run_on_mailboxes(problem, work):
    p = PP.problem(problem)
    ranks = PR.MailboxRanks(p.nranks)
    return ranks, PC.run_ranks(p.nranks, PC.csr_triple(p.matrix), work, starts=p.starts, ranks=ranks, every_rank_has_ghosts=False)


SOLVES = [("wrap_skip", "cg", 0, 1), ("wrap_skip", "cg", S.POLY_DEGREE, 1), ("wrap_skip", "cg", S.POLY_DEGREE, 0), ("one_way", "bicgstab", 0, 1)]


@pytest.mark.parametrize("nc", (3, 33))
@pytest.mark.parametrize("problem,method,K,fused", SOLVES)
def test_solves_converge_where_ranks_take_different_forms(problem, method, K, fused, nc):
    """what tests/test_gpu_iter_partition.py::test_partitioned_solves_converge asserts, with its bounds"""
    import rails_amd

    A, Bm, cr = solve_reference(problem, K, nc)

    def work(r, ctx, op, plan, r0, r1):
        inv = rails_amd.IterativeInverse(ctx, op, method=method, tol=TOL, maxit=5000)
        if K:
            inv.set("poly_ratio", S.POLY_RATIO)
            inv.set("poly_fused", fused)
            inv.set("poly_degree", K)
        X = inv.solve(rails_amd.HipMultiVectorWrapper(ctx, data=Bm[r0:r1])).to_host()
        out = dict(X=X, cols=[a.copy() for a in inv.columns()], stats=inv.stats(), plan=(plan.n_ghost, plan.n_send))
        inv.close()
        return out

    ranks, res = run_on_mailboxes(problem, work)
    n = len(res)
    facts = PP.rank_facts(PP.problem(problem))
    it, rel, flags = res[0]["cols"]
    for r in range(n):
        assert res[r]["plan"] == (facts[r]["n_ghost"], facts[r]["n_send"])
        for a, b in zip(res[r]["cols"], res[0]["cols"]):
            assert np.array_equal(a, b)  # the same scalars on every rank
        st = res[r]["stats"]
        assert st["unconverged_columns"] == 0
        exchanges = facts[r]["n_ghost"] > 0 or facts[r]["n_send"] > 0
        if K and fused:  # the last application: one exchange per fused step where the rank exchanges, none on the empty rank
            assert st["fused_launches"] > 0 and st["halo_exchanges"] == (st["fused_launches"] if exchanges else 0), (r, st)
        else:
            assert st["fused_launches"] == 0 and st["halo_exchanges"] == 0, (r, st)
        assert (ranks.exchanges[r] > 0) == exchanges
    X = np.vstack([res[r]["X"] for r in range(n)])
    true_rel = R.true_relres(A, X, Bm)
    print("%s on %s, degree %d, fused %d, %d columns: iterations %d..%d (restatement %d..%d), true relative residual %.2e" % (
        method, problem, K, fused, nc, it.min(), it.max(), cr.iter.min(), cr.iter.max(), true_rel.max()))
    assert np.all(np.isfinite(X)) and true_rel.max() <= 10 * TOL, true_rel.max()
    assert np.all(flags == 2) and np.all(rel <= TOL)
    assert np.all(it <= 1.5 * cr.iter), (it, cr.iter)


_poly_expected = {}
_precondition_worst = {}


def poly_expected(problem, nc):
    """test_gpu_iter_partition_steps.py::poly_expected's rule on the problem's float matrix, degree 2, ratio 30, Jacobi: the longdouble
    polynomial and per column 4 times the float64 restatement's error against it, at least 64 eps |y|_inf"""
    if (problem, nc) not in _poly_expected:
        A = PP.problem(problem).matrix
        g = C.g_of(A, True)
        hi = C.gershgorin(A, g)
        Xm = R.rhs(A.shape[0], nc, seed=9)
        Zl = C.polynomial(A, Xm, S.POLY_DEGREE, hi, S.POLY_RATIO, g, dtype=np.longdouble)
        Z64 = C.polynomial(A, Xm, S.POLY_DEGREE, hi, S.POLY_RATIO, g)
        bound = np.maximum(4 * np.abs(Z64 - Zl).max(0), 64 * S.EPS * np.abs(Zl).max(0)).astype(float)
        _poly_expected[(problem, nc)] = (A, Xm, Zl, bound, hi)
    return _poly_expected[(problem, nc)]


@pytest.mark.parametrize("nc", (3, 17, 32))
@pytest.mark.parametrize("fused", (1, 0))
@pytest.mark.parametrize("problem", ("wrap_skip", "one_way"))
def test_precondition_where_ranks_take_different_forms(problem, fused, nc):
    """The polynomial on its own (17 columns: the pad column travels with the ghost rows).  wrap_skip: ranks 0 and 2 run the ghost-row
    fused step behind an exchange of their own, rank 1 the plain form with no exchange beside them.  one_way (the polynomial of a
    matrix that is not symmetric is still a polynomial): rank 0 runs the ghost-row form against a ghost buffer of one row it never
    reads and only sends, rank 2 only receives."""
    import rails_amd

    A, Xm, Zl, bound, hi = poly_expected(problem, nc)

    def work(r, ctx, op, plan, r0, r1):
        inv = rails_amd.IterativeInverse(ctx, op, method="cg", poly_degree=S.POLY_DEGREE, poly_ratio=S.POLY_RATIO)
        inv.set("poly_fused", fused)
        n0 = ctx.stats()["allreduce"]
        Z = inv.precondition(rails_amd.HipMultiVectorWrapper(ctx, data=Xm[r0:r1])).to_host()
        out = dict(Z=Z, stats=inv.stats(), allreduces=ctx.stats()["allreduce"] - n0)
        inv.close()
        return out

    ranks, res = run_on_mailboxes(problem, work)
    Z = np.vstack([res[r]["Z"] for r in range(3)])
    for r, f in enumerate(PP.rank_facts(PP.problem(problem))):
        exchanges = f["n_ghost"] > 0 or f["n_send"] > 0
        assert exchanges == (not (problem == "wrap_skip" and r == 1))
        st = res[r]["stats"]
        assert st["poly_applications"] == 1 and st["products"] == S.POLY_DEGREE and res[r]["allreduces"] == 0 and st["allreduces"] == 0
        assert st["fused_launches"] == (S.POLY_DEGREE if fused else 0), (r, st)
        assert st["halo_exchanges"] == (st["fused_launches"] if exchanges else 0), (r, st)
        assert ranks.exchanges[r] == (S.POLY_DEGREE if exchanges else 0)  # fused or through rails_spmm: one exchange per product
        assert st["eig_hi"] == res[0]["stats"]["eig_hi"] and abs(st["eig_hi"] - hi) <= 4 * S.EPS * hi
    err = np.abs(Z - Zl).astype(float)
    ratio = float((err.max(0) / bound).max())
    _precondition_worst[(problem, nc, fused)] = (ratio, float(bound.max()))
    print("precondition on %s, %d columns, fused %d: largest error / allowed error %.3f (bound at most %.3e)" % (problem, nc, fused, ratio, bound.max()))
    assert np.all(err <= bound[None, :]), (problem, nc, fused, ratio)
