"""The iterative A^-1 operator on a row partition (rails_amd/csrc/itsolve.hip: k_iter_reduce, the all-reduce, k_iter_compute; the
ghost-row form of k_cheb_step_csr) step by step against the longdouble restatement of tests/iter_steps_reference.py.  A partition is one
more order of summation, so the rule is that module's: tolerance 0 and max_iterations k stop every column after exactly k iterations, the
ranks' rows of x_k stacked and the recurrence's relative residual must lie within its bounds.  Ranks are threads on one device
(tests/test_gpu_partition.py's emulation); the matrices are tridiagonal, every rank has ghost rows.  Beside the bounds: the scalars are the
same bits on every rank, the counts of all-reduces and of ghost-row exchanges are exact, two runs give the same bits, and on a world of
one rank (a hook that changes nothing, the library's own one-rank RCCL communicator) the split scalar step gives the bits of a plain
context."""
import numpy as np
import pytest

import cheb_reference as C
import iter_partition_cases as PC
import iter_reference as R
import iter_steps_reference as S

pytestmark = pytest.mark.gpu

MAXIT_FLAG = 4
_worst = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for variant in sorted(_worst):
        print("\n%s on a partition: largest error / bound over its cases: x %.3f, relative residual %.3f" % ((variant,) + tuple(_worst[variant])), end="")
    print()


def make_inverse(ctx, A_or_op, c):
    """test_gpu_iter_steps.py's object, for the rank's operator wrapper (or a matrix on one rank)"""
    import rails_amd

    inv = rails_amd.IterativeInverse(ctx, A_or_op, method=c.method, tol=0.0, maxit=1, jacobi=c.jacobi)
    if c.poly:
        A = c.matrix()
        inv.set("poly_ratio", S.POLY_RATIO)
        inv.set("eig_max", C.gershgorin(A, C.g_of(A, c.jacobi)))  # the restatement's own number
        inv.set("poly_fused", 1 if c.fused else 0)
        inv.set("poly_degree", c.poly)
    return inv


def solve_steps(ctx, inv, Bl, steps):
    """per step k: (x_k of these rows, iterations, relative residuals, flags, the object's counters, all-reduces the context counted)"""
    import rails_amd

    out = {}
    for k in steps:
        inv.set("max_iterations", k)
        n0 = ctx.stats()["allreduce"]
        X = inv.solve(rails_amd.HipMultiVectorWrapper(ctx, data=Bl)).to_host()
        it, rel, flags = inv.columns()
        out[k] = dict(X=X, it=it.copy(), rel=rel.copy(), flags=flags.copy(), stats=inv.stats(), ctx_allreduces=ctx.stats()["allreduce"] - n0)
    return out


def run_case(c, nranks):
    B = c.rhs()

    def work(r, ctx, op, plan, r0, r1):
        n0 = ctx.stats()["allreduce"]
        inv = make_inverse(ctx, op, c)
        created = ctx.stats()["allreduce"] - n0
        out = solve_steps(ctx, inv, B[r0:r1], c.steps)
        inv.close()
        return dict(steps=out, created=created, ghosts=plan.n_ghost)

    return PC.run_ranks(nranks, PC.csr_triple(c.matrix()), work)


@pytest.mark.parametrize("case_id,nranks", PC.STEP_PARAMS)
def test_steps_against_longdouble(case_id, nranks):
    c = PC.step_case(case_id)
    e = S.expected(c)
    res = run_case(c, nranks)
    groups = len(S.groups(c.w))
    per_iteration = 2 if c.method == "cg" else 3
    worst_x = worst_r = 0.0
    failures = []
    for r in range(nranks):
        assert res[r]["ghosts"] > 0 and res[r]["created"] == 1  # create's one all-reduce: the agreement
    for k in c.steps:
        X = np.vstack([res[r]["steps"][k]["X"] for r in range(nranks)])
        first = res[0]["steps"][k]
        for r in range(nranks):
            s = res[r]["steps"][k]
            assert np.all(s["it"] == k) and np.all(s["flags"] == MAXIT_FLAG), (case_id, k, r, s["it"], s["flags"])
            for name in ("it", "rel", "flags"):  # all-reduced sums: the same bits on every rank
                assert np.array_equal(s[name], first[name]), (case_id, k, r, name)
            st = s["stats"]
            assert st["allreduces"] == groups * (1 + per_iteration * k), (case_id, k, r, st)
            assert s["ctx_allreduces"] == st["allreduces"]
            if c.poly:
                assert st["poly_applications"] == (k + 1) * groups
                want = st["poly_applications"] * c.poly if c.fused else 0  # the ghost-row form really ran, each step behind its own exchange
                assert st["fused_launches"] == want and st["halo_exchanges"] == want, (case_id, k, r, st)
            else:
                assert st["halo_exchanges"] == 0 and st["fused_launches"] == 0
        rx, rr = e.ratios(k, X, first["rel"])
        worst_x, worst_r = max(worst_x, rx), max(worst_r, rr)
        if not (rx <= 1.0 and rr <= 1.0):
            failures.append((k, rx, rr))
    print("%s on %d ranks: largest error / bound: x %.3f, relative residual %.3f" % (case_id, nranks, worst_x, worst_r))
    w = _worst.setdefault(c.variant, [0.0, 0.0])
    w[0], w[1] = max(w[0], worst_x), max(w[1], worst_r)
    assert not failures, "%s on %d ranks: (step, x error / bound, residual error / bound) outside: %r" % (case_id, nranks, failures)


@pytest.mark.parametrize("case_id,nranks", [("cg-jacobi-m72-w17", 3), ("bicgstab-jacobi-m2181-w33", 2), ("cg-poly-fused-m72-w17", 2)])
def test_two_runs_give_the_same_bits(case_id, nranks):
    c = PC.step_case(case_id)
    a, b = run_case(c, nranks), run_case(c, nranks)
    for r in range(nranks):
        for k in c.steps:
            for name in ("X", "it", "rel", "flags"):
                assert np.array_equal(a[r]["steps"][k][name], b[r]["steps"][k][name]), (case_id, r, k, name)


def _one_rank(c, prepare):
    """the case on one context that `prepare` has made reduce (or not): its steps' results and counters"""
    import rails_amd

    ctx = rails_amd.Context(device=0, seed=3)
    try:
        prepare(ctx)
        inv = make_inverse(ctx, c.matrix(), c)
        out = solve_steps(ctx, inv, c.rhs(), c.steps)
        inv.close()
        return out
    finally:
        ctx.close()


def _same_bits_as_plain(c, prepare):
    plain = _one_rank(c, lambda ctx: None)
    split = _one_rank(c, prepare)
    groups = len(S.groups(c.w))
    for k in c.steps:
        p, s = plain[k], split[k]
        for name in ("X", "it", "rel", "flags"):
            assert np.array_equal(p[name], s[name]), (c.id, k, name)
        assert p["stats"]["allreduces"] == 0 and p["ctx_allreduces"] == 0
        want = groups * (1 + (2 if c.method == "cg" else 3) * k)
        assert s["stats"]["allreduces"] == want and s["ctx_allreduces"] == want
        assert s["stats"]["launches"] == p["stats"]["launches"] + want  # two launches where there was one, per scalar step


ONE_RANK_CASES = ["cg-jacobi-m72-w17", "bicgstab-jacobi-m72-w17", "cg-jacobi-m2181-w33", "bicgstab-jacobi-m2181-w33"]


@pytest.mark.parametrize("case_id", ONE_RANK_CASES)
def test_a_hook_that_changes_nothing_gives_the_bits_of_a_plain_context(case_id):
    _same_bits_as_plain(PC.step_case(case_id), lambda ctx: ctx.set_allreduce(lambda ptr, n, stream: 0))


@pytest.mark.parametrize("case_id", ONE_RANK_CASES)
def test_one_rank_rccl_communicator_gives_the_bits_of_a_plain_context(case_id):
    """the library's own communicator on a world of one (tests/test_gpu_hooks.py::test_native_rccl_single_rank): the all-reduce between
    the two scalar kernels is ncclAllReduce on the context's stream"""
    import rails_amd

    _same_bits_as_plain(PC.step_case(case_id), lambda ctx: ctx.init_rccl(rails_amd.Context.rccl_unique_id(), 1, 0))


_poly_expected = {}


def poly_expected(nc):
    """test_gpu_iter_poly.py::expected's rule for the 72-row matrix of the CG step cases, degree 2, ratio 30, Jacobi: the longdouble
    polynomial and per column 4 times the float64 restatement's error against it, at least 64 eps |y|_inf"""
    if nc not in _poly_expected:
        A = S.matrix("cg", 72)
        g = C.g_of(A, True)
        hi = C.gershgorin(A, g)
        Xm = R.rhs(72, nc, seed=9)
        Zl = C.polynomial(A, Xm, S.POLY_DEGREE, hi, S.POLY_RATIO, g, dtype=np.longdouble)
        Z64 = C.polynomial(A, Xm, S.POLY_DEGREE, hi, S.POLY_RATIO, g)
        bound = np.maximum(4 * np.abs(Z64 - Zl).max(0), 64 * S.EPS * np.abs(Zl).max(0)).astype(float)
        _poly_expected[nc] = (A, Xm, Zl, bound, hi)
    return _poly_expected[nc]


@pytest.mark.parametrize("nc", (3, 32))
@pytest.mark.parametrize("fused", (1, 0))
def test_precondition_on_two_ranks(fused, nc):
    """the polynomial on its own, through the ghost-row fused step and through rails_spmm and one pass; the interval's upper end is the
    bound the ranks agreed on at create"""
    import rails_amd

    A, Xm, Zl, bound, hi = poly_expected(nc)

    def work(r, ctx, op, plan, r0, r1):
        inv = rails_amd.IterativeInverse(ctx, op, method="cg", poly_degree=S.POLY_DEGREE, poly_ratio=S.POLY_RATIO)
        inv.set("poly_fused", fused)
        n0 = ctx.stats()["allreduce"]
        Z = inv.precondition(rails_amd.HipMultiVectorWrapper(ctx, data=Xm[r0:r1])).to_host()
        out = dict(Z=Z, stats=inv.stats(), allreduces=ctx.stats()["allreduce"] - n0)
        inv.close()
        return out

    res = PC.run_ranks(2, PC.csr_triple(A), work)
    Z = np.vstack([res[r]["Z"] for r in range(2)])
    for r in range(2):
        st = res[r]["stats"]
        assert st["poly_applications"] == 1 and st["products"] == S.POLY_DEGREE and res[r]["allreduces"] == 0 and st["allreduces"] == 0
        assert st["fused_launches"] == (S.POLY_DEGREE if fused else 0) and st["halo_exchanges"] == st["fused_launches"]
        assert st["eig_hi"] == res[0]["stats"]["eig_hi"] and abs(st["eig_hi"] - hi) <= 4 * S.EPS * hi
    err = np.abs(Z - Zl).astype(float)
    print("precondition on 2 ranks, %d columns, fused %d: largest error / allowed error %.3f" % (nc, fused, (err.max(0) / bound).max()))
    assert np.all(err <= bound[None, :]), (nc, fused, (err.max(0) / bound).max())
