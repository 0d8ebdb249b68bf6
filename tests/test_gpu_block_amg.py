"""The block multigrid preconditioner of the iterative A^-1 operator (include/rails_hip.h: "block_amg", rails_iter_block_amg_setup,
rails_iter_block_amg_info; rails_amd/csrc/block_amg_host.cpp and iter_hierarchy.hip for the set-up, itsolve.hip: Run::vcycle on block sweeps, iter_kernels.inc:
k_cheb_step_bsr, k_amg_residual_bsr, k_cheb_init_bj, k_cheb_pass_bj on bsr_row_gather.inc and iter_pass_block) on the GPU against the
restatement of tests/block_amg_reference.py: one cycle against a longdouble evaluation on the shapes at which the kernels take their
different paths, the fused step against the unfused one bit for bit, converged solves against the restatement's iteration counts and
against block Jacobi, "block_amg" 0 bit for bit, determinism, the counts per cycle of DESIGN.md section 16, the refusals, and one
Lyapunov solve.  Three larger problems put the fine level's fused step and residual at 2 and 4 block rows per lane group
(tests/bsr_reference.py::shape_for; tests/test_gpu_bsr_rounds.py has the product itself there)."""
import numpy as np
import pytest

import block_amg_reference as B
import block_jacobi_reference as BJ
import bsr_reference as K
import iter_reference as R

pytestmark = pytest.mark.gpu

TOL = 1e-8
EPS = np.finfo(float).eps
WIDTHS = (1, 2, 3, 16, 17, 33)  # 8 lanes per block row up to 16 columns, 16 above; odd last columns and the pad column; a group of 32 and a tail
DEGREES = (0, 1, 2)             # no smoother step beyond the first, and both parities of the fused step's ping-pong
PANEL, XC0, YC0 = 120, 37, 71   # windows at odd columns of panels 120 columns wide
SENTINEL = 7.25
# one block row (no level, the dense inverse alone) at every b; 48 cells with two matrices at every b (fewer block rows than a workgroup's
# lane groups on both); 216 and 100 cells; 512 cells with three matrices; a positive definite operator; a block row of 72 blocks at b = 8,
# longer than the 64 blocks of the LDS buffer
ONES = ["one%d" % b for b in B.J.BS]
SMALL = ["d4x4x3b%dc%d" % (b, 8 * b) for b in B.J.BS]
PROBLEMS = ONES + SMALL + ["d6x6x6b3", "d5x5x4b6", "d8x8x8b4", "d4x4x3b3c24p", "long8"]
# Fine levels with enough block rows for more than one round of the shared block-row body, at one degree: {width: block rows per lane group}
# of k_cheb_step_bsr / k_amg_residual_bsr<b, 8 lanes up to 16 columns, 16 above>.  The names are the grids for 256 compute units (32768,
# 16900 and 4096 cells; at b = 8 a workgroup is one wave of four lane groups); on another device rounds_problem sizes the grid instead.
ROUNDS = {"d32x32x32b2": {16: 2, 15: 2, 17: 4, 32: 4}, "d26x26x25b3": {17: 2}, "d16x16x16b8": {17: 2, 32: 2}}
ROUNDS_DEGREES = (1,)


@pytest.fixture(scope="module")
def ctx():
    import rails_amd

    c = rails_amd.Context(device=0, seed=3)
    yield c
    c.close()


_inverses = {}
_operators = {}


def operator(ctx, tag):
    import rails_amd

    ip, ix, dt = B.problem(tag)[0]
    return rails_amd.HipOperatorWrapper.from_bsr(ctx, np.asarray(ip, dtype=np.int64), np.asarray(ix, dtype=np.int32), np.ascontiguousarray(dt))


def inverse(ctx, tag):
    """one IterativeInverse (CG) on the block-CSR handle per problem, shared by the tests of this module, with every setting at a known
    value and "block_amg" on"""
    import rails_amd

    if tag not in _inverses:
        _operators[tag] = operator(ctx, tag)
        _inverses[tag] = rails_amd.IterativeInverse(ctx, _operators[tag], method="cg", tol=TOL)
    inv = _inverses[tag]
    for name, value in (("tolerance", TOL), ("jacobi", 1), ("max_iterations", 1000), ("strict", 0), ("check_every", 8), ("poly_degree", 0), ("block_jacobi", 0),
                        ("poly_fused", 1), ("amg_degree", B.DEGREE), ("amg_ratio", B.RATIO), ("amg_theta", B.THETA), ("amg_coarse", B.problem(tag)[1]),
                        ("block_amg", 1)):
        inv.set(name, value)
    return inv


@pytest.fixture(scope="module", autouse=True)
def _close_inverses(ctx):
    yield
    for inv in _inverses.values():
        inv.close()
    _inverses.clear()
    _operators.clear()


def window(mv, c0, nc):
    return mv.view(c0, c0 + nc - 1) if nc > 1 else mv.view(c0)


def levels_of(tag):
    return len(B.hierarchy(tag)[1]["levels"])


def cycle_counts(tag, S):
    """DESIGN.md section 16, per cycle and multigrid level: 2 S + 4 kernels of the object (the first smoother step from zero, S steps, the
    residual, the prolongation, 1 + S steps) and 2 S + 4 products (2 S + 2 with A_l, one with P', one with P), plus the dense kernel:
    (launches, products, fused steps)"""
    L = levels_of(tag)
    return L * (2 * S + 4) + 1, L * (2 * S + 4), L * (2 * S + 1)


def block_size(tag):
    return B.hierarchy(tag)[1]["b"]


def rounds_problem(tag, num_cu):
    """the problem of ROUNDS[tag] for a device of num_cu compute units: the named grid where its cell count gives every width its rounds
    (256 compute units), else the most cubic grid nx = ny >= nz that does"""
    b = int(tag.split("b")[1])
    lo = max(K.shape_for(b, K.lanes(nc), rpg, num_cu)[0] for nc, rpg in ROUNDS[tag].items())
    hi = min(K.shape_for(b, K.lanes(nc), 2 * rpg, num_cu)[0] for nc, rpg in ROUNDS[tag].items() if rpg < 4)
    nx, ny, nz = (int(v) for v in tag[1:].split("b")[0].split("x"))
    if not lo <= nx * ny * nz < hi:
        nx = ny = int(np.ceil(lo ** (1.0 / 3.0)))
        nz = -(-lo // (nx * ny))
    assert lo <= nx * ny * nz < hi, (tag, num_cu, lo, hi)
    return "d%dx%dx%db%d" % (nx, ny, nz, b)


def rule_fuses(tag, nc, ld=34):
    """block_amg_choice.h through its restatement: whether every level of the problem takes the fused step at this width"""
    h = B.hierarchy(tag)[1]
    out = []
    for lv in h["levels"]:
        ip = lv["bsr"][0]
        out.append(B.step_choice(h["b"], nc, len(ip) - 1, int(np.diff(ip).max()), ld, True)[1])
    return all(out)


def test_block_amg_is_a_setting(ctx):
    """(without the feature: RAILS_EINVAL, "no setting named")"""
    import rails_amd

    lib = ctx.lib
    assert hasattr(lib, "rails_iter_block_amg_setup") and hasattr(lib, "rails_iter_block_amg_info")
    inv = inverse(ctx, "d4x4x3b3c24")
    inv.set("block_amg", 1)
    A = B.hierarchy("d4x4x3b3c24")[0]
    Bm = R.rhs(144, 2)
    assert R.true_relres(A, inv.solve_host(Bm), Bm).max() <= 10 * TOL
    info = inv.block_amg_info()
    assert info["levels"] == 2 and info["rows"] == [144, 24] and info["cycles"] > 0
    assert inv.amg_info()["levels"] == 0  # (the scalar hierarchy's info does not speak for the block one)
    assert np.all(inv.columns()[2] == 2)
    with pytest.raises(rails_amd.RailsError, match="block_amg"):
        inv.set("no_such_setting", 1)


def test_info_is_the_restatements_hierarchy(ctx):
    for tag in PROBLEMS:
        inv = inverse(ctx, tag)
        info = inv.block_amg_setup()
        A, h = B.hierarchy(tag)
        assert info["levels"] == len(h["levels"]) + 1 and info["rows"] == B.rows_of(h), (tag, info)
        assert info["nnz"] == B.nnz_of(h)
        for got, lv in zip(info["hi"], h["levels"]):
            assert abs(got - lv["hi"]) <= 1e-9 * lv["hi"]
        assert info["hi"][-1] == 0.0 and abs(info["operator_complexity"] - B.operator_complexity(h)) <= 1e-12
        assert all(r % h["b"] == 0 for r in info["rows"])


_longdouble = {}


def expected(tag, S):
    """the longdouble evaluation of one cycle on a shared input of the widest width (columns are independent: narrower widths take its
    first columns) and the allowed error per column (block_amg_reference.cycle_reference)"""
    if (tag, S) not in _longdouble:
        A, h = B.hierarchy(tag)
        Xm = R.rhs(A.shape[0], max(WIDTHS), seed=9)
        Zl, bound = B.cycle_reference(h, Xm, S)
        _longdouble[(tag, S)] = (Xm, Zl, bound)
    return _longdouble[(tag, S)]


def precondition_both_ways(ctx, inv, Xm):
    """on full panels and on windows at odd columns (NaN beside X, sentinels beside Y); returns the two results"""
    import rails_amd

    n, nc = Xm.shape
    X = rails_amd.HipMultiVectorWrapper(ctx, data=Xm)
    full = inv.precondition(X).to_host()
    assert np.array_equal(X.to_host(), Xm)
    big = np.full((n, PANEL), np.nan)
    big[:, XC0:XC0 + nc] = Xm
    Xp = rails_amd.HipMultiVectorWrapper(ctx, data=big)
    Yp = rails_amd.HipMultiVectorWrapper(ctx, data=np.full((n, PANEL), SENTINEL))
    inv.precondition(window(Xp, XC0, nc), window(Yp, YC0, nc))
    assert np.array_equal(Xp.to_host(), big, equal_nan=True)
    Yh = Yp.to_host()
    assert np.all(Yh[:, :YC0] == SENTINEL) and np.all(Yh[:, YC0 + nc:] == SENTINEL)
    return full, Yh[:, YC0:YC0 + nc].copy()


@pytest.mark.parametrize("tag", PROBLEMS + list(ROUNDS))
def test_one_cycle_against_longdouble_fused_and_unfused(ctx, tag):
    """items 2, 3 and 7: the cycle within the restatement's bound at every degree and width, through full panels and windows bit for
    bit; the fused and the unfused step give the same bits; launches and products per cycle and level are section 16's.  The problems
    of ROUNDS at their own widths and one degree: the fine level's launch has the block rows per lane group named there, by the restated
    rule at the context's compute units and by what the handle reports of the unfused step's product, the same launch."""
    degrees, widths, rounds = DEGREES, WIDTHS, ROUNDS.get(tag)
    if rounds:
        num_cu = ctx.lib.rails_ctx_num_cu(ctx.h)
        tag, degrees, widths = rounds_problem(tag, num_cu), ROUNDS_DEGREES, tuple(rounds)
        fine = B.hierarchy(tag)[1]["levels"][0]["bsr"][0]
        fine_mb, fine_longest = len(fine) - 1, int(np.diff(fine).max())
        for nc in widths:
            assert K.predicted_stats(block_size(tag), nc, fine_mb, fine_longest, num_cu)["rpg"] == rounds[nc], (tag, nc, num_cu)
    inv = inverse(ctx, tag)
    worst = 0.0
    for S in degrees:
        Xall, Zall, ball = expected(tag, S)
        inv.set("amg_degree", S)
        launches, products, fused_steps = cycle_counts(tag, S)
        for nc in widths:
            Xm, Zl, bound = np.ascontiguousarray(Xall[:, :nc]), Zall[:, :nc], ball[:nc]
            groups = (nc + 31) // 32
            got = {}
            for fused in (1, 0):
                inv.set("poly_fused", fused)
                full, win = precondition_both_ways(ctx, inv, Xm)
                info, st = inv.block_amg_info(), inv.stats()
                assert info["cycles"] == groups and info["cycle_launches"] == groups * launches and info["cycle_products"] == groups * products, (info, S, nc)
                assert st["launches"] == groups * launches and st["products"] == groups * products
                # the rule sends no block size to the unfused step by itself (no instantiation spills); what it decides shows here
                takes_fused = fused and all(rule_fuses(tag, min(32, nc - 32 * g)) for g in range(groups))
                assert st["fused_launches"] == (groups * fused_steps if takes_fused else 0), (st, S, nc, fused)
                assert np.array_equal(full, win)  # the same bits through a window
                err = np.abs(full - Zl).astype(float)
                worst = max(worst, (err.max(0) / bound).max())
                assert np.all(err <= bound[None, :]), (tag, nc, S, fused, (err.max(0) / bound).max())
                got[fused] = full
                if rounds and not fused:  # the last product on the handle: the fine level's, in the second sweep
                    st, want = _operators[tag].bsr_stats(), K.predicted_stats(block_size(tag), nc, fine_mb, fine_longest, num_cu)
                    assert {k: st[k] for k in want} == want and st["rpg"] == rounds[nc], (st, want)
                    print("problem %s, %d columns: the fine level's product reports rpg %d, all_staged %s" % (tag, nc, st["rpg"], st["all_staged"]))
            assert np.array_equal(got[1], got[0]), (tag, nc, S)  # the product is the row-gather order either way, the epilogue one function
    Xm, Zl, _ = expected(tag, 1)
    assert np.all(np.sign((Xm * Zl).sum(0)) == B.hierarchy(tag)[1]["defsign"])  # the cycle has the operator's own sign
    print("problem %s, rows %s: largest error / allowed error %.3f" % (tag, B.rows_of(B.hierarchy(tag)[1]), worst))


_solves = {}


def reference_solve(tag, nc):
    """the restatement's solves with the cycle and with block Jacobi on iter_reference's shared right-hand side, computed once"""
    if (tag, nc) not in _solves:
        A, h = B.hierarchy(tag)
        Bm = R.rhs(A.shape[0], nc)
        X, c = B.pcg(A, Bm, lambda r: B.vcycle(h, r), tol=TOL)
        G = B.block_jacobi_of(B.problem(tag)[0])
        _, cj = B.pcg(A, Bm, lambda r: BJ.apply_blocks(G, r), tol=TOL)
        _solves[(tag, nc)] = (A, Bm, c, cj)
    return _solves[(tag, nc)]


@pytest.mark.parametrize("tag,nc", [(t, n) for t in ("d6x6x6b3", "d8x8x8b3", "d12x12x12b3", "d8x8x8b4") for n in (3, 17)])
def test_converged_solves(ctx, tag, nc):
    """block_diffusion7(n, n, n, b, spread 100, reaction 0.01) to 1e-8: the true residual within 10 times the tolerance, the iteration
    count within 1.5 times the float64 restatement's, and block Jacobi on the device needs at least twice the cycle's count.  The
    restatement's own counts, cycle / block Jacobi, checked on the CPU before any device run (3 and 17 columns alike up to one):
    6^3 x 3: 6 / 31..34; 8^3 x 3: 7 / 42..45; 12^3 x 3: 7 / 61..63; 8^3 x 4: 7 / 43..45."""
    import rails_amd

    A, Bm, cr, cj = reference_solve(tag, nc)
    assert np.all(cr.flags == R.CONVERGED) and np.all(cj.flags == R.CONVERGED) and np.all(cj.iter >= 2 * cr.iter.max())
    inv = inverse(ctx, tag)
    big = np.full((A.shape[0], PANEL), np.nan)
    big[:, XC0:XC0 + nc] = Bm
    Xp = rails_amd.HipMultiVectorWrapper(ctx, data=big)
    Yp = rails_amd.HipMultiVectorWrapper(ctx, data=np.full((A.shape[0], PANEL), SENTINEL))
    inv.solve(window(Xp, XC0, nc), window(Yp, YC0, nc))
    Yh = Yp.to_host()
    assert np.all(Yh[:, :YC0] == SENTINEL) and np.all(Yh[:, YC0 + nc:] == SENTINEL)
    Xg = Yh[:, YC0:YC0 + nc]
    it, rel, flags = inv.columns()
    it = it.copy()
    assert np.all(np.isfinite(Xg)) and np.all(flags == 2), flags
    assert R.true_relres(A, Xg, Bm).max() <= 10 * TOL
    assert np.all(it <= 1.5 * cr.iter), (it, cr.iter)
    inv.set("block_amg", 0)
    inv.block_jacobi()
    Xj = inv.solve_host(Bm)
    itj = inv.columns()[0].copy()
    assert R.true_relres(A, Xj, Bm).max() <= 10 * TOL
    inv.set("block_jacobi", 0)
    print("problem %s, %d columns: cycle %d..%d (restatement %d..%d), block Jacobi %d..%d (restatement %d..%d)" % (
        tag, nc, it.min(), it.max(), cr.iter.min(), cr.iter.max(), itj.min(), itj.max(), cj.iter.min(), cj.iter.max()))
    assert np.all(itj >= 2 * it.max()), (itj, it)


def test_switching_back(ctx):
    """"block_amg" 0 after 1 and a solve: the bits, launches and products of an object that never had it; block Jacobi installed
    afterwards works as before"""
    import rails_amd

    tag = "d6x6x6b3"
    A = B.hierarchy(tag)[0]
    Bm = R.rhs(A.shape[0], 5)
    diag = A.diagonal()
    fresh = rails_amd.IterativeInverse(ctx, operator(ctx, tag), method="cg", tol=TOL, diag=diag)
    X0 = fresh.solve_host(Bm)
    st0 = fresh.stats()
    used = rails_amd.IterativeInverse(ctx, operator(ctx, tag), method="cg", tol=TOL, diag=diag, block_amg=True)
    used.solve_host(Bm)
    assert used.block_amg_info()["cycles"] > 0
    used.set("block_amg", 0)
    X1 = used.solve_host(Bm)
    st1 = used.stats()
    assert np.array_equal(X0, X1)
    assert st0["launches"] == st1["launches"] and st0["products"] == st1["products"] and st1["poly_applications"] == 0 and st1["fused_launches"] == 0
    assert used.block_amg_info()["cycles"] == 0
    fresh.block_jacobi()
    used.block_jacobi()
    assert np.array_equal(fresh.solve_host(Bm), used.solve_host(Bm))
    assert fresh.stats()["launches"] == used.stats()["launches"] and np.array_equal(fresh.columns()[0], used.columns()[0])
    fresh.close()
    used.close()


def test_determinism_and_columns_of_different_speed(ctx):
    """the same bits at check_every 1 and 8; a zero column and columns of different speed; max_iterations flags a column"""
    tag = "d8x8x8b4"
    A, h = B.hierarchy(tag)
    inv = inverse(ctx, tag)
    Bm = R.rhs(A.shape[0], 6)
    Bm[:, 1] = 0.0
    Bm[:, 2] = 0.0
    Bm[5, 2] = 1.0               # one unknown: an iteration fewer in the restatement (the cycle leaves little room for more)
    Bm[:, 3] = 1e-3 * Bm[:, 4]  # another scale
    _, cr = B.pcg(A, Bm, lambda r: B.vcycle(h, r), tol=TOL)
    assert len(set(cr.iter.tolist())) >= 3, cr.iter
    out = {}
    for every in (1, 8, 8):
        inv.set("check_every", every)
        X = inv.solve_host(Bm)
        it, rel, fl = inv.columns()
        out.setdefault(every, []).append((X, it.copy(), fl.copy()))
    X1, it1, fl1 = out[1][0]
    for X, it, fl in out[8]:
        assert np.array_equal(X, X1) and np.array_equal(it, it1) and np.array_equal(fl, fl1)
    assert it1[1] == 0 and np.all(X1[:, 1] == 0.0) and np.all(fl1 == 2)
    assert len(set(it1.tolist())) >= 3, it1
    assert R.true_relres(A, np.delete(X1, 1, 1), np.delete(Bm, 1, 1)).max() <= 10 * TOL
    inv.set("max_iterations", 2)
    inv.solve_host(Bm)
    it, rel, fl = inv.columns()
    assert fl[0] == 4 and it[0] == 2 and fl[1] == 2
    inv.set("max_iterations", 1000)


def test_refusals(ctx):
    """every refusal of include/rails_hip.h, in either order of setting; the object still solves afterwards"""
    import rails_amd

    tag = "d4x4x3b3c24"
    ip, ix, dt = (np.asarray(t) for t in B.problem(tag)[0])
    A = B.hierarchy(tag)[0]
    Bm = R.rhs(A.shape[0], 2)
    op = operator(ctx, tag)

    def refused(call, text):
        with pytest.raises(rails_amd.RailsError, match=text):
            call()

    bi = rails_amd.IterativeInverse(ctx, op, method="bicgstab", tol=TOL)
    refused(lambda: bi.set("block_amg", 1), "BiCGStab")
    refused(lambda: bi.block_amg_setup(), "BiCGStab")
    refused(lambda: bi.set("amg", 1), "BiCGStab")
    assert R.true_relres(A, bi.solve_host(Bm), Bm).max() <= 10 * TOL
    bi.close()
    # not a block-CSR handle
    csr = rails_amd.IterativeInverse(ctx, sp_csr(A), method="cg", tol=TOL)
    refused(lambda: csr.set("block_amg", 1), "not a block-CSR handle")
    refused(lambda: csr.block_amg_setup(), "not a block-CSR handle")
    assert R.true_relres(A, csr.solve_host(Bm), Bm).max() <= 10 * TOL
    csr.close()
    inv = rails_amd.IterativeInverse(ctx, op, method="cg", tol=TOL, amg_coarse=24)
    # what existing tests pin stays: "amg" on a block-CSR handle, "poly_degree" without a bound
    refused(lambda: inv.set("amg", 1), "scalar CSR arrays")
    # one preconditioner at a time, in either order
    inv.set("block_amg", 1)
    refused(lambda: inv.block_jacobi(), "one preconditioner at a time")
    refused(lambda: inv.set("poly_degree", 2), "one preconditioner at a time")
    refused(lambda: inv.set("amg", 1), "one preconditioner at a time")
    inv.set("block_amg", 0)
    inv.block_jacobi()
    refused(lambda: inv.set("block_amg", 1), "one preconditioner at a time")
    refused(lambda: inv.block_amg_setup(), "one preconditioner at a time")
    inv.set("block_jacobi", 0)
    inv.set("eig_max", 300.0)
    inv.set("poly_degree", 2)
    refused(lambda: inv.set("block_amg", 1), "one preconditioner at a time")
    inv.set("poly_degree", 0)
    inv.set("block_amg", 1)
    assert R.true_relres(A, inv.solve_host(Bm), Bm).max() <= 10 * TOL and inv.block_amg_info()["levels"] == 2
    inv.close()

    # refusals of the set-up, each on an operator of its own; "block_amg" itself is accepted (the entries are looked at by the set-up),
    # the solve and the set-up refuse, and with the setting off again the object solves
    def setup_refuses(triple, text, solves=True):
        bad = rails_amd.HipOperatorWrapper.from_bsr(ctx, np.asarray(triple[0], dtype=np.int64), np.asarray(triple[1], dtype=np.int32), np.ascontiguousarray(triple[2]))
        obj = rails_amd.IterativeInverse(ctx, bad, method="cg", tol=TOL, amg_coarse=24, block_amg=True)
        rhs = R.rhs((len(triple[0]) - 1) * triple[2].shape[1], 2)
        refused(lambda: obj.block_amg_setup(), text)
        refused(lambda: obj.solve_host(rhs), text)
        assert obj.block_amg_info()["levels"] == 0
        obj.set("block_amg", 0)
        if solves:
            obj.set("max_iterations", 3)
            assert np.all(np.isfinite(obj.solve_host(rhs)))
        obj.close()

    keep = np.ones(len(ix), dtype=bool)
    keep[np.flatnonzero((ix == 5) & (np.repeat(np.arange(len(ip) - 1), np.diff(ip)) == 5))] = False
    ip2 = np.concatenate([[0], np.cumsum(np.add.reduceat(keep.astype(np.int64), ip[:-1]))])
    setup_refuses((ip2, ix[keep], dt[keep]), "no stored diagonal block")
    swapped_ix, swapped_dt = ix.copy(), dt.copy()
    swapped_ix[[ip[7], ip[7] + 1]] = swapped_ix[[ip[7] + 1, ip[7]]]
    swapped_dt[[ip[7], ip[7] + 1]] = swapped_dt[[ip[7] + 1, ip[7]]]
    setup_refuses((ip, swapped_ix, swapped_dt), "not strictly increasing")
    nonfinite = dt.copy()
    nonfinite[11, 1, 2] = np.nan
    setup_refuses((ip, ix, nonfinite), "not finite", solves=False)
    centre = np.flatnonzero(ix == np.repeat(np.arange(len(ip) - 1), np.diff(ip)))
    mixed = dt.copy()
    mixed[centre[3], 0, 0] *= -1.0
    setup_refuses((ip, ix, mixed), "both signs")
    zero = dt.copy()
    zero[centre[3], 1, 1] = 0.0
    setup_refuses((ip, ix, zero), "zero or not finite")
    differ = dt.copy()
    differ[centre[3]] *= -1.0
    setup_refuses((ip, ix, differ), "both signs")
    singular = dt.copy()
    singular[centre[3]] = -np.ones((3, 3)) - 1e-300 * np.eye(3)
    setup_refuses((ip, ix, singular), "diagonal block 3")
    eye = np.arange(600)
    setup_refuses((np.arange(601), eye, np.tile(np.eye(2), (600, 1, 1)) * (1.0 + eye % 5)[:, None, None]), "does not coarsen", solves=False)
    setup_refuses((np.array([0, 1]), np.array([0]), np.array([[[1.0, 3.0], [3.0, 1.0]]])), "not definite", solves=False)


def test_refusal_of_more_rows_than_the_cycle_addresses(ctx):
    """2^24 rows (2^23 diagonal blocks of 2): refused by the setting and by the set-up before anything is built, and the object solves"""
    import rails_amd

    mb = 1 << 23
    data = np.tile(np.array([[2.0, 0.5], [0.5, 1.0]]), (mb, 1, 1))
    op = rails_amd.HipOperatorWrapper.from_bsr(ctx, np.arange(mb + 1, dtype=np.int64), np.arange(mb, dtype=np.int32), data)
    inv = rails_amd.IterativeInverse(ctx, op, method="cg", tol=TOL)
    for call in (lambda: inv.set("block_amg", 1), lambda: inv.block_amg_setup()):
        with pytest.raises(rails_amd.RailsError, match="fewer than 2\\^24 rows"):
            call()
    X = rails_amd.HipMultiVectorWrapper(ctx, data=np.ones((2 * mb, 1)))
    Y = inv.solve(X).to_host()
    assert np.all(inv.columns()[2] == 2) and abs(Y[0, 0] - 2.0 / 7.0) <= 1e-8 and abs(Y[1, 0] - 6.0 / 7.0) <= 1e-8
    inv.close()


def sp_csr(A):
    import scipy.sparse as sp

    return sp.csr_matrix(A)


def test_lyapunov_solve_with_the_inverse_krylov_projection(ctx):
    """"Projection method" 1.1 on block_diffusion7(6, 6, 6, 4), B of 4 columns, the inverse an IterativeInverse on the block-CSR handle:
    with block Jacobi and with the block multigrid cycle the solve converges by the solver's own test, and the cycle needs fewer inner
    iterations"""
    import rails_amd
    from rails_amd import problems as P

    tag = "d6x6x6b4"
    A = B.hierarchy(tag)[0]
    Bm = P.rhs(A.shape[0], 4, seed=2)
    params = {"Restart size": 80, "Reduced size": 40, "Expand size": 4, "Lanczos iterations": 8, "Tolerance": 1e-6, "Projection method": 1.1}
    op = operator(ctx, tag)

    def solve_with(inverse):
        s = rails_amd.Solver(ctx, op, Bm)
        assert s.set_parameters(params) == 0
        s.set_option("verbose", 0)
        s.set_inverse(inverse)
        code, V, T = s.solve()
        out = (code, s.relative_residual(), s.trips())
        s.close()
        return out

    def run(inverse):
        # In a thread of its own: the projected Lyapunov solve keeps what it learned per thread from call to call (DESIGN.md section 18,
        # the end of its contracts), so both solves start alike and the main thread stays as the rest of the suite expects it.
        import threading

        box = {}

        def work():
            try:
                box["out"] = solve_with(inverse)
            except BaseException as e:  # handed to the main thread below
                box["error"] = e

        t = threading.Thread(target=work)
        t.start()
        t.join()
        if "error" in box:
            raise box["error"]
        return box["out"]

    block = rails_amd.IterativeInverse(ctx, op, method="cg", tol=TOL, block_jacobi=True)
    code_b, rel_b, trips_b = run(block)
    total_b = block.stats()["total_iterations"]
    assert block.stats()["total_flagged_columns"] == 0
    block.close()
    mg = rails_amd.IterativeInverse(ctx, op, method="cg", tol=TOL, block_amg=True)
    code_m, rel_m, trips_m = run(mg)
    total_m = mg.stats()["total_iterations"]
    assert mg.stats()["total_flagged_columns"] == 0
    mg.close()
    print("block Jacobi: code %d, %d trips, relative residual %.2e, %d inner iterations; block multigrid: code %d, %d trips, %.2e, %d" % (
        code_b, trips_b, rel_b, total_b, code_m, trips_m, rel_m, total_m))
    assert code_b == 0 and code_m == 0
    assert 0 < total_m < total_b
