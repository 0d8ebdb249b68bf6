"""Bits and counters of the iterative A^-1 operator (rails_amd/csrc/itsolve.hip, iter_setup.hip, iter_hierarchy.hip) over a fixed list of cases, to compare two builds of the
library: a refactoring of the host code must leave every result, every column's iterations, flags and residual and every counter as they
were.

    python scripts/iter_identity.py --tree PATH --out ONE.json      # imports rails_amd from PATH in a fresh child process, runs the cases
    python scripts/iter_identity.py --compare PARENT.json NEW.json --out profiles/iter_refactor_identity.json

The cases come from the fixtures of the tests (tests/iter_reference.py, cheb_reference.py, amg_reference.py, block_jacobi_reference.py, block_amg_reference.py,
iter_partition_cases.py):
solve and precondition at widths 1, 3, 16, 17, 32 and 33 (the pad column, the 8-lane against the 16-lane gather, the group loop); CG with
and without Jacobi and on a negative definite matrix, BiCGStab with and without Jacobi and transposed; the polynomial at degrees 1, 2 and 5
fused and unfused; the multigrid cycle on five problems at smoother degrees 0, 1 and 2 fused and unfused; block Jacobi under CG and BiCGStab (plain
and transposed) with the blocks taken from a CSR operator, from a block-CSR operator and passed in; the block multigrid cycle on six problems
at smoother degrees 0, 1 and 2 fused and unfused; check_every 8 and 1 at every width; the two-rank polynomial cases (the ghost-row form of the fused step) at degrees 1 and 4, ranks as threads on one device.
A case is one setting of the object and one call, solve or precondition, run at every width (two-rank cases: on both ranks), so that
the file stays small.  Per case: the SHA-256 of the results' bytes in the order they were computed, the SHA-256 of the columns'
iterations, flags and relative residuals after each call, and the counters launches, products, inner products, polynomial applications,
fused launches, all-reduces, own halo exchanges, cycles, cycle launches, cycle products, summed over the calls of the case."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (1, 3, 16, 17, 32, 33)
COUNTERS = ("launches", "products", "inner_products", "poly_applications", "fused_launches", "allreduces", "halo_exchanges")
CYCLE_COUNTERS = ("cycles", "cycle_launches", "cycle_products")


class Record:
    """what a case holds, gathered over its calls"""

    def __init__(self):
        self.result, self.columns, self.counters = hashlib.sha256(), hashlib.sha256(), [0] * len(COUNTERS + CYCLE_COUNTERS)

    def add(self, inv, Y):
        import numpy as np

        it, rel, flags = inv.columns()
        st, amg, bamg = inv.stats(), inv.amg_info(), inv.block_amg_info()  # (a hierarchy is of one kind: the other's counters read 0)
        self.result.update(np.ascontiguousarray(Y.to_host()).tobytes())
        for a in (it, flags, rel):
            self.columns.update(np.ascontiguousarray(a).tobytes())
        self.counters = [c + v for c, v in zip(self.counters, [st[n] for n in COUNTERS] + [amg[n] + bamg[n] for n in CYCLE_COUNTERS])]

    def merge(self, other):
        """another rank's record, behind this one"""
        self.result.update(other.result.digest())
        self.columns.update(other.columns.digest())
        self.counters = [c + v for c, v in zip(self.counters, other.counters)]

    def json(self):
        return {"result": self.result.hexdigest(), "columns": self.columns.hexdigest(), "counters": self.counters}


def both_calls(rails_amd, ctx, inv, B, out, key, trans=False):
    """solve (check_every 8 and 1) and precondition of the first w columns of B, for every width"""
    solve, pre = Record(), Record()
    for w in WIDTHS:
        X = rails_amd.HipMultiVectorWrapper(ctx, data=B[:, :w])
        for every in (8, 1):
            inv.set("check_every", every)
            solve.add(inv, inv.solve(X, trans=trans))
        pre.add(inv, inv.precondition(X))
    out[key + " solve"], out[key + " precondition"] = solve.json(), pre.json()


def single_gpu(rails_amd, ctx, out):
    import amg_reference as AM
    import cheb_reference as C
    import iter_reference as R

    # CG with Jacobi, without, and on a negative definite matrix (the 7-point Laplacian); BiCGStab with Jacobi, without, transposed
    for tag, jacobi, trans in (("a", True, False), ("a", False, False), ("d", False, False), ("c", True, False), ("c", False, False), ("c", True, True)):
        A, method = R.problem(tag)
        inv = rails_amd.IterativeInverse(ctx, A, method=method, tol=1e-10, maxit=5000, jacobi=jacobi)
        both_calls(rails_amd, ctx, inv, R.rhs(A.shape[0], max(WIDTHS)), out, "%s %s jacobi%d trans%d" % (method, tag, jacobi, trans), trans=trans)
        inv.close()
    # the polynomial: odd and even degrees start in different panels
    A = C.problem("lap64")
    B = R.rhs(A.shape[0], max(WIDTHS))
    inv = rails_amd.IterativeInverse(ctx, A, method="cg", tol=1e-10, maxit=5000)
    for jacobi in (1, 0):
        for K in (1, 2, 5):
            for fused in (1, 0):
                for name, value in (("jacobi", jacobi), ("poly_degree", K), ("poly_fused", fused)):
                    inv.set(name, value)
                both_calls(rails_amd, ctx, inv, B, out, "poly lap64 jacobi%d K%d fused%d" % (jacobi, K, fused))
    inv.close()
    # the multigrid cycle: several levels in 2D and 3D, a negative definite banded matrix with long rows of P, two one-block hierarchies
    for tag in ("lap24", "lap7_12", "neg_banded41", "stencil27", "one"):
        A, coarse = AM.problem(tag)
        B = R.rhs(A.shape[0], max(WIDTHS))
        inv = rails_amd.IterativeInverse(ctx, A, method="cg", tol=1e-10, maxit=5000, amg=True, amg_coarse=coarse)
        for S in (0, 1, 2):
            for fused in (1, 0):
                inv.set("amg_degree", S)
                inv.set("poly_fused", fused)
                both_calls(rails_amd, ctx, inv, B, out, "amg %s S%d fused%d" % (tag, S, fused))
        inv.close()
    block_jacobi(rails_amd, ctx, out)
    block_cycle(rails_amd, ctx, out)


def block_jacobi(rails_amd, ctx, out):
    """block Jacobi: CG, BiCGStab plain and transposed; the blocks of a CSR operator by block_size, a block-CSR operator's own, blocks
    passed in (on the CSR handle)"""
    import numpy as np

    import block_jacobi_reference as BJ
    import iter_reference as R

    for variant in BJ.VARIANTS:
        for shape in ((6, 5, 4, 2), (5, 5, 4, 6)):
            c = BJ.Case(variant, shape + ((), (1,), ""), 1)
            bsr, A = c.problem()
            B = R.rhs(c.m, max(WIDTHS))
            plain = rails_amd.HipOperatorWrapper(ctx, A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data)
            blocked = rails_amd.HipOperatorWrapper.from_bsr(ctx, *bsr)
            for source, op, how in (("csr", plain, dict(block_jacobi=True, block_size=c.b)), ("bsr", blocked, dict(block_jacobi=True)),
                                    ("blocks", plain, dict(block_jacobi=BJ.diagonal_blocks(A, c.b)))):
                inv = rails_amd.IterativeInverse(ctx, op, method=c.method, tol=1e-10, maxit=2000, **how)
                both_calls(rails_amd, ctx, inv, B, out, "block_jacobi %s %dx%dx%d b%d %s" % ((c.variant,) + shape + (source,)), trans=c.trans)
                inv.close()


def block_cycle(rails_amd, ctx, out):
    """the block multigrid cycle: no level, two and three matrices, a positive definite operator, a block row longer than the LDS buffer"""
    import numpy as np

    import block_amg_reference as BA
    import iter_reference as R

    for tag in ("one4", "d4x4x3b3c24", "d6x6x6b3", "d8x8x8b4", "d4x4x3b3c24p", "long8"):
        (ip, ix, dt), coarse = BA.problem(tag)
        op = rails_amd.HipOperatorWrapper.from_bsr(ctx, np.asarray(ip, dtype=np.int64), np.asarray(ix, dtype=np.int32), np.ascontiguousarray(dt))
        B = R.rhs(int(op.M()), max(WIDTHS))
        inv = rails_amd.IterativeInverse(ctx, op, method="cg", tol=1e-10, maxit=2000, amg_coarse=coarse, block_amg=True)
        for S in (0, 1, 2):
            for fused in (1, 0):
                inv.set("amg_degree", S)
                inv.set("poly_fused", fused)
                both_calls(rails_amd, ctx, inv, B, out, "block_amg %s S%d fused%d" % (tag, S, fused))
        inv.close()


def two_ranks(rails_amd, out):
    import cheb_reference as C
    import iter_partition_cases as PC
    import iter_steps_reference as S

    for c, ranks in PC.STEP_CASES:
        if not c.poly or 2 not in ranks:
            continue
        A, B = c.matrix(), c.rhs()
        for K in (1, 4):
            def work(r, ctx, op, plan, r0, r1):
                inv = rails_amd.IterativeInverse(ctx, op, method="cg", tol=1e-10, maxit=40, jacobi=c.jacobi, poly_degree=K, poly_ratio=S.POLY_RATIO,
                                                 eig_max=C.gershgorin(A, C.g_of(A, c.jacobi)))
                inv.set("poly_fused", 1 if c.fused else 0)
                X = rails_amd.HipMultiVectorWrapper(ctx, data=B[r0:r1])
                solve, pre = Record(), Record()
                solve.add(inv, inv.solve(X))
                pre.add(inv, inv.precondition(X))
                inv.close()
                return solve, pre

            ranks = PC.run_ranks(2, PC.csr_triple(A), work)
            for call, rec0, rec1 in (("solve", ranks[0][0], ranks[1][0]), ("precondition", ranks[0][1], ranks[1][1])):
                rec0.merge(rec1)
                out["ranks2 %s K%d %s" % (c.id, K, call)] = rec0.json()


def child(tree, path):
    tree = os.path.abspath(tree)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, tree)
    import rails_amd

    assert os.path.dirname(os.path.abspath(rails_amd.__file__)) == os.path.join(tree, "rails_amd"), rails_amd.__file__
    out = {}
    ctx = rails_amd.Context(device=0, seed=1)
    single_gpu(rails_amd, ctx, out)
    ctx.close()
    two_ranks(rails_amd, out)
    with open(path, "w") as fh:
        json.dump({"counters": list(COUNTERS + CYCLE_COUNTERS), "cases": out}, fh)
    print("%d cases" % len(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", help="the tree to import rails_amd from (built)")
    ap.add_argument("--compare", nargs=2, metavar=("PARENT.json", "NEW.json"))
    ap.add_argument("--out", required=True)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--timeout", type=float, default=540.0, help="seconds the child process may take")
    a = ap.parse_args()
    if a.compare:
        sides = [json.load(open(p)) for p in a.compare]
        keys = sorted(set(sides[0]["cases"]) | set(sides[1]["cases"]))
        differ = [k for k in keys if sides[0]["cases"].get(k) != sides[1]["cases"].get(k)]
        equal = not differ and sides[0] == sides[1] and len(keys) > 0
        with open(a.out, "w") as fh:  # one line per case, both sides on it
            fh.write('{"equal": %s, "cases": %d, "differ": %s, "counters": %s, "sides": {\n' % (json.dumps(equal), len(keys), json.dumps(differ), json.dumps(sides[0]["counters"])))
            fh.write(",\n".join(' %s: {"parent": %s, "new": %s}' % (json.dumps(k), json.dumps(sides[0]["cases"].get(k)), json.dumps(sides[1]["cases"].get(k))) for k in keys))
            fh.write("\n}}\n")
        print("equal: %s (%d cases, %d differ)" % (equal, len(keys), len(differ)))
        for k in differ[:20]:
            print(k, sides[0]["cases"].get(k), sides[1]["cases"].get(k))
        sys.exit(0 if equal else 1)
    if a.child:
        child(a.tree, a.out)
        return
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--tree", a.tree, "--out", a.out], timeout=a.timeout)
    sys.exit(p.returncode)


if __name__ == "__main__":
    main()
