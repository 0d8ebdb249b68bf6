"""The rule of the iterative A^-1 operator's preconditioners (rails_amd/csrc/iter_precond.h) as the library applies it (iter_setup.hip:
rails_iter_set; iter_hierarchy.hip: the set-ups and rails_iter_block_jacobi; itsolve.hip: begin_call), on three tiny objects: conjugate
gradients and BiCGStab on a CSR handle of the 6 x 6-cell, b = 2 block Laplacian of tests/block_amg_reference.py (72 rows), conjugate
gradients on its block-CSR handle.  (a) Every refusal -- each preconditioner asked for while each other one is on, and every single
request the rule refuses on the object -- has, as its whole message, the line that the host program of tests/test_iter_precond_host.py
prints for the object's facts.  (b) Switching from one preconditioner to another between two solves gives, bit for bit and counter for
counter, what an object that only ever had the second one gives: the work panels a later setting asks for are there and clean.  Nothing
here depends on size; width 3 has an odd last column beside the pad column."""
import os
import subprocess

import numpy as np
import pytest

import block_amg_reference as B
import iter_precond_reference as P
import iter_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rails_amd", "lib", "iter_precond_host")
TAG, BLOCK, ROWS, COARSE = "d6x6x1b2", 2, 72, 16  # (16 rows or fewer are inverted densely: both hierarchies have a level above that)
TOL, WIDTH = 1e-8, 3
OBJECTS = ("cg_csr", "bicgstab_csr", "cg_bsr")
# how a preconditioner is turned on and off through the settings, and the request that doing so makes of the rule
ON = {"poly_degree": ("poly_degree", P.POLY), "amg": ("amg", 1), "block_amg": ("block_amg", 1), "block_jacobi": ("block_jacobi", 1)}
COUNTERS = ("launches", "products", "inner_products", "poly_applications", "fused_launches", "allreduces", "halo_exchanges", "workspace_columns")
CYCLE_COUNTERS = ("cycles", "cycle_launches", "cycle_products")


@pytest.fixture(scope="module")
def ctx():
    import rails_amd

    c = rails_amd.Context(device=0, seed=3)
    yield c
    c.close()


@pytest.fixture(scope="module")
def lines():
    """the host program's table for 72 rows and b = 2: {(key of the facts, request, value): "granted" or the refusal}"""
    p = subprocess.run([EXE, "--table", str(ROWS), str(BLOCK)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:]
    out = {}
    for ln in p.stdout.splitlines():
        if ln.startswith("R "):
            key, request, answer = ln[2:].split(" | ", 2)
            out[(key,) + tuple(request.split())] = answer
    return out


_matrix = {}


def matrix():
    if not _matrix:
        ip, ix, dt = (np.asarray(t) for t in B.problem(TAG)[0])
        A = B.expand(ip, ix, dt)
        A.sort_indices()
        _matrix.update(triple=(ip.astype(np.int64), ix.astype(np.int32), np.ascontiguousarray(dt)), A=A, eig_max=float((np.asarray(abs(A).sum(axis=1)).ravel() / np.abs(A.diagonal())).max()), rhs=R.rhs(ROWS, WIDTH))
        assert A.shape == (ROWS, ROWS)
    return _matrix


def make(ctx, which):
    """a fresh object with every preconditioner off: the diagonal is given, so that the three differ in the method and the handle alone, and
    with it the Gershgorin bound of the Jacobi-scaled matrix, which a block-CSR handle cannot take from its arrays"""
    import rails_amd

    M = matrix()
    A = M["A"]
    if which.endswith("bsr"):
        op = rails_amd.HipOperatorWrapper.from_bsr(ctx, *M["triple"])
    else:
        op = rails_amd.HipOperatorWrapper(ctx, A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data)
    return rails_amd.IterativeInverse(ctx, op, method=which.split("_")[0], tol=TOL, maxit=500, diag=A.diagonal(), amg_coarse=COARSE, eig_max=M["eig_max"])


def facts_of(which, inv):
    """the facts of the object as it stands (the sign of the diagonal is no part of a request's line)"""
    on = {name: 0 for name in ON}
    on.update(inv._on)
    return P.facts(cg=which.startswith("cg"), op="bsr" if which.endswith("bsr") else "stored", m=ROWS, diag=1, blocks=inv.block_jacobi_info()["b"], poly_degree=on["poly_degree"],
                   amg=on["amg"], block_amg=on["block_amg"], block_jacobi=on["block_jacobi"])


def turn(inv, name, on):
    if name == "block_jacobi" and on and not inv.block_jacobi_info()["blocks"]:
        inv.block_jacobi(b=BLOCK)  # (installing turns it on)
    else:
        inv.set(ON[name][0], ON[name][1] if on else 0)
    inv._on[name] = ON[name][1] if on else 0


def ask(inv, request):
    """makes the request of the library"""
    if request in ON:
        inv.set(*ON[request])
    elif request == "install_blocks":
        inv.block_jacobi(b=BLOCK)
    elif request == "amg_setup":
        inv.amg_setup()
    else:
        inv.block_amg_setup()


def message(call):
    import rails_amd

    with pytest.raises(rails_amd.RailsError) as e:
        call()
    return str(e.value).split("): ", 1)[1]


def value_of(request):
    return ON[request][1] if request in ON else BLOCK if request == "install_blocks" else 1


def available(lines, which):
    """the preconditioners the rule grants on the fresh object (block Jacobi: once its blocks are installed)"""
    f = P.facts(cg=which.startswith("cg"), op="bsr" if which.endswith("bsr") else "stored", m=ROWS, diag=1, blocks=BLOCK)
    return [name for name in ON if lines[(P.key(f), name, str(ON[name][1]))] == "granted"]


@pytest.mark.parametrize("which", OBJECTS)
def test_refusals_are_the_rules_lines(ctx, lines, which):
    inv = make(ctx, which)
    inv._on = {}
    requests = [r for r, _, _ in P.REQUESTS]
    asked = 0

    def refusals_now():
        n = 0
        for request in requests:
            want = lines[(P.key(facts_of(which, inv)), request, str(value_of(request)))]
            if want != "granted":
                assert message(lambda: ask(inv, request)) == want, (which, inv._on, request)
                n += 1
        return n

    # every single request the rule refuses on the object: without blocks, then with blocks installed and off
    single = refusals_now()
    inv.block_jacobi(b=BLOCK)
    inv.set("block_jacobi", 0)
    single += refusals_now()
    assert single >= {"cg_csr": 3, "bicgstab_csr": 9, "cg_bsr": 3}[which], single
    # every ordered pair: the first on, then the second asked for -- as a setting, and as the install or the set-up that goes with it
    firsts = available(lines, which)
    assert firsts == {"cg_csr": ["poly_degree", "amg", "block_jacobi"], "bicgstab_csr": ["block_jacobi"], "cg_bsr": ["poly_degree", "block_amg", "block_jacobi"]}[which]
    for first in firsts:
        turn(inv, first, True)
        f = facts_of(which, inv)
        for second in ON:
            if second != first:
                assert lines[(P.key(f), second, str(ON[second][1]))] != "granted"
        asked += refusals_now()
        turn(inv, first, False)
    assert asked >= len(firsts) * 5
    # the object still solves
    turn(inv, firsts[-1], True)
    import rails_amd

    X = inv.solve(rails_amd.HipMultiVectorWrapper(ctx, data=matrix()["rhs"]))
    assert R.true_relres(matrix()["A"], X.to_host(), matrix()["rhs"]).max() <= 100 * TOL and np.all(inv.columns()[2] == 2)
    inv.close()


def outcome(ctx, inv):
    """one solve of WIDTH columns: the result's bits, the columns and the counters (a hierarchy left from an earlier setting is no part of
    them: the cycle's counters are those of the last call)"""
    import rails_amd

    Y = inv.solve(rails_amd.HipMultiVectorWrapper(ctx, data=matrix()["rhs"])).to_host()
    it, rel, flags = inv.columns()
    st, amg, bamg = inv.stats(), inv.amg_info(), inv.block_amg_info()
    return Y.tobytes(), it.tobytes(), rel.tobytes(), flags.tobytes(), [st[n] for n in COUNTERS], [amg[n] for n in CYCLE_COUNTERS], [bamg[n] for n in CYCLE_COUNTERS]


_fresh = {}


def fresh(ctx, which, name):
    """what an object that only ever had `name` on gives, computed once"""
    if (which, name) not in _fresh:
        inv = make(ctx, which)
        inv._on = {}
        turn(inv, name, True)
        _fresh[(which, name)] = outcome(ctx, inv)
        if name in ("amg", "block_amg"):  # a level above the dense one
            assert (inv.amg_info() if name == "amg" else inv.block_amg_info())["levels"] >= 2
        assert np.all(np.frombuffer(_fresh[(which, name)][3], dtype=np.int32) == 2)  # (converged: the comparison is of complete solves)
        inv.close()
    return _fresh[(which, name)]


PAIRS = [(which, first, second) for which, names in (("cg_csr", ("poly_degree", "amg", "block_jacobi")), ("cg_bsr", ("poly_degree", "block_amg", "block_jacobi")))
         for first in names for second in names if first != second]


@pytest.mark.parametrize("which,first,second", PAIRS, ids=["%s-%s-then-%s" % p for p in PAIRS])
def test_switching_gives_the_bits_of_a_fresh_object(ctx, lines, which, first, second):
    assert first in available(lines, which) and second in available(lines, which)
    inv = make(ctx, which)
    inv._on = {}
    turn(inv, first, True)
    outcome(ctx, inv)
    turn(inv, first, False)
    turn(inv, second, True)
    got, want = outcome(ctx, inv), fresh(ctx, which, second)
    inv.close()
    names = ("result", "iterations", "residuals", "flags", "counters", "amg_info", "block_amg_info")
    differ = [n for n, g, w in zip(names, got, want) if g != w]
    assert not differ, (differ, got[4:], want[4:])
    if second in ("amg", "block_amg"):
        assert (got[5] if second == "amg" else got[6])[0] > 0  # the cycle ran
