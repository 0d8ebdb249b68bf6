"""Bits, counters and text of whole solves through the C ABI (rails_amd/csrc/solver_capi.cpp over rails/LyapunovSolver.hpp) on small seeded
problems, both back ends, to compare two builds of the library: a refactoring of the outer loop must leave every result as it was.

    python scripts/solver_identity.py --tree PATH --out ONE.json     # imports rails_amd from PATH in a fresh child process, runs the cases
    python scripts/solver_identity.py --compare PARENT.json NEW.json --out profiles/solver_refactor_identity.json [--intended scale]

The cases: dense_stable 256 with p = 4 ("Restart size" 32, "Reduced size" 16), the n = 20 cases of tests/test_gpu_solver.py (restart by
size, no minimisation, minimisation, restart by trip count, warm start, a trip limit of 1, a trip budget), a mass matrix with
M-orthogonalisation, a nullspace, a start space with restart upon start, projection method 2.1 with the LU inverse, and a sparse B -- each
on both back ends where the option reaches both.  Per case: SHA-256 of V and of T, the history, trips, code, scale, ranks, the keys of
profile(), the counters of backend_stats() without the seconds, how far the integer counters of ctx.stats() moved, and the SHA-256 of what
the verbose solve printed.  --intended NAME: a field that may differ on the coordinate-space back end; it is listed, not counted."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sha(a):
    import numpy as np

    return hashlib.sha256(np.asfortranarray(a).tobytes(order="F")).hexdigest()


class CapturedStdout:
    """what the library prints on file descriptor 1 while the block runs"""

    def __enter__(self):
        sys.stdout.flush()
        self.saved, self.tmp = os.dup(1), tempfile.TemporaryFile()
        os.dup2(self.tmp.fileno(), 1)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 1)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode()
        self.tmp.close()


def tridiagonal_problem(np, n, seed):
    g = np.random.default_rng(seed)
    A = g.uniform(-1, 1, (n, n))
    for i in range(n):
        for j in range(n):
            if abs(i - j) > 1:
                A[i, j] = 0.0
            elif i == j:
                A[i, j] *= 3.0
    B = np.zeros((n, 1))
    B[n - 1, 0] = g.uniform(-1, 1)
    return A, B


def run_cases():
    import numpy as np
    import scipy.sparse as sp

    import rails_amd
    from rails_amd import problems as P

    ctx = rails_amd.Context(device=0, seed=1)
    out = {}

    def integers(stats):
        return {k: v for k, v in stats.items() if isinstance(v, int) and not isinstance(v, bool)}

    def case(name, A, B, params, subspace, seed=1, M=None, options=None, prepare=None, V0=None, keep=None):
        csr = A if isinstance(A, tuple) else P.dense_to_csr(A)
        op = rails_amd.HipOperatorWrapper(ctx, *csr)
        mop = rails_amd.HipOperatorWrapper(ctx, *M) if M is not None else None
        s = rails_amd.Solver(ctx, op, B, M=mop)
        prc = s.set_parameters(params)
        for key, value in {"verbose": 1, "subspace": subspace, **(options or {})}.items():
            s.set_option(key, value)
        held = prepare(s) if prepare else None
        ctx.set_seed(seed, 0)
        before = integers(ctx.stats())
        with CapturedStdout() as printed:
            code, V, T = s.solve(V0=V0)
        after = integers(ctx.stats())
        stats = s.backend_stats()
        stats.pop("seconds", None)
        tag = "%s [%s]" % (name, "coordinate" if subspace else "direct")
        out[tag] = {"set_parameters": prc, "code": code, "trips": s.trips(), "k": int(V.shape[1]), "V": sha(V), "T": sha(T), "history": [float(x).hex() for x in s.history()],
                    "scale": float(s.scale()).hex(), "nullspace_rank": s.nullspace_rank, "start_rank": s.start_rank, "profile_keys": sorted(s.profile()),
                    "backend": "coordinate" if stats else "direct", "backend_stats": {k: v for k, v in stats.items() if not isinstance(v, float)},
                    "ctx_moved": {k: after[k] - before.get(k, 0) for k in after}, "printed_lines": printed.text.count("\n"),
                    "printed": hashlib.sha256(printed.text.encode()).hexdigest()}
        print("%-64s code %2d trips %3d k %3d" % (tag, code, s.trips(), V.shape[1]), flush=True)
        if keep is not None:
            keep[subspace] = (V, T)
        s.close()
        if held is not None and hasattr(held, "close"):
            held.close()
        return V, T

    both = (1, 0)
    A, B = P.dense_stable(256, seed=1), P.rhs(256, 4, seed=2)
    for sub in both:
        case("dense_stable 256 p 4", A, B, {"Restart size": 32, "Reduced size": 16, "Expand size": 3, "Lanczos iterations": 10, "Tolerance": 1e-3}, sub)
    n20 = [("n20 restart size 19", 2, {"Restart Size": 19, "Reduced Size": 15, "Expand Size": 1, "Minimize solution space": 0}),
           ("n20 no minimisation", 3, {"Minimize solution space": 0, "Tolerance": 1e-8}),
           ("n20 minimisation", 3, {"Minimize solution space": 1, "Tolerance": 1e-8}),
           ("n20 restart iterations 10", 4, {"Restart iterations": 10, "Minimize solution space": 0, "Expand size": 1}),
           ("n20 trip limit 1", 3, {"Maximum iterations": 1}),
           ("n20 loose tolerance, trip limit 7", 3, {"Maximum iterations": 7, "Tolerance": 1e-1})]
    for name, seed, params in n20:
        A, B = tridiagonal_problem(np, 20, seed)
        for sub in both:
            case(name, A, B, params, sub)
    A, B = tridiagonal_problem(np, 20, 3)
    for sub in both:
        case("n20 trip budget 3", A, B, {"Tolerance": 1e-8}, sub, options={"max_trips": 3})
    A, B = tridiagonal_problem(np, 20, 5)
    prm = {"Minimize solution space": 1, "Tolerance": 1e-8}
    for sub in both:
        V, T = case("n20 cold for the warm start", A, B, prm, sub)
        A2 = A.copy()
        A2[19, 19] = 4.0
        case("n20 warm start", A2, B, {**prm, "Restart from solution": 1}, sub, V0=V)
    case("n20 restart from solution without a V", A, B, {**prm, "Restart from solution": 1}, 1)
    # mass matrix, V kept M-orthonormal
    A = P.laplace7(8, 8, 6)
    m = A[0].size - 1
    B = P.rhs(m, 3, seed=6)
    prm = {"Restart size": 40, "Reduced size": 20, "Expand size": 4, "Lanczos iterations": 8, "Tolerance": 1e-4}
    for sub in both:
        case("mass matrix, M-orthogonal", A, B, prm, sub, seed=9, M=P.mass_tridiag(m), options={"mass": 1, "mass_orthogonalisation": 1})
        case("mass matrix", A, B, prm, sub, seed=9, M=P.mass_tridiag(m), options={"mass": 1})
    # nullspace: the 2D Neumann Laplacian, kernel = the constants (tests/test_gpu_nullspace.py)
    k = 12
    Tm = 2 * np.eye(k) - np.eye(k, k=1) - np.eye(k, k=-1)
    Tm[0, 0] = Tm[-1, -1] = 1.0
    A = -(np.kron(np.eye(k), Tm) + np.kron(Tm, np.eye(k)))
    n = A.shape[0]
    N = np.ones((n, 1)) / np.sqrt(n)
    B = np.random.default_rng(11).uniform(-1, 1, (n, 2))
    B = np.asfortranarray(B - N @ (N.T @ B))
    prm = {"Expand size": 3, "Lanczos iterations": 10, "Tolerance": 1e-6}
    first = {}
    for sub in both:
        case("nullspace", A, B, prm, sub, prepare=lambda s: s.set_nullspace(np.ones((n, 2))), keep=first)
    # start space (neither orthonormal nor independent) with restart upon start; with the nullspace as well
    for sub in both:
        V1 = first[sub][0]
        S = np.hstack([V1, B, V1[:, :2] @ np.array([[1.0, 2.0], [-3.0, 0.5]])])
        case("start space, restart upon start", A - 0.5 * np.eye(n), B, {**prm, "Restart upon start": 1, "Reduced size": 8}, sub, prepare=lambda s: s.set_start_space(S))
        case("start space with a nullspace", A, B, prm, sub, prepare=lambda s: (s.set_nullspace(np.ones((n, 1))), s.set_start_space(S))[0])
    # projection method 2.1 with the LU inverse
    L = sp.csr_matrix(A - 0.5 * np.eye(n))
    L.sort_indices()
    csr = (L.indptr.astype(np.int64), L.indices.astype(np.int32), L.data.astype(np.float64))

    def with_lu(s):
        lu = rails_amd.SparseLU(ctx, csr)
        s.set_inverse(lu)
        return lu

    for sub in both:
        for method in (2.1, 1.2):
            case("projection method %g, LU inverse" % method, csr, B, {**prm, "Projection method": method, "Restart size": 30, "Reduced size": 12}, sub, prepare=with_lu)
    # sparse B (always the direct back end)
    A = P.laplace7(8, 8, 6)
    m = A[0].size - 1
    Bs = sp.random(m, 5, density=0.02, random_state=np.random.RandomState(3), format="csr")
    for sub in both:
        case("sparse B", A, Bs, {"Restart size": 40, "Reduced size": 20, "Expand size": 4, "Lanczos iterations": 8, "Tolerance": 1e-4}, sub)
    ctx.close()
    return out


def child(tree, path):
    tree = os.path.abspath(tree)
    sys.path.insert(0, tree)
    import rails_amd

    assert os.path.dirname(os.path.abspath(rails_amd.__file__)) == os.path.join(tree, "rails_amd"), rails_amd.__file__
    out = run_cases()
    with open(path, "w") as fh:
        json.dump({"cases": out}, fh)
    print("%d cases" % len(out))


def compare(parent, new, out, intended):
    sides = [json.load(open(p))["cases"] for p in (parent, new)]
    keys = sorted(set(sides[0]) | set(sides[1]))
    differ, allowed = [], {}
    for k in keys:
        a, b = sides[0].get(k), sides[1].get(k)
        if a == b:
            continue
        fields = sorted(f for f in set(a or {}) | set(b or {}) if (a or {}).get(f) != (b or {}).get(f))
        if a and b and b["backend"] == "coordinate" and set(fields) <= set(intended):
            allowed[k] = {f: {"parent": float.fromhex(a[f]) if isinstance(a[f], str) else a[f], "new": float.fromhex(b[f]) if isinstance(b[f], str) else b[f]} for f in fields}
        else:
            differ.append(k)
    equal = not differ and len(keys) > 0
    with open(out, "w") as fh:  # one line per case; both sides where they differ
        fh.write('{"what": "scripts/solver_identity.py: the parent commit\'s library against this one\'s, one fresh process each, same MI355X",\n')
        fh.write(' "equal": %s, "cases": %d, "differ": %s,\n "intended_change": %s,\n "sides": {\n' % (json.dumps(equal), len(keys), json.dumps(differ), json.dumps(allowed)))
        fh.write(",\n".join('  %s: %s' % (json.dumps(k), json.dumps(sides[1].get(k) if k not in differ else {"parent": sides[0].get(k), "new": sides[1].get(k)})) for k in keys))
        fh.write("\n }}\n")
    print("equal: %s (%d cases, %d differ, %d with an intended change)" % (equal, len(keys), len(differ), len(allowed)))
    for k in differ[:20]:
        a, b = sides[0].get(k) or {}, sides[1].get(k) or {}
        print(k, {f: (a.get(f), b.get(f)) for f in set(a) | set(b) if a.get(f) != b.get(f)})
    return 0 if equal else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", help="the tree to import rails_amd from (built)")
    ap.add_argument("--compare", nargs=2, metavar=("PARENT.json", "NEW.json"))
    ap.add_argument("--intended", action="append", default=[], help="a field that may differ on the coordinate-space back end")
    ap.add_argument("--out", required=True)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds the child process may take")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(a.compare[0], a.compare[1], a.out, a.intended))
    if a.child:
        child(a.tree, a.out)
        return
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--tree", a.tree, "--out", a.out], timeout=a.timeout)
    sys.exit(p.returncode if p.returncode >= 0 else 1)


if __name__ == "__main__":
    main()
