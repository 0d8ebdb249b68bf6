"""The multigrid preconditioner of the iterative A^-1 operator ("amg") measured against what the object had: per
solve, CG with Jacobi, CG with the Chebyshev polynomial at the best degree of section 15, and CG with the V-cycle, in the same run, at
1 / 16 / 32 columns to 1e-10 and 1e-6 on the 256^2 and 512^2 Laplacians, laplace7(100,100,100) and the 1M-row banded-random benchmark matrix
made symmetric and definite; and end to end on the 256^2 Laplacian (tolerance 1e-6, default back end): method 1, and method 2.2 with the
LU, CG, CG with the polynomial and CG with the V-cycle as A^-1.  Medians of --reps runs after --warmup, as scripts/iter_bench.py.  Prints
one JSON object per row; --out writes them all to a file.

    python scripts/amg_bench.py [--reps 10] [--warmup 2] [--widths 1 16 32] [--skip-large] [--skip-solver] [--out profiles/amg_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from iter_bench import iter_row, laplacian  # noqa: E402

POLY_DEGREE = 4           # the best degree at the default ratio
POLY_DEGREE_SOLVER = 8    # ... and the one its end-to-end line used


def symmetric_banded(m):
    """the benchmark's banded-random matrix made symmetric and definite: (B + B') / 2 off the diagonal, diagonal -(row sum + 1)"""
    import scipy.sparse as sp

    from rails_amd import problems as P

    rowptr, col, val = P.banded_random(m)
    B = sp.csr_matrix((val, col, rowptr), shape=(m, m))
    S = ((B + B.T) * 0.5).tocsr()
    S.setdiag(0.0)
    S.eliminate_zeros()
    S = (S - sp.diags(np.asarray(abs(S).sum(1)).ravel() + 1.0)).tocsr()
    S.sort_indices()
    return S


def solver_row(ctx, rails_amd, A, op, B, method, kind, **inverse_args):
    inverse = None
    t0 = time.perf_counter()
    if kind == "lu":
        inverse = rails_amd.SparseLU(ctx, A)
    elif kind:
        inverse = rails_amd.IterativeInverse(ctx, A, method="cg", tol=1e-8, maxit=20000, **inverse_args)
        if inverse_args.get("amg"):
            inverse.amg_setup()
    t_setup = time.perf_counter() - t0
    ctx.set_seed(1)
    s = rails_amd.Solver(ctx, op, B)
    if inverse is not None:
        s.set_inverse(inverse)
    assert s.set_parameters({"Maximum iterations": 3000, "Tolerance": 1e-6, "Expand size": 3, "Lanczos iterations": 10, "Projection method": method}) == 0
    s.set_option("verbose", 0)
    ctx.sync()
    t0 = time.perf_counter()
    code, V, T = s.solve()
    ctx.sync()
    row = {"problem": "laplace 256x256", "method": method, "inverse": kind, "code": code, "trips": s.trips(), "seconds": time.perf_counter() - t0,
           "inverse_setup_seconds": t_setup, "k": V.shape[1], "relative_residual": s.relative_residual()}
    if kind and kind != "lu":
        st = inverse.stats()
        row.update({"inner_solves": st["total_solves"], "inner_iterations": st["total_iterations"], "flagged_columns": st["total_flagged_columns"],
                    "inner_products_with_A": st["total_products"], **{k: v for k, v in inverse_args.items()}})
        if inverse_args.get("amg"):
            row["levels"] = inverse.amg_info()["rows"]
    s.close()
    if inverse is not None:
        inverse.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--widths", type=int, nargs="+", default=[1, 16, 32])
    ap.add_argument("--grids", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--skip-large", action="store_true", help="leave out the 1M-row operators")
    ap.add_argument("--skip-solver", action="store_true", help="leave out the end-to-end projection runs")
    ap.add_argument("--out")
    a = ap.parse_args()
    import scipy.sparse as sp

    import rails_amd
    from rails_amd import problems as P

    ctx = rails_amd.Context(device=0, seed=1)
    out = {"per_solve": [], "setup": [], "solver": []}

    def emit(key, row):
        out[key].append(row)
        print(json.dumps(row), flush=True)

    def save():
        if a.out:
            with open(a.out, "w") as fh:
                json.dump(out, fh, indent=1)

    problems = [("laplace %dx%d" % (k, k), lambda k=k: laplacian(k)) for k in a.grids]
    if not a.skip_large:
        def lap7():
            rowptr, col, val = P.laplace7(100, 100, 100)
            return sp.csr_matrix((val, col, rowptr), shape=(rowptr.size - 1, rowptr.size - 1))
        problems += [("laplace7(100,100,100)", lap7), ("banded_random(1000000), symmetric", lambda: symmetric_banded(1000000))]
    for name, make in problems:
        A = sp.csr_matrix(make())
        A.sort_indices()
        inv = rails_amd.IterativeInverse(ctx, A, method="cg", maxit=20000)
        inv.set("amg", 1)
        t0 = time.perf_counter()
        try:
            info = inv.amg_setup()
            emit("setup", {"problem": name, "n": A.shape[0], "nnz": int(A.nnz), "levels": info["rows"], "level_nnz": info["nnz"], "level_hi": info["hi"],
                           "operator_complexity": info["operator_complexity"], "host_setup_seconds": info["host_seconds"], "upload_seconds": info["upload_seconds"],
                           "setup_call_seconds": time.perf_counter() - t0})
            have_amg = True
        except rails_amd.RailsError as e:
            emit("setup", {"problem": name, "n": A.shape[0], "nnz": int(A.nnz), "refused": str(e), "setup_call_seconds": time.perf_counter() - t0})
            have_amg = False
        inv.set("amg", 0)
        for nc in a.widths:
            for tol in (1e-10, 1e-6):
                for variant in ("jacobi", "poly", "amg"):
                    if variant == "amg" and not have_amg:
                        continue
                    inv.set("poly_degree", POLY_DEGREE if variant == "poly" else 0)
                    inv.set("amg", 1 if variant == "amg" else 0)
                    row = iter_row(ctx, rails_amd, inv, A, name, nc, tol, a)
                    st = inv.stats()
                    row.update({"variant": variant, "poly_degree": POLY_DEGREE if variant == "poly" else 0, "inner_products": st["inner_products"],
                                "fused_launches": st["fused_launches"]})
                    if variant == "amg":
                        info = inv.amg_info()
                        row.update({"cycles": info["cycles"], "cycle_products": info["cycle_products"], "cycle_launches": info["cycle_launches"], "levels": info["rows"]})
                    inv.set("amg", 0)
                    emit("per_solve", row)
                    save()
        inv.close()

    if not a.skip_solver:
        A = laplacian(256)
        n = A.shape[0]
        op = rails_amd.HipOperatorWrapper(ctx, A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data.astype(np.float64))
        B = np.asfortranarray(np.random.default_rng(4).uniform(0, 1, (n, 1)))
        for method, kind, args in ((1.0, None, {}), (2.2, "lu", {}), (2.2, "iterative 1e-8", {}), (2.2, "iterative 1e-8", {"poly_degree": POLY_DEGREE_SOLVER}),
                                   (2.2, "iterative 1e-8", {"amg": True})):
            emit("solver", solver_row(ctx, rails_amd, A, op, B, method, kind, **args))
            save()
    ctx.close()
    save()


if __name__ == "__main__":
    main()
