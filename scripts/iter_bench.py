"""The iterative A^-1 operator (rails_iter_solve, rails_amd/csrc/itsolve.hip) measured: against rails_lu_solve on the 2D Laplacians, on
the benchmark's 1M-row 3D operators (time per solve, iterations, the split of an iteration into products and the library's own passes,
the passes against 8 TB/s), check_every at 1, 8 and 32, and the projection methods end to end on the 256 x 256 Laplacian.  Medians of
--reps runs after --warmup.  Prints one JSON object per row; --out writes them all to a file.

    python scripts/iter_bench.py [--reps 10] [--warmup 2] [--widths 1 16 32] [--skip-large] [--out profiles/iter_bench.json]

--poly K[,K..] runs the sweep of the Chebyshev polynomial preconditioner instead: CG to 1e-10 on the same
Laplacians and on laplace7(100,100,100) at every degree given, with the fused step kernel and without it, degree 0 in the same run as the
comparison, and the end-to-end line (256 x 256, method 2.2, CG at 1e-8) at degree 0 and at the degree that was fastest at 16 columns.

    python scripts/iter_bench.py --poly 0,2,4,8 [--poly-ratio R] --out profiles/iter_poly_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# passes over a work panel per iteration beside the products (loads + stores)
PASSES = {("cg", True): 12, ("cg", False): 10, ("bicgstab", True): 21, ("bicgstab", False): 17}
PRODUCTS = {"cg": 1, "bicgstab": 2}


def laplacian(k):
    import scipy.sparse as sp

    T = sp.diags([np.ones(k - 1), -4 * np.ones(k), np.ones(k - 1)], [-1, 0, 1])
    S = sp.diags([np.ones(k - 1), np.ones(k - 1)], [-1, 1])
    return (sp.kron(sp.eye(k), T) + sp.kron(S, sp.eye(k))).tocsr()


def timed(ctx, fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ctx.sync()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def iter_row(ctx, rails_amd, inv, A, name, nc, tol, a, split=False):
    n = A.shape[0]
    Bh = np.random.default_rng(nc).uniform(-1, 1, (n, nc))
    X = rails_amd.HipMultiVectorWrapper(ctx, data=Bh)
    Y = rails_amd.HipMultiVectorWrapper(ctx, n, nc)
    inv.set("tolerance", tol)
    med, lo, hi = timed(ctx, lambda: inv.solve(X, Y), a.reps, a.warmup)
    it, rel, flags = inv.columns()
    st = inv.stats()
    Yh = Y.to_host()
    true_rel = float((np.linalg.norm(A @ Yh - Bh, axis=0) / np.linalg.norm(Bh, axis=0)).max())
    row = {"problem": name, "n": n, "nc": nc, "method": inv.method, "tolerance": tol, "solve_ms": 1e3 * med, "solve_ms_min": 1e3 * lo, "solve_ms_max": 1e3 * hi,
           "iterations_max": int(it.max()), "iterations_min": int(it.min()), "flagged_columns": int((flags != 2).sum()), "true_relative_residual": true_rel,
           "launches": st["launches"], "products": st["products"]}
    if split:
        iters = int(it.max())
        P = rails_amd.HipMultiVectorWrapper(ctx, n, nc)
        t_prod, _, _ = timed(ctx, lambda: [inv.A.apply(X, P) for _ in range(20)], a.reps, a.warmup)
        t_prod /= 20
        per_iter = med / max(iters, 1)
        own = per_iter - PRODUCTS[inv.method] * t_prod
        nbytes = PASSES[(inv.method, True)] * nc * n * 8
        row.update({"ms_per_iteration": 1e3 * per_iter, "product_ms": 1e3 * t_prod, "products_per_iteration": PRODUCTS[inv.method],
                    "own_passes_ms_per_iteration": 1e3 * own, "own_passes_bytes_per_iteration": nbytes, "own_passes_TBps": nbytes / own / 1e12 if own > 0 else None,
                    "own_passes_fraction_of_8TBps": nbytes / own / 8e12 if own > 0 else None, "product_kernel": inv.A.last_kernel()})
    return row


def solver_row(ctx, rails_amd, A, op, B, method, kind, poly=0, ratio=None):
    """one end-to-end solve of the 256 x 256 problem: method 1, or 2.2 with the LU or CG at 1e-8 (polynomial of degree `poly`) as A^-1"""
    inverse = None
    t0 = time.perf_counter()
    if kind == "lu":
        inverse = rails_amd.SparseLU(ctx, A)
    elif kind:
        inverse = rails_amd.IterativeInverse(ctx, A, method="cg", tol=1e-8, maxit=20000, poly_degree=poly, poly_ratio=ratio)
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
                    "poly_degree": poly, "inner_products_with_A": st["total_products"]})
    s.close()
    if inverse is not None:
        inverse.close()
    return row


def poly_sweep(ctx, rails_amd, a, emit):
    import scipy.sparse as sp

    from rails_amd import problems as P

    degrees = [int(v) for v in a.poly.split(",")]
    problems = [("laplace %dx%d" % (k, k), laplacian(k)) for k in a.grids]
    if not a.skip_large:
        rowptr, col, val = P.laplace7(100, 100, 100)
        n = rowptr.size - 1
        problems.append(("laplace7(100,100,100)", sp.csr_matrix((val, col, rowptr), shape=(n, n))))
    best = {}
    for name, A in problems:
        inv = rails_amd.IterativeInverse(ctx, A, method="cg", maxit=20000, poly_ratio=a.poly_ratio)
        for nc in a.widths:
            for K in degrees:
                for fused in ((1, 0) if K else (1,)):
                    inv.set("poly_degree", K)
                    inv.set("poly_fused", fused)
                    row = iter_row(ctx, rails_amd, inv, A, name, nc, 1e-10, a)
                    st = inv.stats()
                    row.update({"poly_degree": K, "poly_fused": fused if K else None, "poly_ratio": st["eig_hi"] / st["eig_lo"] if K else None,
                                "inner_products": st["inner_products"], "fused_launches": st["fused_launches"]})
                    emit("poly", row)
                    if nc == 16 and (name not in best or row["solve_ms"] < best[name][0]):
                        best[name] = (row["solve_ms"], K)
        inv.close()
    if not a.skip_solver:
        A = laplacian(256)
        n = A.shape[0]
        op = rails_amd.HipOperatorWrapper(ctx, A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data.astype(np.float64))
        B = np.asfortranarray(np.random.default_rng(4).uniform(0, 1, (n, 1)))
        K = best.get("laplace 256x256", (0.0, max(degrees)))[1]
        for poly in sorted({0, K}):
            emit("poly_solver", solver_row(ctx, rails_amd, A, op, B, 2.2, "iterative 1e-8", poly=poly, ratio=a.poly_ratio))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--widths", type=int, nargs="+", default=[1, 16, 32])
    ap.add_argument("--grids", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--skip-large", action="store_true", help="leave out the 1M-row operators")
    ap.add_argument("--skip-solver", action="store_true", help="leave out the end-to-end projection runs")
    ap.add_argument("--poly", metavar="K[,K..]", help="the sweep of the polynomial preconditioner at these degrees, instead of everything else")
    ap.add_argument("--poly-ratio", type=float, default=None, help="hi / lo of the polynomial's interval (default: the library's)")
    ap.add_argument("--out")
    a = ap.parse_args()
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla

    import rails_amd
    from rails_amd import problems as P

    ctx = rails_amd.Context(device=0, seed=1)
    out = {"laplace2d": [], "large": [], "check_every": [], "solver": []}

    def emit(key, row):
        out.setdefault(key, []).append(row)
        print(json.dumps(row), flush=True)

    if a.poly:
        out = {}
        poly_sweep(ctx, rails_amd, a, emit)
        ctx.close()
        if a.out:
            with open(a.out, "w") as fh:
                json.dump(out, fh, indent=1)
        return

    for k in a.grids:
        A = laplacian(k)
        n = A.shape[0]
        inv = rails_amd.IterativeInverse(ctx, A, method="cg", maxit=20000)
        t0 = time.time()
        lu = rails_amd.SparseLU(ctx, A, lu=spla.splu(sp.csc_matrix(A), permc_spec="COLAMD"))
        t_factor = time.time() - t0
        for nc in a.widths:
            for tol in (1e-10, 1e-6):
                emit("laplace2d", iter_row(ctx, rails_amd, inv, A, "laplace %dx%d" % (k, k), nc, tol, a))
            X = rails_amd.HipMultiVectorWrapper(ctx, data=np.random.default_rng(nc).uniform(-1, 1, (n, nc)))
            Y = rails_amd.HipMultiVectorWrapper(ctx, n, nc)
            med, lo, hi = timed(ctx, lambda: lu.solve(X, Y), a.reps, a.warmup)
            emit("laplace2d", {"problem": "laplace %dx%d" % (k, k), "n": n, "nc": nc, "method": "lu", "solve_ms": 1e3 * med, "solve_ms_min": 1e3 * lo,
                               "solve_ms_max": 1e3 * hi, "factor_seconds": t_factor, "nnz_LU": lu.nnz})
        if k == 256:
            nc = 16
            X = rails_amd.HipMultiVectorWrapper(ctx, data=np.random.default_rng(nc).uniform(-1, 1, (n, nc)))
            Y = rails_amd.HipMultiVectorWrapper(ctx, n, nc)
            inv.set("tolerance", 1e-10)
            for every in (1, 8, 32):
                inv.set("check_every", every)
                med, lo, hi = timed(ctx, lambda: inv.solve(X, Y), a.reps, a.warmup)
                emit("check_every", {"problem": "laplace 256x256", "nc": nc, "check_every": every, "solve_ms": 1e3 * med, "solve_ms_min": 1e3 * lo,
                                     "solve_ms_max": 1e3 * hi, "iterations_max": int(inv.columns()[0].max())})
            inv.set("check_every", 8)
        lu.close()
        inv.close()

    if not a.skip_large:
        for name, triple, method in (("laplace7(100,100,100)", P.laplace7(100, 100, 100), "cg"),
                                     ("stencil27(100,100,100, random_values=True)", P.stencil27(100, 100, 100, random_values=True), "bicgstab")):
            rowptr, col, val = triple
            n = rowptr.size - 1
            A = sp.csr_matrix((val, col, rowptr), shape=(n, n))
            inv = rails_amd.IterativeInverse(ctx, A, method=method, maxit=20000)
            for nc in a.widths:
                emit("large", iter_row(ctx, rails_amd, inv, A, name, nc, 1e-10, a, split=True))
            inv.close()

    if not a.skip_solver:
        A = laplacian(256)
        n = A.shape[0]
        csr = (A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data.astype(np.float64))
        B = np.asfortranarray(np.random.default_rng(4).uniform(0, 1, (n, 1)))
        op = rails_amd.HipOperatorWrapper(ctx, *csr)
        for method, kind in ((1.0, None), (2.2, "lu"), (2.2, "iterative 1e-8")):
            emit("solver", solver_row(ctx, rails_amd, A, op, B, method, kind))
    ctx.close()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
