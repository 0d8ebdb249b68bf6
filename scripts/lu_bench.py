"""Device sparse LU solve (rails_lu_solve, rails_amd/csrc/splu.hip) against DeviceLU.solve (rails_amd/schur.py: sptrsv.hip with its two
permutation passes) on the same COLAMD factors of the 5-point Laplacian, and the projection methods 1 and 2.2 on the 256 x 256
Laplacian (default back end).  Prints one JSON object; --out writes it to a file as well.

    python scripts/lu_bench.py [--grids 256 512] [--widths 1 16 32] [--reps 20] [--solver] [--out profiles/lu_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def laplacian(k):
    import scipy.sparse as sp

    T = sp.diags([np.ones(k - 1), -4 * np.ones(k), np.ones(k - 1)], [-1, 0, 1])
    S = sp.diags([np.ones(k - 1), np.ones(k - 1)], [-1, 1])
    return (sp.kron(sp.eye(k), T) + sp.kron(S, sp.eye(k))).tocsc()


def timed(ctx, fn, reps):
    fn()
    ctx.sync()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        t.append(time.perf_counter() - t0)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--widths", type=int, nargs="+", default=[1, 16, 32])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--solver", action="store_true", help="also trips and wall time of methods 1 and 2.2 on the 256 x 256 Laplacian")
    ap.add_argument("--out")
    a = ap.parse_args()
    import scipy.sparse.linalg as spla

    import rails_amd
    from rails_amd.schur import DeviceLU

    ctx = rails_amd.Context(device=0, seed=1)
    out = {"solve": [], "solver": []}
    for k in a.grids:
        A = laplacian(k)
        n = A.shape[0]
        t0 = time.time()
        f = spla.splu(A, permc_spec="COLAMD")
        t_factor = time.time() - t0
        new = rails_amd.SparseLU(ctx, A, lu=f)
        old = DeviceLU(ctx, f)
        st = new.stats()
        factor_bytes = 2 * (new.nnz * 12 + (n + 1) * 8 + n * 8)  # both triangles of a solve: values + columns, row pointers, diagonal
        for nc in a.widths:
            X = rails_amd.HipMultiVectorWrapper(ctx, data=np.random.default_rng(nc).uniform(-1, 1, (n, nc)))
            Y = rails_amd.HipMultiVectorWrapper(ctx, n, nc)
            tmp = rails_amd.HipMultiVectorWrapper(ctx, n, nc)
            t_new = timed(ctx, lambda: new.solve(X, Y), a.reps)
            launches = new.stats()["launches"]
            t_old = timed(ctx, lambda: old.solve(X, tmp, Y), a.reps)
            Yn = new.solve(X).to_host()
            old.solve(X, tmp, Y)
            agree = float(np.abs(Yn - Y.to_host()).max() / np.abs(Yn).max())
            row = {"grid": k, "n": n, "nc": nc, "rails_lu_solve_ms": 1e3 * t_new, "DeviceLU_solve_ms": 1e3 * t_old, "speedup": t_old / t_new,
                   "levels": [st["levels_L"], st["levels_U"]], "levels_old": [old.levels()["L"], old.levels()["U"]], "nnz_LU": new.nnz,
                   "launches": launches, "factor_GBps": factor_bytes / t_new / 1e9, "max_rel_diff": agree, "factor_seconds": t_factor}
            out["solve"].append(row)
            print(json.dumps(row), flush=True)
        new.close()
        old.close()
    if a.solver:
        A = laplacian(256)
        n = A.shape[0]
        Acsr = A.tocsr()
        Acsr.sort_indices()
        csr = (Acsr.indptr.astype(np.int64), Acsr.indices.astype(np.int32), Acsr.data.astype(np.float64))
        B = np.asfortranarray(np.random.default_rng(4).uniform(0, 1, (n, 1)))
        op = rails_amd.HipOperatorWrapper(ctx, *csr)
        lu = rails_amd.SparseLU(ctx, A)
        for method in (1.0, 2.2):
            ctx.set_seed(1)
            s = rails_amd.Solver(ctx, op, B)
            s.set_inverse(lu)
            assert s.set_parameters({"Maximum iterations": 3000, "Tolerance": 1e-6, "Expand size": 3, "Lanczos iterations": 10,
                                     "Projection method": method}) == 0
            s.set_option("verbose", 0)
            ctx.sync()
            t0 = time.perf_counter()
            code, V, T = s.solve()
            ctx.sync()
            row = {"problem": "laplace 256x256", "method": method, "code": code, "trips": s.trips(), "seconds": time.perf_counter() - t0,
                   "k": V.shape[1], "relative_residual": s.relative_residual()}
            out["solver"].append(row)
            print(json.dumps(row), flush=True)
            s.close()
        lu.close()
    ctx.close()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
