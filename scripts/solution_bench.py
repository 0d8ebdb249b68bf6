"""The solution object X = U S U' (include/rails_solution.h) on one MI355X, timed with HIP events on the context's stream (warm-up calls
first, medians of --reps calls):
  (a) rails_panel_rowquad, the one-pass variance kernel (rails_amd/csrc/solution.hip);
  (b) what a caller could compose before it existed: rails_panel_gemm_wide into an m x k temporary, then a row-wise dot of the temporary
      with U (torch.einsum on views of the two panels, on the same stream);
  (c) trace, eigs(10) and apply at 16 columns of the object;
  (d) SchurOperator.lift on the MOC problem (tests/golden/moc_erik.npz) and on a synthetic descriptor system.
Prints one JSON object; --out writes it to a file as well.

    python scripts/solution_bench.py [--m 1000000] [--k 128 256] [--reps 20] [--out profiles/r06_solution.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rails_amd._lib import check  # noqa: E402
from rails_amd.wrappers import _p  # noqa: E402


class _DeviceArray:
    """a panel's device memory (m x ld doubles, row-major) for torch.as_tensor"""

    def __init__(self, ptr, m, ld):
        self.__cuda_array_interface__ = {"shape": (m, ld), "typestr": "<f8", "data": (ptr, False), "version": 2}


def timed(ctx, fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    ctx.sync()
    ms = []
    for _ in range(reps):
        ctx.timer_start()
        fn()
        ms.append(ctx.timer_stop())
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=1000000)
    ap.add_argument("--k", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-lift", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import rails_amd
    from rails_amd.wrappers import HipMultiVectorWrapper as MV

    tstream = torch.cuda.Stream(device=0)
    torch.cuda.set_stream(tstream)
    ctx = rails_amd.Context(device=0, stream=tstream.cuda_stream, seed=5)
    lib, m = ctx.lib, args.m
    g = np.random.default_rng(1)
    result = {"m": m, "reps": args.reps, "device": torch.cuda.get_device_name(0), "kernel": [], "object": [], "lift": []}
    for k in args.k:
        U = MV(ctx, m, k)
        U.random()
        S = g.standard_normal((k, k))
        S = np.asfortranarray(S + S.T)
        out = MV(ctx, m, 1)
        a_med, a_min = timed(ctx, lambda: check(lib.rails_panel_rowquad(ctx.h, U.panel.h, 0, k, _p(S), k, out.panel.h, 0), "rails_panel_rowquad"), args.reps)
        va = out.to_host()[:, 0]
        # (b) the composition: P = U S (m x k temporary), then sum_j P_ij U_ij
        P = MV(ctx, m, k)
        ld = lib.rails_panel_ld(U.panel.h)
        Ut = torch.as_tensor(_DeviceArray(lib.rails_panel_device_ptr(U.panel.h), m, ld), device="cuda")[:, :k]
        Pt = torch.as_tensor(_DeviceArray(lib.rails_panel_device_ptr(P.panel.h), m, lib.rails_panel_ld(P.panel.h)), device="cuda")[:, :k]
        res = {}

        def composed():
            check(lib.rails_panel_gemm_wide(ctx.h, 1.0, U.panel.h, 0, k, _p(S), k, k, 0.0, P.panel.h, 0), "rails_panel_gemm_wide")
            res["v"] = torch.einsum("ij,ij->i", Pt, Ut)

        b_med, b_min = timed(ctx, composed, args.reps)
        g_med, _ = timed(ctx, lambda: check(lib.rails_panel_gemm_wide(ctx.h, 1.0, U.panel.h, 0, k, _p(S), k, k, 0.0, P.panel.h, 0), "rails_panel_gemm_wide"), args.reps)
        vb = res["v"].cpu().numpy()
        flop = 2.0 * m * k * k + 2.0 * m * k
        result["kernel"].append({"k": k, "rowquad_ms": a_med, "rowquad_ms_min": a_min, "rowquad_tflops": flop / a_med * 1e-9, "composed_ms": b_med, "composed_ms_min": b_min,
                                 "composed_gemm_only_ms": g_med, "gemm_only_tflops": 2.0 * m * k * k / g_med * 1e-9, "temporary_bytes_composed": 8 * m * lib.rails_panel_ld(P.panel.h),
                                 "temporary_bytes_rowquad": 8 * m, "max_rel_difference": float(np.abs(va - vb).max() / np.abs(vb).max())})
        del P, Pt
        # (c) the object
        sol = rails_amd.Solution(ctx, U, S)
        W = MV(ctx, m, 16)
        W.random()
        t_med, _ = timed(ctx, sol.trace, args.reps)
        e_med, _ = timed(ctx, lambda: sol.eigs(10, fetch=False), max(3, args.reps // 4), warmup=1)
        p_med, _ = timed(ctx, lambda: sol.apply(W), args.reps)
        result["object"].append({"k": k, "trace_ms": t_med, "eigs10_ms": e_med, "apply16_ms": p_med})
        sol.close()
        del U, W, out
    if not args.skip_lift:
        import scipy.sparse as sp

        from rails_amd.schur import SchurOperator

        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import moc_problem

        def lift_case(name, A, mdiag, k):
            A = A.tocsr()
            A.sort_indices()
            c2 = rails_amd.Context(device=0, stream=tstream.cuda_stream, seed=5)
            sch = SchurOperator(c2, (A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data.astype(np.float64)), mdiag, tol=1e-12)
            V = MV(c2, sch.m2, k)
            V.random()
            T = g.standard_normal((k, k))
            sol = rails_amd.Solution(c2, V, T + T.T)
            med, mn = timed(c2, lambda: sch.lift(sol).close(), max(3, args.reps // 2), warmup=2)
            result["lift"].append({"problem": name, "n": int(A.shape[0]), "m1": int(sch.m1), "m2": int(sch.m2), "k": k, "lift_ms": med, "lift_ms_min": mn,
                                   "A11_levels": sch.dlu.levels() if sch.dlu else None})
            sol.close()
            c2.close()

        A, mdiag, _ = moc_problem.add_border(*moc_problem.load())
        lift_case("MOC with border", A, mdiag, 60)
        # synthetic: a 2-D 5-point operator on the dynamic unknowns, every fourth unknown an algebraic constraint coupled to its neighbours
        side = 300
        n = side * side
        T1 = sp.diags([np.ones(side - 1), -4.0 * np.ones(side), np.ones(side - 1)], [-1, 0, 1])
        L = (sp.kron(sp.identity(side), T1) + sp.kron(sp.diags([np.ones(side - 1), np.ones(side - 1)], [-1, 1]), sp.identity(side))).tolil()
        mdiag = np.where(np.arange(n) % 4 == 0, 0.0, 1.0)
        lift_case("synthetic 300 x 300 grid, a quarter of the unknowns algebraic", L.tocsr(), mdiag, 128)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
