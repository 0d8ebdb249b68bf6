"""The fused deflated block orthogonalisation (rails_orthogonalize_deflated, rails_amd/csrc/orth.hip: one Gram pass over [N V_old]'W, one
all-reduce and one update pass per projection round) against what a caller without it does: rails_orthogonalize against V_old, with N
projected out before and after it by separate Gram (rails_gram, to the host) and update (rails_panel_gemm) calls -- the solver template's
generic path.  W is refilled with random columns before every call (not timed).  Medians of --reps calls.  Prints one JSON object; --out
writes it to a file as well.

    python scripts/nullspace_bench.py [--m 1000000] [--kold 128 300] [--q 1 4 16] [--w 16 17] [--reps 20] [--out profiles/r05_nullspace.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rails_amd._lib import check  # noqa: E402


def orthonormal(ctx, lib, m, k):
    """k random orthonormal columns on the device (blocks of at most 64 columns through rails_orthogonalize)"""
    import rails_amd

    X = rails_amd.HipMultiVectorWrapper(ctx, m=m, n=k, capacity=max(k, 1))
    X.random()
    for k0 in range(0, k, 64):
        used = C.c_int(0)
        check(lib.rails_orthogonalize(ctx.h, X.panel.h, k0, min(64, k - k0), 0, C.byref(used)), "rails_orthogonalize")
    return X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=1000000)
    ap.add_argument("--kold", type=int, nargs="+", default=[128, 300])
    ap.add_argument("--q", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--w", type=int, nargs="+", default=[16, 17])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import rails_amd

    ctx = rails_amd.Context(device=0, seed=5)
    lib = ctx.lib
    m = args.m
    rows = []
    for k_old in args.kold:
        for q in args.q:
            # [V_old N] orthonormal as in the solver, where V is kept orthogonal to the nullspace; N in a panel of its own
            X = orthonormal(ctx, lib, m, k_old + q)
            Vold = X.view(0, k_old - 1)
            N = rails_amd.HipMultiVectorWrapper(ctx, m=m, n=q, capacity=q)
            check(lib.rails_panel_copy(ctx.h, X.panel.h, k_old, q, N.panel.h, 0), "rails_panel_copy")
            for w in args.w:
                P = rails_amd.HipMultiVectorWrapper(ctx, m=m, n=k_old + w, capacity=k_old + w)
                check(lib.rails_panel_copy(ctx.h, Vold.panel.h, 0, k_old, P.panel.h, 0), "rails_panel_copy")
                D = np.zeros((q, w), order="F")
                dp = D.ctypes.data_as(C.POINTER(C.c_double))
                used = C.c_int(0)

                def refill():
                    check(lib.rails_panel_random(ctx.h, P.panel.h, k_old, w), "rails_panel_random")
                    ctx.sync()

                def fused():
                    check(lib.rails_orthogonalize_deflated(ctx.h, P.panel.h, k_old, w, N.panel.h, 0, q, 0, C.byref(used)), "rails_orthogonalize_deflated")

                def project_n():
                    check(lib.rails_gram(ctx.h, N.panel.h, 0, q, P.panel.h, k_old, w, dp, q), "rails_gram")
                    check(lib.rails_panel_gemm(ctx.h, -1.0, N.panel.h, 0, q, dp, q, w, 1.0, P.panel.h, k_old), "rails_panel_gemm")

                def separate():
                    project_n()
                    project_n()
                    check(lib.rails_orthogonalize(ctx.h, P.panel.h, k_old, w, 0, C.byref(used)), "rails_orthogonalize")
                    project_n()
                    project_n()

                def plain():
                    check(lib.rails_orthogonalize(ctx.h, P.panel.h, k_old, w, 0, C.byref(used)), "rails_orthogonalize")

                times = {"plain": [], "fused": [], "separate": []}
                for rep in range(args.reps + 1):  # the first round warms every shape up and is not kept
                    for name, fn in (("plain", plain), ("fused", fused), ("separate", separate)):  # interleaved
                        refill()
                        t0 = time.perf_counter()
                        fn()
                        ctx.sync()
                        if rep:
                            times[name].append(time.perf_counter() - t0)
                # the result of the fused call: orthogonal to [N V_old] and orthonormal
                refill()
                fused()
                ctx.sync()
                L = np.zeros((q + k_old, w), order="F")
                Wd = P.view(k_old, k_old + w - 1)
                G = Wd.dot(Wd)
                ortho = float(np.abs(G - np.eye(w)).max())
                L[:q] = N.dot(Wd)
                L[q:] = Vold.dot(Wd)
                med = {k: float(np.median(v)) * 1e3 for k, v in times.items()}
                row = {"m": m, "k_old": k_old, "q": q, "w": w, "ms_plain": med["plain"], "ms_fused": med["fused"], "ms_separate": med["separate"],
                       "fused_over_plain": med["fused"] / med["plain"], "bound_(k_old+q+w)/(k_old+w)": (k_old + q + w) / (k_old + w),
                       "separate_over_fused": med["separate"] / med["fused"], "max_abs_NV_W": float(np.abs(L).max()), "max_abs_WtW_minus_I": ortho}
                rows.append(row)
                print(json.dumps(row), flush=True)
    out = {"what": "rails_orthogonalize_deflated vs rails_orthogonalize (plain, no nullspace) and vs rails_orthogonalize with separate N passes; "
                   "medians of %d calls, ms" % args.reps, "rows": rows}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
