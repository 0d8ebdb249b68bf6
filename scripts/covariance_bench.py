"""Pairs and one-point maps of the solution object X = U S U' (include/rails_solution.h) on one MI355X, timed with HIP events on the
context's stream (warm-up calls first, medians of --reps calls), one process:
  (a) rails_panel_rowquad, as a check against profiles/r06_solution.json, measured twice (first and last) for the run-to-run spread;
  (b) rails_panel_rowpair with identity index arrays (m pairs): the same kernel body plus the index upload and loads; (b0) the same
      with NULL for both (the identity without any index traffic): the pair kernel alone against (a);
  (c) the same with a random permutation for ia and another for ib: what the gathers cost;
  (d) the composition a caller had before: two rails_panel_move_rows into m x k temporaries, rails_panel_gemm_wide into a third, and a
      row-wise dot (torch.einsum on views of the panels, on the same stream);
  (e) Solution.maps at q = 16, covariances and correlations.
The event pair brackets the whole call as queued on the stream: for (b), (c) the staged upload of the 2 m indices (8 m bytes) is inside it.
Prints one JSON object; --out writes it to a file as well.

    python scripts/covariance_bench.py [--m 1000000] [--k 128 256] [--reps 20] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rails_amd._lib import check  # noqa: E402
from rails_amd.wrappers import _p  # noqa: E402

_i32p = C.POINTER(C.c_int32)


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
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=1000000)
    ap.add_argument("--k", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--reps", type=int, default=20)
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
    ident = np.arange(m, dtype=np.int32)
    pa, pb = g.permutation(m).astype(np.int32), g.permutation(m).astype(np.int32)
    result = {"m": m, "reps": args.reps, "device": torch.cuda.get_device_name(0), "cases": []}

    def view(panel, k):
        return torch.as_tensor(_DeviceArray(lib.rails_panel_device_ptr(panel.h), m, lib.rails_panel_ld(panel.h)), device="cuda")[:, :k]

    for k in args.k:
        U = MV(ctx, m, k)
        U.random()
        S = g.standard_normal((k, k))
        S = np.asfortranarray(S + S.T)
        out = MV(ctx, m, 1)

        def rowquad():
            check(lib.rails_panel_rowquad(ctx.h, U.panel.h, 0, k, _p(S), k, out.panel.h, 0), "rails_panel_rowquad")

        def rowpair(ia, ib):
            check(lib.rails_panel_rowpair(ctx.h, U.panel.h, 0, k, _p(S), k, ia.ctypes.data_as(_i32p), ib.ctypes.data_as(_i32p), m, out.panel.h, 0), "rails_panel_rowpair")

        a1 = timed(ctx, rowquad, args.reps)
        va = out.to_host()[:, 0]
        b = timed(ctx, lambda: rowpair(ident, ident), args.reps)
        vb = out.to_host()[:, 0]
        # the pair kernel without any index traffic (NULL = identity on both sides): the body's own cost against (a)
        b0 = timed(ctx, lambda: check(lib.rails_panel_rowpair(ctx.h, U.panel.h, 0, k, _p(S), k, None, None, m, out.panel.h, 0), "rails_panel_rowpair"), args.reps)
        c = timed(ctx, lambda: rowpair(pa, pb), args.reps)
        vc = out.to_host()[:, 0]
        # (d) the composition: gather both sides, P = Ua S, then sum_j P_ij Ub_ij
        Ua, Ub, P = MV(ctx, m, k), MV(ctx, m, k), MV(ctx, m, k)
        Pt, Bt = view(P.panel, k), view(Ub.panel, k)
        res = {}

        def composed():
            check(lib.rails_panel_move_rows(ctx.h, U.panel.h, 0, k, pa.ctypes.data_as(_i32p), m, 0, Ua.panel.h, 0), "rails_panel_move_rows")
            check(lib.rails_panel_move_rows(ctx.h, U.panel.h, 0, k, pb.ctypes.data_as(_i32p), m, 0, Ub.panel.h, 0), "rails_panel_move_rows")
            check(lib.rails_panel_gemm_wide(ctx.h, 1.0, Ua.panel.h, 0, k, _p(S), k, k, 0.0, P.panel.h, 0), "rails_panel_gemm_wide")
            res["v"] = torch.einsum("ij,ij->i", Pt, Bt)

        d = timed(ctx, composed, args.reps)
        vd = res["v"].cpu().numpy()
        temp = 3 * 8 * m * lib.rails_panel_ld(P.panel.h)
        del Ua, Ub, P, Pt, Bt
        a2 = timed(ctx, rowquad, args.reps)
        # (e) the maps
        sol = rails_amd.Solution(ctx, U, S)
        rows = g.integers(0, m, 16).astype(np.int32)
        e_cov = timed(ctx, lambda: sol.maps(rows, fetch=False), args.reps)
        e_cor = timed(ctx, lambda: sol.maps(rows, correlation=True, fetch=False), args.reps)
        sol.close()
        flop = 2.0 * m * k * k + 2.0 * m * k
        result["cases"].append({
            "k": k, "a_rowquad_first": a1, "a_rowquad_last": a2, "a_spread_last_over_first": a2["median_ms"] / a1["median_ms"],
            "b_rowpair_identity": b, "b_over_a": b["median_ms"] / a1["median_ms"], "b_tflops": flop / b["median_ms"] * 1e-9,
            "b0_rowpair_null_indices": b0, "b0_over_a": b0["median_ms"] / a1["median_ms"],
            "b_equals_a_bitwise": bool(np.array_equal(va.view(np.uint64), vb.view(np.uint64))),
            "c_rowpair_permuted": c, "c_over_b": c["median_ms"] / b["median_ms"],
            "d_composed": d, "d_over_c": d["median_ms"] / c["median_ms"], "d_max_rel_difference_to_c": float(np.abs(vc - vd).max() / np.abs(vd).max()),
            "temporary_bytes_rowpair": 8 * m + 2 * 4 * m, "temporary_bytes_composed": temp,
            "e_maps16_covariance": e_cov, "e_maps16_correlation": e_cor})
        del U, out
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
