"""rails_orthogonalize_range (rails_amd/csrc/orth.hip: blocks of 128 columns, block operations only) against what a wide start space
costs through rails_orthogonalize, which takes the reference's column-wise recurrence above 256 columns (two norm passes and two
projection passes per column, a host synchronisation with every norm).  The same full-rank input for both: m x w random columns,
k_old = 0, refilled before every call (not timed).  One warm-up call, then the median of --reps timed calls each.  The counts of the
range routine (passes over a block of columns, host synchronisations) are the library's own counters (rails_ctx_stats); those of the
column-wise recurrence are read off its code: per column 2 norms (a pass and a synchronisation each) and 2 projections (a Gram pass
and an update pass each, against all columns before it).  Prints one JSON object; --out writes it to a file as well.

    python scripts/range_basis_bench.py [--m 200000] [--w 300] [--reps 3] [--out profiles/range_basis_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=200000)
    ap.add_argument("--w", type=int, default=300)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import rails_amd

    ctx = rails_amd.Context(device=0, seed=5)
    m, w = args.m, args.w
    X = rails_amd.HipMultiVectorWrapper(ctx, m=m, n=w, capacity=w)

    def timed(call):
        times = []
        for rep in range(args.reps + 1):  # the first call warms up (workspaces, code objects)
            ctx.set_seed(5, 0)
            X.resize(w)
            X.random()
            X.orthogonalized = 0
            ctx.sync()
            t0 = time.perf_counter()
            out = call()
            ctx.sync()
            times.append(time.perf_counter() - t0)
        return float(np.median(times[1:])), times[1:], out

    before = ctx.stats()
    t_col, all_col, used = timed(lambda: X.orthogonalize(0))
    mid = ctx.stats()
    t_rng, all_rng, (kept, _) = timed(lambda: X.orthogonalize_range())
    after = ctx.stats()
    G = X.dot(X)
    calls = args.reps + 1
    out = {
        "m": m, "w": w, "k_old": 0, "reps": args.reps,
        "rails_orthogonalize": {
            "median_s": t_col, "seconds": all_col, "method_used": used,
            "columnwise_calls": mid["orth_columnwise"] - before["orth_columnwise"],
            "host_synchronisations_from_code": 2 * w if used == 1 else None,
            "passes_from_code": 6 * w if used == 1 else None,
        },
        "rails_orthogonalize_range": {
            "median_s": t_rng, "seconds": all_rng, "kept": kept,
            "host_synchronisations": (after["orth_range_syncs"] - mid["orth_range_syncs"]) // calls,
            "passes": (after["orth_range_passes"] - mid["orth_range_passes"]) // calls,
            "orthonormality": float(np.abs(G - np.eye(kept)).max()),
        },
        "speedup": t_col / t_rng,
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
