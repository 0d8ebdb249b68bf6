"""Block Jacobi against point Jacobi for the conjugate-gradients inverse: problems.block_coupled7 at about one million rows (b = 4 at 64^3,
b = 6 at 56^3), spread 1e3, right-hand sides of 16 and 32 columns.  Three objects in one process, alternating:

  csr_point   point Jacobi on the CSR handle (variant 0: the automatic choice of kernel), what the driver builds without
              --inverse-block-jacobi
  bsr_point   point Jacobi on the block-CSR handle, the diagonal given
  bsr_block   block Jacobi on the block-CSR handle

Per object and width: (a) the time of one iteration, from solves with tolerance 0 and max_iterations K (every column runs exactly K
iterations; check_every K, so the host reads back once): medians of `reps` solves after `warmup`, each between HIP events, divided by K,
with the spread of the repeats (largest minus smallest) -- the start pass and the two panel copies are inside, spread over K iterations
alike for all three; (b) the iterations (most of a column) and the time of a solve to 1e-8, medians of `reps_b` solves with their spread.
Beside them what the byte count of DESIGN.md section 18 expects for block over point on the same handle, and whether block Jacobi reaches
1e-8 sooner than each point form by more than twice the spread of the slower object's repeats.

Every matrix runs in a child process under its own time limit, and the script stops at the first failure.

    python scripts/block_jacobi_bench.py [--out profiles/block_jacobi.json] [--cases 4:64,6:56] [--widths 16,32]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NAMES = ("csr_point", "bsr_point", "bsr_block")


def child(b, n, widths, K, reps, warm, reps_b):
    import rails_amd
    from rails_amd import problems as P

    (indptr, indices, data), (rowptr, col, val) = P.block_coupled7(n, n, n, b, 1e3, seed=1)
    m, nnzb = rowptr.size - 1, indices.size
    rows = np.repeat(np.arange(m), np.diff(rowptr))
    diag = np.zeros(m)
    diag[rows[rows == col]] = val[rows == col]
    ctx = rails_amd.Context(device=0, seed=1)
    blocked = rails_amd.HipOperatorWrapper.from_bsr(ctx, indptr, indices, data)
    plain = rails_amd.HipOperatorWrapper(ctx, rowptr, col, val)
    plain.set_variant(0)
    del data, val, col, rows
    inv = {"csr_point": rails_amd.IterativeInverse(ctx, plain, method="cg"),
           "bsr_point": rails_amd.IterativeInverse(ctx, blocked, method="cg", diag=diag),
           "bsr_block": rails_amd.IterativeInverse(ctx, blocked, method="cg", block_jacobi=True)}
    out = []
    for nc in widths:
        X = rails_amd.HipMultiVectorWrapper(ctx, m=m, n=nc, capacity=nc)
        X.random()
        Y = rails_amd.HipMultiVectorWrapper(ctx, m=m, n=nc, capacity=nc)
        row = {"b": b, "grid": n, "rows": m, "nnzb": int(nnzb), "cols": nc, "iterations_per_timed_solve": K}
        # (a) one iteration
        times = {k: [] for k in NAMES}
        for v in inv.values():
            v.set("tolerance", 0.0)
            v.set("max_iterations", K)
            v.set("check_every", K)
        for it in range(warm + reps):
            for name in NAMES:
                ctx.timer_start()
                inv[name].solve(X, Y)
                ms = ctx.timer_stop()
                if it >= warm:
                    times[name].append(ms / K)
        for name in NAMES:
            t = np.array(times[name])
            row[name] = {"ms_per_iteration": float(np.median(t)), "spread_ms": float(t.max() - t.min()), "repeats": len(t),
                         "kernel": inv[name].A.last_kernel()}
        # (b) to 1e-8
        for v in inv.values():
            v.set("tolerance", 1e-8)
            v.set("max_iterations", 5000)
            v.set("check_every", 8)
        times = {k: [] for k in NAMES}
        for it in range(1 + reps_b):
            for name in NAMES:
                ctx.timer_start()
                inv[name].solve(X, Y)
                ms = ctx.timer_stop()
                if it >= 1:
                    times[name].append(ms)
                st = inv[name].stats()
                row[name]["iterations_to_1e-8"] = st["max_iterations_of_a_column"]
                row[name]["unconverged_columns"] = st["unconverged_columns"]
        for name in NAMES:
            t = np.array(times[name])
            row[name]["ms_to_1e-8"] = float(np.median(t))
            row[name]["spread_ms_to_1e-8"] = float(t.max() - t.min())
        # a pass of the update moves 7 panels (reads p, q, x, r; writes x, r, z) and the preconditioner's 8 or 8 b bytes per row
        row["expected_update_pass_ratio"] = (7 * 8 * nc + 8 * b) / (7 * 8 * nc + 8)
        row["block_over_point_per_iteration"] = row["bsr_block"]["ms_per_iteration"] / row["bsr_point"]["ms_per_iteration"]
        for other in ("csr_point", "bsr_point"):
            gain = row[other]["ms_to_1e-8"] - row["bsr_block"]["ms_to_1e-8"]
            row["speedup_to_1e-8_over_" + other] = row[other]["ms_to_1e-8"] / row["bsr_block"]["ms_to_1e-8"]
            row["faster_than_" + other] = bool(gain > 2.0 * row[other]["spread_ms_to_1e-8"])
        out.append(row)
    for v in inv.values():
        v.close()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "block_jacobi.json"))
    ap.add_argument("--cases", default="4:64,6:56")
    ap.add_argument("--widths", default="16,32")
    ap.add_argument("--iterations", type=int, default=20, help="iterations of a timed solve of part (a)")
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps-b", type=int, default=5)
    ap.add_argument("--timeout", type=float, default=400.0, help="seconds each child process may take")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    widths = [int(w) for w in a.widths.split(",")]
    if a.child:
        b, n = (int(x) for x in a.child.split(":"))
        print(json.dumps(child(b, n, widths, a.iterations, a.reps, a.warmup, a.reps_b)))
        return 0
    rows = []
    for case in a.cases.split(","):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case, "--widths", a.widths, "--iterations", str(a.iterations), "--reps", str(a.reps),
                            "--warmup", str(a.warmup), "--reps-b", str(a.reps_b)], stdout=subprocess.PIPE, text=True, timeout=a.timeout)
        if p.returncode != 0:
            print("case %s failed with code %d: stopping" % (case, p.returncode))
            return 1
        rows += json.loads(p.stdout.splitlines()[-1])
        for r in rows[-len(widths):]:
            print("b %d, %d columns: ms per iteration %s; block / point on the block-CSR handle %.3f (update pass by bytes %.3f); to 1e-8: %s" % (
                r["b"], r["cols"], ", ".join("%s %.3f (+-%.3f)" % (k, r[k]["ms_per_iteration"], r[k]["spread_ms"]) for k in NAMES),
                r["block_over_point_per_iteration"], r["expected_update_pass_ratio"],
                ", ".join("%s %d iterations %.1f ms (+-%.1f)" % (k, r[k]["iterations_to_1e-8"], r[k]["ms_to_1e-8"], r[k]["spread_ms_to_1e-8"]) for k in NAMES)), flush=True)
    with open(a.out, "w") as f:
        json.dump({"what": "conjugate-gradients inverse on problems.block_coupled7 (spread 1e3): point Jacobi on the CSR handle and on the block-CSR handle, block Jacobi "
                           "on the block-CSR handle; (a) medians of %d solves of %d iterations after %d warm-ups, (b) medians of %d solves to 1e-8; alternating in one "
                           "process" % (a.reps, a.iterations, a.warmup, a.reps_b), "cases": rows}, f, indent=1)
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
