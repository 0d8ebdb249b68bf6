"""Block multigrid against block Jacobi for the conjugate-gradients inverse: problems.block_diffusion7 (spread 100, reaction 0.01) at
about one million rows (b = 4 at 64^3, b = 6 at 56^3), right-hand sides of 16 and 32 columns.  Three objects on the block-CSR handle in one
process, alternating:

  block_jacobi   block Jacobi
  amg_fused      the block multigrid cycle with the fused step (k_cheb_step_bsr, k_amg_residual_bsr)
  amg_unfused    the same cycle with "poly_fused" 0 (rails_spmm and k_cheb_pass_bj)

Per object and width: the iterations (most of a column) and the time of a solve to 1e-8, medians of `reps` solves after `warmup`, each
between HIP events, with the spread of the repeats (largest minus smallest); for the two multigrid objects also the time of one cycle
(rails_iter_precondition, medians of `reps` after `warmup`).  Per case the hierarchy: rows per level, operator complexity, the host
set-up and upload times.  "amg_faster_than_block_jacobi": the fused cycle reaches 1e-8 sooner than block Jacobi by more than twice the
spread of the slower object's repeats; "fused_faster_than_unfused": the same for the fused against the unfused step.

Every matrix runs in a child process under its own time limit, and the script stops at the first failure.

    python scripts/block_amg_bench.py [--out profiles/block_amg.json] [--cases 4:64,6:56] [--widths 16,32]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NAMES = ("block_jacobi", "amg_fused", "amg_unfused")


def child(b, n, widths, reps, warm):
    import rails_amd
    from rails_amd import problems as P

    (indptr, indices, data), _ = P.block_diffusion7(n, n, n, b, 100.0, 0.01, seed=1)
    m, nnzb = (indptr.size - 1) * b, indices.size
    ctx = rails_amd.Context(device=0, seed=1)
    blocked = rails_amd.HipOperatorWrapper.from_bsr(ctx, indptr, indices, data)
    del data
    inv = {"block_jacobi": rails_amd.IterativeInverse(ctx, blocked, method="cg", block_jacobi=True),
           "amg_fused": rails_amd.IterativeInverse(ctx, blocked, method="cg", block_amg=True),
           "amg_unfused": rails_amd.IterativeInverse(ctx, blocked, method="cg", block_amg=True)}
    inv["amg_unfused"].set("poly_fused", 0)
    hier = {}
    for name in NAMES[1:]:
        info = inv[name].block_amg_setup()
        hier[name] = {k: info[k] for k in ("levels", "rows", "nnz", "hi", "operator_complexity", "host_seconds", "upload_seconds")}
    for v in inv.values():
        v.set("tolerance", 1e-8)
        v.set("max_iterations", 5000)
    out = []
    for nc in widths:
        X = rails_amd.HipMultiVectorWrapper(ctx, m=m, n=nc, capacity=nc)
        X.random()
        Y = rails_amd.HipMultiVectorWrapper(ctx, m=m, n=nc, capacity=nc)
        row = {"b": b, "grid": n, "rows": m, "nnzb": int(nnzb), "cols": nc, "hierarchy": hier["amg_fused"],
               "unfused_set_up": {k: hier["amg_unfused"][k] for k in ("host_seconds", "upload_seconds")}}
        times = {k: [] for k in NAMES}
        for it in range(warm + reps):
            for name in NAMES:
                ctx.timer_start()
                inv[name].solve(X, Y)
                ms = ctx.timer_stop()
                if it >= warm:
                    times[name].append(ms)
                st = inv[name].stats()
                row.setdefault(name, {}).update({"iterations_to_1e-8": st["max_iterations_of_a_column"], "unconverged_columns": st["unconverged_columns"],
                                                 "products": st["products"], "launches": st["launches"], "fused_launches": st["fused_launches"]})
        for name in NAMES:
            t = np.array(times[name])
            row[name].update({"ms_to_1e-8": float(np.median(t)), "spread_ms_to_1e-8": float(t.max() - t.min()), "repeats": len(t)})
        cyc = {k: [] for k in NAMES[1:]}
        for it in range(warm + reps):
            for name in NAMES[1:]:
                ctx.timer_start()
                inv[name].precondition(X, Y)
                ms = ctx.timer_stop()
                if it >= warm:
                    cyc[name].append(ms)
        for name in NAMES[1:]:
            t = np.array(cyc[name])
            row[name].update({"ms_per_cycle": float(np.median(t)), "spread_ms_per_cycle": float(t.max() - t.min())})
        slower = max(("block_jacobi", "amg_fused"), key=lambda k: row[k]["ms_to_1e-8"])
        row["speedup_to_1e-8_over_block_jacobi"] = row["block_jacobi"]["ms_to_1e-8"] / row["amg_fused"]["ms_to_1e-8"]
        row["amg_faster_than_block_jacobi"] = bool(row["block_jacobi"]["ms_to_1e-8"] - row["amg_fused"]["ms_to_1e-8"] > 2.0 * row[slower]["spread_ms_to_1e-8"])
        row["fused_over_unfused_to_1e-8"] = row["amg_fused"]["ms_to_1e-8"] / row["amg_unfused"]["ms_to_1e-8"]
        row["fused_over_unfused_per_cycle"] = row["amg_fused"]["ms_per_cycle"] / row["amg_unfused"]["ms_per_cycle"]
        slower = max(("amg_fused", "amg_unfused"), key=lambda k: row[k]["ms_to_1e-8"])
        row["fused_faster_than_unfused"] = bool(row["amg_unfused"]["ms_to_1e-8"] - row["amg_fused"]["ms_to_1e-8"] > 2.0 * row[slower]["spread_ms_to_1e-8"])
        out.append(row)
    for v in inv.values():
        v.close()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "block_amg.json"))
    ap.add_argument("--cases", default="4:64,6:56")
    ap.add_argument("--widths", default="16,32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=float, default=400.0, help="seconds each child process may take")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    widths = [int(w) for w in a.widths.split(",")]
    if a.child:
        b, n = (int(x) for x in a.child.split(":"))
        print(json.dumps(child(b, n, widths, a.reps, a.warmup)))
        return 0
    rows = []
    for case in a.cases.split(","):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case, "--widths", a.widths, "--reps", str(a.reps), "--warmup", str(a.warmup)],
                           stdout=subprocess.PIPE, text=True, timeout=a.timeout)
        if p.returncode != 0:
            print("case %s failed with code %d: stopping" % (case, p.returncode))
            return 1
        rows += json.loads(p.stdout.splitlines()[-1])
        for r in rows[-len(widths):]:
            print("b %d, %d columns, rows %s (complexity %.2f, set-up %.2f s + %.2f s): to 1e-8 %s; one cycle fused %.3f ms, unfused %.3f ms" % (
                r["b"], r["cols"], r["hierarchy"]["rows"], r["hierarchy"]["operator_complexity"], r["hierarchy"]["host_seconds"], r["hierarchy"]["upload_seconds"],
                ", ".join("%s %d iterations %.1f ms (+-%.1f)" % (k, r[k]["iterations_to_1e-8"], r[k]["ms_to_1e-8"], r[k]["spread_ms_to_1e-8"]) for k in NAMES),
                r["amg_fused"]["ms_per_cycle"], r["amg_unfused"]["ms_per_cycle"]), flush=True)
    with open(a.out, "w") as f:
        json.dump({"what": "conjugate-gradients inverse on problems.block_diffusion7 (spread 100, reaction 0.01) on the block-CSR handle: block Jacobi, the block multigrid "
                           "cycle with the fused step and with the unfused one; medians of %d solves to 1e-8 and of %d cycles after %d warm-ups, alternating in one "
                           "process" % (a.reps, a.reps, a.warmup), "cases": rows}, f, indent=1)
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
