"""Block-CSR against CSR on the same matrix: problems.block_stencil7 at about one million rows (b = 2 at 80^3, 3 at 70^3, 4 at 64^3, 6 at
56^3), panels of 16, 32 and 128 columns.  The block-CSR handle and the CSR handle with variant 0 -- whichever kernels the automatic choice
takes, recorded -- are timed in one process, alternating, as medians of 20 products after 3 warm-ups, each product between HIP events.

Per case: the two times, the fraction of 8 TB/s each reaches on the algorithmic bytes of its format, the ratio
CSR / block-CSR, and the spread of the CSR repeats (largest minus smallest; the interquartile range beside it).  "faster" says whether
block-CSR beats CSR by more than twice that spread.

Every matrix runs in a child process under its own time limit, and the script stops at the first failure.

    python scripts/bsr_bench.py [--out profiles/bsr_spmm.json] [--cases 2:80,3:70,4:64,6:56] [--widths 16,32,128]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK = 8.0e12  # bytes per second


def child(b, n, widths, reps, warm):
    import rails_amd
    from rails_amd import problems as P

    (indptr, indices, data), (rowptr, col, val) = P.block_stencil7(n, n, n, b, seed=1)
    mb, m, nnzb, nnz = indptr.size - 1, rowptr.size - 1, indices.size, val.size
    ctx = rails_amd.Context(device=0, seed=1)
    blocked = rails_amd.HipOperatorWrapper.from_bsr(ctx, indptr, indices, data)
    plain = rails_amd.HipOperatorWrapper(ctx, rowptr, col, val)
    plain.set_variant(0)
    del data, val, col
    out = []
    for nc in widths:
        X = rails_amd.HipMultiVectorWrapper(ctx, m=m, n=nc, capacity=nc)
        X.random()
        Y = rails_amd.HipMultiVectorWrapper(ctx, m=m, n=nc, capacity=nc)
        times = {"bsr": [], "csr": []}
        for it in range(warm + reps):
            for name, op in (("bsr", blocked), ("csr", plain)):
                ctx.timer_start()
                op.apply(X, Y)
                ms = ctx.timer_stop()
                if it >= warm:
                    times[name].append(ms)
        tb, tc = np.array(times["bsr"]), np.array(times["csr"])
        bytes_b = nnzb * (b * b * 8 + 4) + (mb + 1) * 8 + 2 * m * nc * 8
        bytes_c = nnz * 12 + (m + 1) * 8 + 2 * m * nc * 8
        spread = float(tc.max() - tc.min())
        st = blocked.bsr_stats()
        out.append({"b": b, "grid": n, "rows": m, "nnz": int(nnz), "nnzb": int(nnzb), "cols": nc,
                    "bsr_ms": float(np.median(tb)), "csr_ms": float(np.median(tc)), "ratio_csr_over_bsr": float(np.median(tc) / np.median(tb)),
                    "bsr_bytes": int(bytes_b), "csr_bytes": int(bytes_c), "bsr_fraction_of_8TBs": bytes_b / (np.median(tb) * 1e-3) / PEAK,
                    "csr_fraction_of_8TBs": bytes_c / (np.median(tc) * 1e-3) / PEAK, "csr_spread_ms": spread,
                    "csr_iqr_ms": float(np.percentile(tc, 75) - np.percentile(tc, 25)), "bsr_spread_ms": float(tb.max() - tb.min()),
                    "faster": bool(np.median(tc) - np.median(tb) > 2.0 * spread), "bsr_kernel": "k_spmm_bsr<%d, %d>" % (st["B"], st["LPR"]),
                    "bsr_launch": {k: st[k] for k in ("threads", "rpg", "all_staged", "grid")}, "csr_kernel": plain.last_kernel(),
                    "bsr_device_bytes": int(st["device_bytes"]), "csr_device_bytes": int(nnz * 12 + (m + 1) * 8)})
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bsr_spmm.json"))
    ap.add_argument("--cases", default="2:80,3:70,4:64,6:56")
    ap.add_argument("--widths", default="16,32,128")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=float, default=240.0, help="seconds each child process may take")
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
            print("b %d, %d columns: block-CSR %.3f ms (%.0f %% of 8 TB/s), CSR %.3f ms (%.0f %%, %s), ratio %.2f, CSR spread %.3f ms, faster: %s" % (
                r["b"], r["cols"], r["bsr_ms"], 100 * r["bsr_fraction_of_8TBs"], r["csr_ms"], 100 * r["csr_fraction_of_8TBs"], r["csr_kernel"], r["ratio_csr_over_bsr"],
                r["csr_spread_ms"], r["faster"]), flush=True)
    with open(a.out, "w") as f:
        json.dump({"what": "block-CSR against CSR (variant 0) on problems.block_stencil7, medians of %d after %d warm-ups, alternating in one process" % (a.reps, a.warmup),
                   "peak_bytes_per_s": PEAK, "cases": rows}, f, indent=1)
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
