#!/usr/bin/env python3
"""Microbenchmark of the fused update + second projection (rails_update_gram_deferred: X -= P C1, C2 = P'X in one pass over P) at the
basis widths a default bench.py run meets, m = 1M rows: HIP events around single calls through the C ABI, the pipelined schedule and the
kernel before it (rails_dense_set_update_gram_pipeline 1 / 0) interleaved in one process, medians of --reps.  One JSON line per shape:
microseconds, GB/s over the algorithmic traffic (k + 2 r) m 8 bytes and the fraction of the measured copy rate (6.29 TB/s).
A library without the switch (a build from before it) is timed as it is: one column, "old".

    python scripts/update_gram_bench.py [--m 1000000] [--reps 9] [--shapes 240x17,274x17,...]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE_GBS = 6290.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--shapes", default="240x17,274x17,289x17,316x9,340x17,345x9")
    args = ap.parse_args()
    import rails_amd
    from rails_amd._lib import check
    from rails_amd.wrappers import HipMultiVectorWrapper as MV, _p

    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    m, kmax = args.m, max(k for k, _ in shapes)
    ctx = rails_amd.Context(device=0, seed=3)
    lib = ctx.lib
    has_switch = hasattr(lib, "rails_dense_set_update_gram_pipeline")
    forms = (("old", 0), ("pipeline", 1)) if has_switch else (("old", None),)
    rng = np.random.default_rng(1)
    P = MV(ctx, m=m, n=kmax + 17, capacity=kmax + 17)
    for j in range(0, kmax + 17, 64):
        P.view(j, min(kmax + 17, j + 64) - 1).random()
    check(lib.rails_deferred_reserve(ctx.h, 8, (kmax + 64) * 32), "reserve")
    for k, r in shapes:
        r2 = min(r, 16)
        C1 = np.asfortranarray(rng.uniform(-1, 1, (k, r)) * 1e-6)

        def call():
            check(lib.rails_update_gram_deferred(ctx.h, -1.0, P.panel.h, 0, k, _p(C1), k, r, P.panel.h, k, r2, 0), "update_gram")

        samples = {name: [] for name, _ in forms}
        for name, v in forms:  # once each, untimed
            if v is not None:
                lib.rails_dense_set_update_gram_pipeline(v)
            call()
        ctx.sync()
        for _ in range(args.reps):
            for name, v in forms:
                if v is not None:
                    lib.rails_dense_set_update_gram_pipeline(v)
                ctx.timer_start()
                call()
                samples[name].append(ctx.timer_stop())
        nbytes = (k + 2 * r) * m * 8
        line = {"k": k, "r": r, "r2": r2, "m": m, "reps": args.reps}
        for name, _ in forms:
            ms = float(np.median(samples[name]))
            line[name] = {"us": round(ms * 1e3, 1), "min_us": round(min(samples[name]) * 1e3, 1), "max_us": round(max(samples[name]) * 1e3, 1),
                          "GBs": round(nbytes / ms / 1e6, 1), "frac_copy_rate": round(nbytes / ms / 1e6 / COPY_RATE_GBS, 3)}
        print(json.dumps(line), flush=True)
    if has_switch:
        lib.rails_dense_set_update_gram_pipeline(1)
    ctx.close()


if __name__ == "__main__":
    main()
