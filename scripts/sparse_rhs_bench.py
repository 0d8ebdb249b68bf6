"""One residual Lanczos run (k = 128 basis columns, L = 20 steps) on stencil27(200, 200, 25)-sized panels (m = 10^6) with B given as

  (a) a dense panel of p = 16 columns through the fused kernel (rails_resid_lanczos),
  (b) the same 16 columns as CSR through the sparse form (rails_resid_lanczos_sparse),
  (c) "selection" with p = 10^4 (one entry per column) through the sparse form,
  (d) the same B as (c) through the generic contract path -- the operation sequence of rails::Solver::resid_lanczos
      (rails/LyapunovSolver.hpp), which is what an operator B ran before the sparse form existed -- mirrored here call for call on the
      Python wrappers (B'q, B z, two Grams, two panel GEMMs, a dot, two axpys, a norm and a scaling per step).

Medians of 20 timed runs after 3 warm-up runs, wall clock around the synchronising call.  Writes profiles/r08_sparse_rhs.json.

    python scripts/sparse_rhs_bench.py [--out FILE] [--m ROWS]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, L, RUNS, WARM = 128, 20, 20, 3
HBM = 8e12


def selection(m, p, rng):
    j = np.arange(p)
    return sp.csr_matrix((rng.uniform(0.5, 1.5, p), (j * (m // p) + 1, j)), shape=(m, p))


def median_ms(fn, ctx):
    for _ in range(WARM):
        fn()
    ts = []
    for _ in range(RUNS):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def contract_lanczos(ctx, AV, V, T, Bop, steps):
    """rails::Solver::resid_lanczos on the wrappers"""
    from rails_amd.wrappers import HipMultiVectorWrapper as MV

    lib = ctx.lib
    Q = MV(ctx, m=AV.M(), n=steps + 1, capacity=steps + 2)
    q0 = Q.view(0)
    q0.random()
    q0 *= 1.0 / q0.norm()
    Bt = Bop.transpose()
    beta = 0.0
    H = np.zeros((steps + 1, steps + 1))
    for j in range(steps):
        qj, qn = Q.view(j), Q.view(j + 1)
        Bop.apply(Bt.apply(qj), qn)
        AV.gemm_into(T @ V.dot(qj), qn, 1.0, 1.0)
        V.gemm_into(T @ AV.dot(qj), qn, 1.0, 1.0)
        alpha = qn.dot(qj)[0, 0]
        H[j, j] = alpha
        lib.rails_panel_axpy(ctx.h, -alpha, qj.panel.h, qj.c0, 1, qn.panel.h, qn.c0)
        if j > 0:
            qp = Q.view(j - 1)
            lib.rails_panel_axpy(ctx.h, -beta, qp.panel.h, qp.c0, 1, qn.panel.h, qn.c0)
        beta = qn.norm()
        if beta < 1e-14:
            break
        H[j + 1, j] = H[j, j + 1] = beta
        qn *= 1.0 / beta
    return H


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_sparse_rhs.json"))
    ap.add_argument("--m", type=int, default=200 * 200 * 25)
    args = ap.parse_args()

    import rails_amd
    from rails_amd.wrappers import HipMultiVectorWrapper as MV

    m = args.m
    rng = np.random.default_rng(3)
    ctx = rails_amd.Context(device=0, seed=1)
    s = np.sqrt(3.0 / m)
    V = MV(ctx, data=s * rng.uniform(-1, 1, (m, K)), capacity=K)
    AV = MV(ctx, data=2.0 * s * rng.uniform(-1, 1, (m, K)), capacity=K)
    T = rng.uniform(-1, 1, (K, K))
    T = 0.05 * (T + T.T)
    B16 = rng.uniform(-1, 1, (m, 16))
    Bd = MV(ctx, data=B16, capacity=16)
    S16 = rails_amd.SparseRHS.from_scipy(ctx, sp.csr_matrix(B16))
    Bsel = selection(m, 10000, rng)
    Ssel = rails_amd.SparseRHS.from_scipy(ctx, Bsel)

    def step_bytes(p_dense, nnz, p):
        # the panels once, the three vectors of the recurrence and the write of the next one; a sparse B: its row pointers (8 B a row), its
        # entries twice (12 B each: the pass and the transposed product) and one gathered double per entry each time
        dense = (2 * K + p_dense + 4) * m * 8
        sparse = (m * 8 + 2 * nnz * (12 + 8) + 2 * p * 8) if nnz is not None else 0
        return dense + sparse

    cases = []

    def record(name, fn, nbytes, note):
        med, lo, hi = median_ms(fn, ctx)
        per_step = med / L
        out = dict(case=name, median_ms=med, min_ms=lo, max_ms=hi, ms_per_step=per_step, note=note)
        if nbytes:
            out.update(bytes_per_step=nbytes, fraction_of_8TBs=nbytes / (per_step * 1e-3) / HBM)
        print(json.dumps(out), flush=True)
        cases.append(out)

    record("a_dense_p16", lambda: rails_amd.resid_lanczos(ctx, AV, V, T, Bd, L), step_bytes(16, None, 0), "rails_resid_lanczos, B a 16-column panel")
    record("b_csr_p16", lambda: rails_amd.resid_lanczos_sparse(ctx, AV, V, T, S16, L), step_bytes(0, S16.nnz(), 16),
           "rails_resid_lanczos_sparse, the same 16 columns as CSR (16 entries in every row)")
    record("c_selection_p10000", lambda: rails_amd.resid_lanczos_sparse(ctx, AV, V, T, Ssel, L), step_bytes(0, Ssel.nnz(), 10000),
           "rails_resid_lanczos_sparse, one entry per column")
    record("d_selection_p10000_contract_path", lambda: contract_lanczos(ctx, AV, V, T, Ssel.op, L), None,
           "the operation sequence of rails::Solver::resid_lanczos on the Python wrappers")
    by = {c["case"]: c for c in cases}
    result = dict(m=m, k=K, L=L, runs=RUNS, warmup=WARM, device=rails_amd.load().rails_version().decode(), cases=cases,
                  c_faster_than_d=by["c_selection_p10000"]["median_ms"] < by["d_selection_p10000_contract_path"]["median_ms"],
                  d_over_c=by["d_selection_p10000_contract_path"]["median_ms"] / by["c_selection_p10000"]["median_ms"],
                  b_over_a=by["b_csr_p16"]["median_ms"] / by["a_dense_p16"]["median_ms"])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("c faster than d: %s (d / c = %.2f); b / a = %.2f" % (result["c_faster_than_d"], result["d_over_c"], result["b_over_a"]))
    for o in (S16, Ssel):
        o.close()
    ctx.close()
    return 0 if result["c_faster_than_d"] else 1


if __name__ == "__main__":
    sys.exit(main())
