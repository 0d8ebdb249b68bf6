"""One call through the public entry points per row of the table that rails_amd/lib/dense_choice_host --table prints (the smallest shape
that reaches each instantiation of the dense kernels, rails_amd/csrc/dense_choice.h), for tests/test_gpu_dense_choice.py and
scripts/dense_identity.py.  A row is a dict: primitive, m, the shape, switches; kernel and inst where the row is one of the table's.

    gram          rails_gram                        gemm_wide     rails_panel_gemm_wide
    panel_gemm    rails_panel_gemm                  update_gram   rails_update_gram_deferred
    gram2, panel_gemm2   rails_orthogonalize_deflated (the two-segment kernels: the nullspace and the old basis as one left operand)

run_row returns the arrays the call wrote (with what lies around the written window), what the context says it launched, and a function
that holds the result against a float64 numpy product within the bound the existing test of that entry point uses (cited there).
Run as a program with a row as JSON it makes that one call and checks it: a row with an environment switch off runs this way, in a fresh
process with the variable set."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rails_amd", "lib", "dense_choice_host")
DP = C.POINTER(C.c_double)
ENV_SWITCHES = {"gram_cols": "RAILS_GRAM_COLS", "gram_extra_column": "RAILS_GRAM_EXTRA_COLUMN", "fused_update_gram": "RAILS_FUSED_UPDATE_GRAM",
                "panel_gemm_wide": "RAILS_PANEL_GEMM_WIDE"}


def table():
    p = subprocess.run([EXE, "--table"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:]
    return [json.loads(line) for line in p.stdout.splitlines()]


def row_id(row):
    shape = "-".join("%s=%d" % (n, row[n]) for n in ("a", "b", "k", "r", "r2") if n in row)
    off = "".join("-no_" + n for n, v in sorted(row.get("switches", {}).items()) if not v)
    return "%s<%s>-%s%s" % (row.get("kernel", row["primitive"]), ",".join(str(i) for i in row.get("inst", [])), shape, off)


def env_of(row):
    """the environment variables a row needs set (to 0) before the library is first used"""
    return {ENV_SWITCHES[n]: "0" for n, v in row.get("switches", {}).items() if n in ENV_SWITCHES and not v}


def last_launch(ctx):
    nbw, ti, tr, form = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_int(-1)
    assert ctx.lib.rails_dense_last_tiles(ctx.h, C.byref(nbw), C.byref(ti), C.byref(tr)) == 0
    assert ctx.lib.rails_dense_last_update_gram_form(ctx.h, C.byref(form)) == 0
    return {"update_gram_nbw": nbw.value, "gram_cols_ti": ti.value, "gemm_wide_tr": tr.value, "update_gram_form": form.value}


def run_row(rails_amd, ctx, row):
    """-> (arrays written, what the context launched last and its update_gram_fused count for this call, check())"""
    lib, chk, MV = ctx.lib, rails_amd._lib.check, rails_amd.HipMultiVectorWrapper
    sw = row.get("switches", {})
    lib.rails_dense_set_tile_fit(sw.get("tile_fit", 1))
    lib.rails_dense_set_update_gram_pipeline(sw.get("update_gram_pipeline", 1))
    m, prim, inst = row["m"], row["primitive"], row.get("inst")
    g = np.random.default_rng(sum(1000 ** i * row.get(n, 0) for i, n in enumerate(("a", "b", "k", "r", "r2"))) + m)
    fused0 = ctx.stats().get("update_gram_fused", 0)
    expect = {}
    if prim == "gram":
        a, b = row["a"], row["b"]
        Xh, Yh = g.uniform(-1, 1, (m, a)), g.uniform(-1, 1, (m, b))
        X, Y = MV(ctx, data=Xh), MV(ctx, data=Yh)
        G = np.zeros((a, b), order="F")
        chk(lib.rails_gram(ctx.h, X.panel.h, 0, a, Y.panel.h, 0, b, G.ctypes.data_as(DP), a), "rails_gram")
        arrays = [G]
        if row.get("kernel") == "k_gram_cols":
            expect["gram_cols_ti"] = inst[0]

        def check():  # tests/test_gpu_kernels.py:221 (test_gram_matches_oracle), tests/test_gpu_tile_fit.py:106
            assert np.abs(G - Xh.T @ Yh).max() <= 1e-14 * m + 1e-13 * np.sqrt(m)
    elif prim == "panel_gemm":
        r, k = row["r"], row.get("k", 33)
        Xh, Ch, Y0 = g.uniform(-1, 1, (m, k)), np.asfortranarray(g.uniform(-1, 1, (k, r))), g.uniform(-1, 1, (m, r + 2))
        X, Y = MV(ctx, data=Xh), MV(ctx, data=Y0)
        chk(lib.rails_panel_gemm(ctx.h, 1.0, X.panel.h, 0, k, Ch.ctypes.data_as(DP), k, r, 0.0, Y.panel.h, 1), "rails_panel_gemm")
        out = Y.to_host()
        arrays = [out]

        def check():  # tests/test_gpu_kernels.py:244 (test_panel_gemm_matches_oracle)
            assert np.abs(out[:, 1:r + 1] - Xh @ Ch).max() <= 1e-14 * k * 4
            assert np.array_equal(out[:, :1], Y0[:, :1]) and np.array_equal(out[:, r + 1:], Y0[:, r + 1:])
    elif prim == "gemm_wide":
        k, r = row["k"], row["r"]
        alpha, beta = row.get("alpha", 1.0), row.get("beta", 0.0)
        Xh, Qh, Y0 = g.uniform(-1, 1, (m, k)), np.asfortranarray(g.uniform(-1, 1, (k, r))), g.uniform(-1, 1, (m, r + 2))
        X, Y = MV(ctx, data=Xh), MV(ctx, data=Y0)
        chk(lib.rails_panel_gemm_wide(ctx.h, alpha, X.panel.h, 0, k, Qh.ctypes.data_as(DP), k, r, beta, Y.panel.h, 1), "rails_panel_gemm_wide")
        out = Y.to_host()
        arrays = [out]
        if inst and r <= 288:  # (one slice: the last launch is the row's)
            expect["gemm_wide_tr"] = inst[0]

        def check():  # tests/test_gpu_kernels.py:431 (test_panel_gemm_wide_matches_numpy), tests/test_gpu_tile_fit.py:145
            np.testing.assert_allclose(out[:, 1:r + 1], beta * Y0[:, 1:r + 1] + alpha * (Xh @ Qh), rtol=0, atol=1e-13 * k)
            assert np.array_equal(out[:, :1], Y0[:, :1]) and np.array_equal(out[:, r + 1:], Y0[:, r + 1:])
    elif prim == "update_gram":
        k, r, r2 = row["k"], row["r"], row["r2"]
        # the block right behind the basis in the same panel (tests/test_gpu_tile_fit.py: the columns between k and k rounded up to 4 are Y's)
        Xh = g.uniform(-1, 1, (m, k + r + 2))
        Ch = np.asfortranarray(g.uniform(-1, 1, (k + 3, r)))
        chk(lib.rails_deferred_reserve(ctx.h, 3, (k + 64) * 32), "rails_deferred_reserve")
        P = MV(ctx, data=Xh)
        chk(lib.rails_update_gram_deferred(ctx.h, -0.5, P.panel.h, 0, k, Ch.ctypes.data_as(DP), k + 3, r, P.panel.h, k, r2, 1), "rails_update_gram_deferred")
        ctx.sync()
        slot = np.zeros((k, r2), order="F")
        chk(lib.rails_deferred_fetch(ctx.h, 1, k * r2, slot.ctypes.data_as(DP)), "rails_deferred_fetch")
        panel = P.to_host()
        arrays = [panel, slot]
        if inst:
            expect.update(update_gram_nbw=inst[0], update_gram_form=2 if row["kernel"] == "k_update_gram_p" else 1, fused=1)

        def check():  # tests/test_gpu_kernels.py:541,546 (test_update_and_second_projection_in_one_pass), tests/test_gpu_tile_fit.py:79-81
            Xa = Xh[:, :k]
            Ynew = Xh[:, k:k + r] - 0.5 * (Xa @ Ch[:k])
            scale = np.abs(Ynew).max()
            np.testing.assert_allclose(panel[:, k:k + r], Ynew, rtol=0, atol=1e-13 * k * scale)
            assert np.array_equal(panel[:, :k], Xa) and np.array_equal(panel[:, k + r:], Xh[:, k + r:])
            np.testing.assert_allclose(slot, Xa.T @ Ynew[:, :r2], rtol=0, atol=1e-13 * m * scale)
    elif prim in ("gram2", "panel_gemm2"):
        # [N | V_old] with a = q + k_old columns against a block of b (or r) columns
        w = row["b"] if prim == "gram2" else row["r"]
        a = row["a"] if prim == "gram2" else 24
        q = 1 if a < 8 else 4
        NV = np.linalg.qr(g.uniform(-1, 1, (m, a)))[0]
        N, Vold, W = NV[:, :q], NV[:, q:], g.uniform(-1, 1, (m, w))
        X = MV(ctx, data=np.hstack([Vold, W]), capacity=a - q + w)
        X.orthogonalized = a - q
        used = X.orthogonalize_deflated(MV(ctx, data=N), 0)
        out = X.to_host()
        arrays = [out, np.array([used], dtype=np.int64)]
        if row.get("kernel") == "k_gram_cols2":
            expect["gram_cols_ti"] = inst[0]

        def check():  # tests/test_gpu_orth_deflated.py:69 and its check(), lines 51-55, at m = 1003 (orth_bound: 1e-13)
            Q = out[:, a - q:]
            ref, R = np.linalg.qr(W - NV @ (NV.T @ W))
            np.testing.assert_allclose(Q, ref * np.sign(np.diag(R))[None, :], rtol=0, atol=1e-12)
            assert np.array_equal(out[:, :a - q], Vold) and np.all(np.isfinite(Q))
            assert np.abs(NV.T @ Q).max() <= max(1e-13, 5e-15 * np.sqrt(m))
            assert np.abs(Q.T @ Q - np.eye(w)).max() <= max(1e-13, 5e-15 * np.sqrt(m))
    else:
        raise ValueError(prim)
    launched = last_launch(ctx)
    launched["fused"] = ctx.stats().get("update_gram_fused", 0) - fused0
    return arrays, launched, check, expect


def check_row(rails_amd, ctx, row):
    arrays, launched, check, expect = run_row(rails_amd, ctx, row)
    for name, value in expect.items():
        assert launched[name] == value, (name, launched, expect)
    check()


def check_row_in_child(row):
    """a fresh process with the row's environment variables set"""
    p = subprocess.run([sys.executable, os.path.abspath(__file__), json.dumps(row)], env=dict(os.environ, **env_of(row)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=120)
    assert p.returncode == 0 and "ROW PASSED" in p.stdout, p.stdout[-4000:]


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import rails_amd

    context = rails_amd.Context(device=0, seed=5)
    check_row(rails_amd, context, json.loads(sys.argv[1]))
    context.close()
    print("ROW PASSED")
