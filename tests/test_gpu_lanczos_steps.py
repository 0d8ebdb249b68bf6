"""The fused residual Lanczos (rails_amd/csrc/lanczos.hip) checked ONE STEP AT A TIME from the device's own stored vectors against a
longdouble reference with derived componentwise bounds (tests/lanczos_reference.py: derivation, case list, and the host test that shows
the bounds are neither too tight for a correct fp64 implementation nor blind to seeded mistakes).  Every case keeps NaN in every panel
column outside the three windows.

Measured error / bound on an MI355X: see DESIGN.md, "Step-local Lanczos bounds"."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import lanczos_reference as R
import lanczos_steps_device as D

pytestmark = pytest.mark.gpu

LD = R.LD


@pytest.fixture(scope="module")
def ctx():
    import rails_amd

    c = rails_amd.Context(device=0, seed=1234)
    yield c
    c.close()


def MV(ctx, data=None, **kw):
    import rails_amd

    return rails_amd.HipMultiVectorWrapper(ctx, data=data, **kw)


def _nan_panel(ctx, m, cap=16):
    return MV(ctx, data=np.full((m, cap), np.nan), capacity=cap)


def _counters(ctx):
    s = ctx.stats()
    seed, nxt = C.c_uint64(0), C.c_uint64(0)
    ctx.lib.rails_ctx_rng_state(ctx.h, C.byref(seed), C.byref(nxt))
    return s["lanczos"], s["lanczos_start"], nxt.value


@pytest.mark.parametrize("c", [c for c in R.CASES if c["group"] in ("windows", "tiny", "empty", "past_rank")], ids=R.case_id)
def test_every_step_is_within_its_bounds(ctx, c):
    out = D.run_case(ctx, c)
    assert out["steps"] <= c["L"]
    assert out["launch"][:2] == D.expected_kernel(c["k"])


def test_grid_stride_loop_makes_a_second_trip(ctx):
    (c,) = R.cases("grid_stride")
    out = D.run_case(ctx, c)
    nch, unroll, nblocks = out["launch"]
    mpad = (c["m"] + 63) // 64 * 64
    assert (mpad + 63) // 64 > 4 * nblocks, (mpad // 64, nblocks)  # more row groups than waves in the grid: every wave's loop wraps
    assert out["steps"] == c["L"]


def _launched(ctx, c):
    """the launch rails_lanczos_last_launch reports after one run of a case (the run's results are other tests' business)"""
    parts = R.make_case(c)
    AV, MVw, B = D.upload(ctx, c, parts)
    ctx.set_seed(c["seed"], c["stream"])
    rc, _, steps = D.call(ctx, AV, MVw, B, parts["T"], c["L"])
    assert rc == 0 and 1 <= steps <= c["L"]
    return D.last_launch(ctx)


def test_grid_follows_the_plan_rule(ctx):
    """nblocks = max(1, min(ceil(ngroups / 4), num_cu * occ)) with ngroups = max(ceil(m / 64), 1) row groups and occ resident blocks per
    CU, 1..4 (rails_amd/csrc/lanczos_plan.h): one block up to four groups, two for five, and no more than are resident however many rows"""
    num_cu = ctx.lib.rails_ctx_num_cu(ctx.h)
    assert num_cu >= 1
    for c in R.cases("tiny"):  # m = 1, 63, 64, 65: one or two groups
        assert _launched(ctx, c)[2] == 1, R.case_id(c)
    five = dict(R.cases("tiny")[0], name="m300", m=300)  # 320 padded rows: five groups, the fifth in a second block
    assert _launched(ctx, five)[2] == 2
    (c,) = R.cases("grid_stride")  # 8196 groups: far more sets of four than blocks fit the device
    nblocks = _launched(ctx, c)[2]
    assert nblocks % num_cu == 0 and 1 <= nblocks // num_cu <= 4, (nblocks, num_cu)
    assert nblocks < (c["m"] + 63) // 64 // 4


def test_all_ten_instantiations_in_fresh_processes():
    """RAILS_LZ_UNROLL is read once per process: one child per U runs the "instantiations" cases (both ends of every NCH range), asserts
    the bounds and the kernel that was launched; the children run one after another and nothing is started after one that fails"""
    seen = set()
    helper = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lanczos_steps_device.py")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for u in (1, 2, 4):
        env = dict(os.environ, RAILS_LZ_UNROLL=str(u), PYTHONPATH=root)
        out = subprocess.run([sys.executable, helper, "instantiations"], env=env, capture_output=True, text=True, timeout=240, cwd=root)
        print(out.stdout)
        assert out.returncode == 0, "U = %d: exit status %d\n%s\n%s" % (u, out.returncode, out.stdout[-3000:], out.stderr[-3000:])
        got = set()
        for line in out.stdout.splitlines():
            if line.startswith("LAUNCH "):
                nch, unroll = int(line.split()[1]), int(line.split()[2])
                got.add((nch, unroll))
        want = {(n, u) for n in (1, 2)} | {(n, min(u, 2)) for n in (3, 4)}
        assert got == want, (u, got, want)  # with U = 4, NCH >= 3 reports unroll 2
        seen |= got
    assert seen == {(1, 1), (1, 2), (1, 4), (2, 1), (2, 2), (2, 4), (3, 1), (3, 2), (4, 1), (4, 2)}


def _start_case():
    c = dict(R.cases("windows")[0], m=741)  # layout (1): AV at [2, 39), MV at [40, 77) of one 80-column panel, B at [6, 9) of 16
    c["seed"], c["stream"] = 77, 5
    return c, R.make_case(c)


def test_lanczos_start_sums_vector_counter_and_stream(ctx, oracle):
    import rails_amd
    from rails_amd._lib import check

    c, parts = _start_case()
    m, k, p = c["m"], c["k"], c["p"]
    AV, MVw, B = D.upload(ctx, c, parts)
    ctx.set_seed(c["seed"], c["stream"])
    before = ctx.stats()["lanczos_start"]
    sums = np.full(2 * k + p + 1, np.nan)
    check(ctx.lib.rails_lanczos_start(ctx.h, AV.panel.h, AV.c0, MVw.panel.h, MVw.c0, k, B.panel.h, B.c0, p, D._ptr(sums)), "rails_lanczos_start")
    assert ctx.stats()["lanczos_start"] == before + 1
    q0 = oracle.random(m, 1, mode=1, seed=c["seed"], stream=c["stream"])[:, 0]
    P = np.hstack([parts["AV"], parts["MV"], parts["B"], q0[:, None]]).astype(LD)
    want = P.T @ q0.astype(LD)
    bound = R.gamma(m + 4) * (np.abs(P).T @ np.abs(q0).astype(LD))
    ratio = np.abs(sums.astype(LD) - want) / bound
    print("lanczos_start: max |err| / bound = %.3g" % float(ratio.max()))
    assert np.all(ratio <= 1.0), float(ratio.max())
    # the raw q0 is Lanczos vector 0
    out = MV(ctx, m=m, n=1, capacity=16)
    rails_amd.lanczos_vectors(ctx, np.array([[1.0]]), out)
    assert np.array_equal(out.to_host()[:, 0], q0)
    # E = q0 * gamma (rails/HipSolverOps.hpp: the start of the coefficient-space recurrence): steps = 1, lds = 1, w = 5
    gam = np.random.default_rng(3).uniform(-1, 1, (1, 5))
    E = MV(ctx, m=m, n=5, capacity=16)
    rails_amd.lanczos_vectors(ctx, gam, E)
    assert np.array_equal(E.to_host(), q0[:, None] * gam)
    assert D.last_launch(ctx)[0] == 1
    # one stream was consumed: the next draw is the oracle's next stream
    v = MV(ctx, m=m, n=1, capacity=16)
    v.random()
    assert np.array_equal(v.to_host(), oracle.random(m, 1, mode=1, seed=c["seed"], stream=c["stream"] + 1))


def test_lanczos_vectors_chunks_offsets_and_leading_dimension(ctx):
    from rails_amd._lib import check

    m, k, p, steps = 1000, 6, 3, 7  # 1000 rows: not a multiple of the 256-row blocks
    rng = np.random.default_rng(11)
    AVh, MVh, Bh, T = R.problem(m, k, p, rng)
    parts = dict(AV=AVh, MV=MVh, B=Bh, T=T)
    out = D.run_parts(ctx, (MV(ctx, AVh, capacity=16), MV(ctx, MVh, capacity=16), MV(ctx, Bh, capacity=16)), parts, steps, 5, 9)
    R.assert_within(out["worst"], 1.0, "vectors")
    assert out["steps"] == steps
    Q = out["Q"].astype(LD)
    sentinel = -7.25
    worst = 0.0
    for w in (1, 16, 17, 33):
        S = np.asfortranarray(np.full((steps + 3, w), np.nan))  # leading dimension steps + 3; the rows below S are never read
        S[:steps] = rng.uniform(-1, 1, (steps, w))
        want = Q @ S[:steps].astype(LD)
        bound = R.gamma(steps) * (np.abs(Q) @ np.abs(S[:steps]).astype(LD))
        for oc0 in (0, 3, 16):
            O = MV(ctx, data=np.full((m, 64), sentinel), capacity=64)
            check(ctx.lib.rails_lanczos_vectors(ctx.h, D._ptr(S), steps + 3, w, O.panel.h, oc0), "rails_lanczos_vectors")
            got = O.to_host()
            err = np.abs(got[:, oc0:oc0 + w].astype(LD) - want)
            assert np.all(err <= bound), (w, oc0, float((err / bound).max()))
            worst = max(worst, float((err / bound).max()))
            outside = np.ones(64, dtype=bool)
            outside[oc0:oc0 + w] = False
            assert np.all(got[:, outside] == sentinel), (w, oc0)
    print("lanczos_vectors: max |err| / bound = %.3g" % worst)


@pytest.mark.parametrize("which", ["zero", "tiny", "second"])
def test_breakdown_is_determined(ctx, oracle, which):
    """k = 0, p = 1, R = B B': where the run stops, what H holds and how many rows of S lanczos_vectors then takes are fixed"""
    bp = R.breakdown_parts(which)
    m, L = R.BREAKDOWN_M, 4
    Bpanel = np.full((m, 16), np.nan)
    Bpanel[:, 0] = bp["B"][:, 0]
    windows = (_nan_panel(ctx, m)._alias(0, 0, True), _nan_panel(ctx, m)._alias(0, 0, True), MV(ctx, data=Bpanel, capacity=16)._alias(0, 1, True))
    out = D.run_parts(ctx, windows, bp, L, bp["seed"], bp["stream"])
    R.assert_within(out["worst"], 1.0, which)
    H, steps = out["H"].copy(), out["steps"]
    q0 = oracle.random(m, 1, mode=1, seed=bp["seed"], stream=bp["stream"])[:, 0]
    if which == "zero":
        assert steps == 1 and not H.any()
    elif which == "tiny":
        assert steps == 1
        ref = R.step_local(bp["AV"], bp["MV"], bp["B"], bp["T"], out["Q"], [H[0, 0]], [])[0]
        want = LD(2.0 ** -60) * LD(q0[R.BREAKDOWN_ROW]) ** 2 / (q0.astype(LD) @ q0.astype(LD))
        assert abs(LD(H[0, 0]) - want) <= ref["ea"] and H[0, 0] > 0
        H[0, 0] = 0.0
        assert not H.any()  # no off-diagonal entry was written
    else:
        assert steps == 2
        ref = R.step_local(bp["AV"], bp["MV"], bp["B"], bp["T"], out["Q"], [H[0, 0], H[1, 1]], [H[1, 0]])
        assert H[1, 0] == H[0, 1] and abs(LD(H[1, 0]) - ref[0]["beta_ref"]) <= ref[0]["eb"] and H[1, 0] > 1e-12
        assert H[2, 1] == 0.0 and H[1, 2] == 0.0
        H[:2, :2] = 0.0
        assert not H.any()
    # lanczos_vectors takes exactly `steps` rows of S afterwards
    O = MV(ctx, m=m, n=1, capacity=16)
    S = np.asfortranarray(np.ones((steps, 1)))
    assert ctx.lib.rails_lanczos_vectors(ctx.h, D._ptr(S), steps, 1, O.panel.h, 0) == 0
    assert ctx.lib.rails_lanczos_vectors(ctx.h, D._ptr(S), steps - 1, 1, O.panel.h, 0) != 0
    rowsum = out["Q"].astype(LD).sum(axis=1)  # what the accepted call wrote; the refused one wrote nothing
    assert np.all(np.abs(O.to_host()[:, 0].astype(LD) - rowsum) <= R.gamma(steps) * np.abs(out["Q"]).sum(axis=1))


def test_state_reuse_and_determinism_on_one_context():
    """one context: a run, a shorter one that reuses the vector buffer with a smaller padded length, a longer one that reallocates it;
    then the first again from the same seed and stream: the reductions have a fixed order, so H and Q come back bit for bit"""
    import rails_amd

    ctx = rails_amd.Context(device=0, seed=1)
    try:
        k, p = 12, 4
        runs = []
        for i, (m, L) in enumerate(((5000, 12), (100, 3), (5000, 20))):
            AVh, MVh, Bh, T = R.problem(m, k, p, np.random.default_rng(50 + i))
            parts = dict(AV=AVh, MV=MVh, B=Bh, T=T)
            windows = (MV(ctx, AVh, capacity=16), MV(ctx, MVh, capacity=16), MV(ctx, Bh, capacity=16))
            out = D.run_parts(ctx, windows, parts, L, 900 + i, 3)
            print("m = %d, L = %d: %r" % (m, L, out["worst"]))
            R.assert_within(out["worst"], 1.0, "run %d" % i)
            assert out["steps"] == L
            runs.append((windows, parts, L, out))
        windows, parts, L, first = runs[0]
        again = D.run_parts(ctx, windows, parts, L, 900, 3)
        assert again["steps"] == first["steps"]
        assert np.array_equal(again["H"], first["H"])
        assert np.array_equal(again["Q"], first["Q"])
    finally:
        ctx.close()


def test_refusals_launch_nothing(ctx):
    import rails_amd

    lib = ctx.lib
    m, k, p, L = 40, 4, 2, 3
    AVh, MVh, Bh, T = R.problem(m, k, p, np.random.default_rng(0))
    AV, MVw, B = MV(ctx, AVh, capacity=16), MV(ctx, MVh, capacity=16), MV(ctx, Bh, capacity=16)
    rc, _, _ = D.call(ctx, AV, MVw, B, T, L)  # the valid call these are variations of
    assert rc == 0
    before = _counters(ctx)

    def refused(text, **kw):
        windows = kw.pop("windows", (AV, MVw, B))
        rc, H, steps = D.call(ctx, windows[0], windows[1], windows[2], T, kw.pop("L", L), **kw)
        assert rc != 0 and text in lib.rails_last_error().decode(), (kw, rc, lib.rails_last_error())
        assert np.isnan(H).all() and steps == -1  # nothing was written back
        assert _counters(ctx) == before  # no run counted, no RNG stream consumed

    refused("even columns", avc0=1)
    refused("even columns", mvc0=3)
    refused("even columns", bc0=1)
    wide = (MV(ctx, m=8, n=4, capacity=528), MV(ctx, m=8, n=4, capacity=528), MV(ctx, m=8, n=2, capacity=144))
    refused("k <= 512", windows=wide, k=513)
    refused("k <= 512", windows=wide, p=129)
    refused("bad sizes", L=0, ldh=4)
    refused("bad sizes", ldh=L)
    refused("row mismatch", windows=(AV, MV(ctx, m=m + 1, n=k, capacity=16), B))
    refused("row mismatch", windows=(AV, MVw, MV(ctx, m=m - 1, n=p, capacity=16)))
    # rails_lanczos_vectors: a row-mismatched output, and a context that has not run Lanczos
    S = np.asfortranarray(np.eye(L))
    assert lib.rails_lanczos_vectors(ctx.h, D._ptr(S), L, L, MV(ctx, m=m + 1, n=L, capacity=16).panel.h, 0) != 0
    assert "row mismatch" in lib.rails_last_error().decode()
    fresh = rails_amd.Context(device=0, seed=1)
    try:
        O = MV(fresh, data=np.full((m, 16), 3.0), capacity=16)
        assert lib.rails_lanczos_vectors(fresh.h, D._ptr(S), L, L, O.panel.h, 0) != 0
        assert "no Lanczos run" in lib.rails_last_error().decode()
        assert np.all(O.to_host() == 3.0)
        nch = C.c_int(0)
        assert lib.rails_lanczos_last_launch(fresh.h, C.byref(nch), C.byref(nch), C.byref(nch)) != 0
    finally:
        fresh.close()
