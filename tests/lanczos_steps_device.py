"""Runs cases of tests/lanczos_reference.py through rails_resid_lanczos on the device and checks them step by step.  Shared by
tests/test_gpu_lanczos_steps.py and, run as a program, the child process of its instantiation test:

    python tests/lanczos_steps_device.py GROUP

runs every case of GROUP on a fresh context, asserts the bounds and that the pass kernel rails_lanczos_last_launch reports is the one
RAILS_LZ_UNROLL (read once per process, hence the child) and k select, prints one "LAUNCH nch unroll nblocks case" line per case and
exits nonzero on any failure."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p_ in (ROOT, os.path.join(ROOT, "tests")):
    if _p_ not in sys.path:
        sys.path.insert(0, _p_)

import lanczos_reference as R  # noqa: E402


def _ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def upload(ctx, c, parts):
    """the NaN-filled panels of a case on the device; returns the three windows (HipMultiVectorWrapper views)"""
    import rails_amd

    dev = {}
    for pn, host in parts["panels"].items():
        d = rails_amd.HipMultiVectorWrapper(ctx, data=host, capacity=host.shape[1])
        assert ctx.lib.rails_panel_ld(d.panel.h) == host.shape[1] == d.panel.capacity
        dev[pn] = d
    return tuple(dev[pn]._alias(c0, w, True) for (pn, c0), w in ((c["av"], c["k"]), (c["mv"], c["k"]), (c["b"], c["p"])))


def call(ctx, AV, MV, B, T, L, ldh=None, avc0=None, mvc0=None, bc0=None, k=None, p=None):
    """rails_resid_lanczos as it is: returns (rc, H, steps); the optional arguments override what the windows say"""
    k = AV.n if k is None else k
    T = np.asfortranarray(np.asarray(T, dtype=np.float64).reshape(AV.n, AV.n))
    ldh = L + 1 if ldh is None else ldh
    H = np.full((max(ldh, 1), L + 1), np.nan, order="F")
    steps = C.c_int(-1)
    rc = ctx.lib.rails_resid_lanczos(ctx.h, AV.panel.h, AV.c0 if avc0 is None else avc0, MV.panel.h, MV.c0 if mvc0 is None else mvc0, k, _ptr(T),
                                     max(1, AV.n), B.panel.h, B.c0 if bc0 is None else bc0, B.n if p is None else p, L, _ptr(H), ldh,
                                     C.byref(steps))
    return rc, H, steps.value


def last_launch(ctx):
    from rails_amd._lib import check

    nch, unroll, nblocks = C.c_int(0), C.c_int(0), C.c_int(0)
    check(ctx.lib.rails_lanczos_last_launch(ctx.h, C.byref(nch), C.byref(unroll), C.byref(nblocks)), "rails_lanczos_last_launch")
    return nch.value, unroll.value, nblocks.value


def stored_vectors(ctx, m, steps):
    """Q = the stored Lanczos vectors (the product with the identity is exact)"""
    import rails_amd

    out = rails_amd.HipMultiVectorWrapper(ctx, m=m, n=steps, capacity=R.pad16(steps))
    rails_amd.lanczos_vectors(ctx, np.eye(steps), out)
    return out.to_host()


def run_parts(ctx, windows, parts, L, seed, stream):
    """one run from (seed, stream), checked against every bound; returns dict(H, steps, Q, launch, worst)"""
    from rails_amd._lib import check

    AV, MV, B = windows
    ctx.set_seed(seed, stream)
    rc, H, steps = call(ctx, AV, MV, B, parts["T"], L)
    check(rc, "rails_resid_lanczos")
    assert 1 <= steps <= L, steps
    assert not np.isnan(H).any()
    Q = stored_vectors(ctx, AV.M(), steps)
    worst = R.check_run(parts, L, H, steps, Q)
    return dict(H=H, steps=steps, Q=Q, launch=last_launch(ctx), worst=worst)


def run_case(ctx, c):
    parts = R.make_case(c)
    out = run_parts(ctx, upload(ctx, c, parts), parts, c["L"], c["seed"], c["stream"])
    w = out["worst"]
    print("%s: steps %d, <%d,%d> on %d blocks, error / bound: alpha %.3g, beta %.3g, r %.3g, norm %.3g" % (
        (R.case_id(c), out["steps"]) + out["launch"] + (w["alpha"], w["beta"], w["r"], w["norm"])))
    R.assert_within(w, 1.0, R.case_id(c))
    return out


def expected_kernel(k):
    """the pass kernel a run takes, stated here independently of rails_amd/csrc/lanczos_plan.h: NCH = ceil(k / 128) in 1..4, U from
    RAILS_LZ_UNROLL (default 4), at most 2 rows in flight for NCH >= 3"""
    nch = min(4, max(1, (k + 127) // 128))
    u = int(os.environ.get("RAILS_LZ_UNROLL", "4"))
    if u not in (1, 2, 4):
        u = 4
    return nch, (2 if nch >= 3 and u > 2 else u)


def main(argv):
    import rails_amd

    group = argv[1]
    ctx = rails_amd.Context(device=0, seed=1)
    try:
        for c in R.cases(group):
            out = run_case(ctx, c)
            nch, unroll, nblocks = out["launch"]
            assert (nch, unroll) == expected_kernel(c["k"]), (R.case_id(c), nch, unroll, expected_kernel(c["k"]))
            print("LAUNCH %d %d %d %s" % (nch, unroll, nblocks, R.case_id(c)))
    finally:
        ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
