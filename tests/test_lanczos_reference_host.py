"""The step-local Lanczos reference of tests/lanczos_reference.py, checked on the host (no GPU): a correct fp64 implementation of the
kernel's algorithm (emulate) stays within a quarter of every derived bound on every case of its list, agrees with the oracle's
recurrence, and each of seven seeded mistakes exceeds a bound at least tenfold."""
import numpy as np
import pytest

import lanczos_reference as R

_runs = {}


def _q0(oracle, m, seed, stream):
    return oracle.random(m, 1, mode=1, seed=seed, stream=stream)[:, 0]


def _run(oracle, c):
    key = R.case_id(c)
    if key not in _runs:
        parts = R.make_case(c)
        out = R.emulate(parts["AV"], parts["MV"], parts["B"], parts["T"], _q0(oracle, c["m"], c["seed"], c["stream"]), c["L"])
        _runs[key] = (parts, out)
    return _runs[key]


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_emulation_stays_within_a_quarter_of_every_bound(oracle, c):
    parts, out = _run(oracle, c)
    worst = R.check_run(parts, c["L"], out["H"], out["steps"], out["Q"])
    print("%s: steps %d, error / bound: alpha %.3g, beta %.3g, r %.3g, norm %.3g" % (R.case_id(c), out["steps"], worst["alpha"], worst["beta"],
                                                                                 worst["r"], worst["norm"]))
    R.assert_within(worst, 0.25, R.case_id(c))


@pytest.mark.parametrize("c", [c for c in R.CASES if c["L"] <= 2 * c["k"] + c["p"]], ids=R.case_id)
def test_emulation_agrees_with_the_oracle(oracle, c):
    """the restated recurrence is the oracle's: H to the project's 1e-9 max|H| (tests/test_gpu_kernels.py)"""
    parts, out = _run(oracle, c)
    ref = oracle.resid_lanczos(parts["AV"], parts["MV"], parts["T"], parts["B"], c["L"], rng_mode=1, seed=c["seed"], stream=c["stream"])
    assert out["steps"] == ref["steps"]
    np.testing.assert_allclose(out["H"], ref["H"], rtol=0, atol=1e-9 * np.abs(ref["H"]).max())


@pytest.mark.parametrize("bug", R.BUGS)
def test_bounds_catch_a_seeded_mistake(oracle, bug):
    """the mistake seeded into emulate exceeds a bound by at least 10x on at least one case"""
    best = 0.0
    for c in R.CASES:
        if c["group"] == "grid_stride":
            continue  # large, and it takes no path of the emulation the smaller cases do not take
        parts, _ = _run(oracle, c)
        out = R.emulate(parts["AV"], parts["MV"], parts["B"], parts["T"], _q0(oracle, c["m"], c["seed"], c["stream"]), c["L"], bug=bug)
        worst = R.check_run(parts, c["L"], out["H"], out["steps"], out["Q"])
        best = max(best, max(worst.values()))
        if best >= 10.0:
            break
    print("%s: error / bound up to %.3g" % (bug, best))
    assert best >= 10.0, (bug, best)


@pytest.mark.parametrize("which", ["zero", "tiny", "second"])
def test_determined_breakdowns(oracle, which):
    """where a run stops and what H holds is fixed on the three rank-deficient cases; the emulation meets it, and the margins are
    there: beta_0 of "second" is above 1e-12 in longdouble, beta_1 far below the threshold"""
    bp = R.breakdown_parts(which)
    m = R.BREAKDOWN_M
    q0 = _q0(oracle, m, bp["seed"], bp["stream"])
    L = 4
    out = R.emulate(bp["AV"], bp["MV"], bp["B"], bp["T"], q0, L)
    H = out["H"]
    worst = R.check_run(bp, L, H, out["steps"], out["Q"])
    R.assert_within(worst, 0.25, which)
    if which == "zero":
        assert out["steps"] == 1 and not H.any()
    elif which == "tiny":
        assert out["steps"] == 1
        j = R.BREAKDOWN_ROW
        want = 2.0 ** -60 * q0[j] ** 2 / (q0 @ q0)
        assert abs(H[0, 0] - want) <= 8 * R.EPS * want and H[0, 0] > 0
        H[0, 0] = 0.0
        assert not H.any()
    else:
        ql = q0.astype(R.LD) / np.sqrt(q0.astype(R.LD) @ q0.astype(R.LD))
        b = bp["B"][:, 0].astype(R.LD)
        r = b * (b @ ql) - (b @ ql) ** 2 * ql
        beta0 = np.sqrt(r @ r)
        assert 1e-12 < beta0 < 2.0 ** -30
        assert out["steps"] == 2
        assert H[1, 0] == H[0, 1] and abs(H[1, 0] - beta0) <= 1e-6 * beta0
        assert H[2, 1] == 0.0 and H[1, 2] == 0.0
        H[:2, :2] = 0.0
        assert not H.any()
