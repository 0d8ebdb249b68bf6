"""The case lists and bounds of tests/solution_reference.py, checked without a GPU: the k list reaches every instantiation of
k_panel_rowquad<TR> and every slice pair with two different TRs that the slice rule can produce, the exact cases are exact by
construction, and numpy in plain double stays inside every bound the GPU tests hold the device to (so the bounds can be met)."""
import ctypes as C
import os
import re

import numpy as np

import solution_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slice_rule_against_the_source():
    """the restated rule reads as rails_panel_rowquad's: the same three expressions are in solution.hip"""
    src = open(os.path.join(ROOT, "rails_amd", "csrc", "solution.hip")).read()
    assert "const int nslices = (k + 255) / 256, width = ((k + nslices - 1) / nslices + 15) / 16 * 16;" in src
    assert "const int nc = std::min(width, k - j0), tiles = (nc + 15) / 16" in src
    assert re.findall(r"tiles <= (\d+)\)\s*RAILS_TRY\(\(launch_rowquad<(\d+)>", src) == [("2", "2"), ("4", "4"), ("8", "8"), ("12", "12")]
    assert "launch_rowquad<16>" in src
    for k in range(0, 513):
        sl = R.slice_rule(k)
        assert len(sl) == (k + 255) // 256
        assert sum(nc for _, nc, _ in sl) == k and all(nc <= 16 * tr and tr in R.TRS for _, nc, tr in sl)
        assert [j0 for j0, _, _ in sl] == [q * sl[0][1] for q in range(len(sl))]


def test_k_list_reaches_every_instantiation_and_every_mixed_pair():
    ks = R.K_LIST
    assert set(ks) >= {0, 1, 3, 4, 5, 31, 32, 33, 64, 128, 129, 192, 193, 256, 257, 270, 300, 384, 385, 512}
    assert {tr for k in ks for _, _, tr in R.slice_rule(k)} == set(R.TRS)
    assert {R.slice_rule(k)[0][2] for k in ks if len(R.slice_rule(k)) == 1} == set(R.TRS)  # each one also in a launch that does not accumulate
    assert R.slice_rule(257) == [(0, 144, 12), (144, 113, 8)]
    assert R.slice_rule(256) == [(0, 256, 16)] and R.slice_rule(512) == [(0, 256, 16), (256, 256, 16)]
    # The first slice is never narrower than the second, so a pair (TR, larger TR) cannot occur; of the pairs with two different TRs
    # the rule produces exactly these two over all k <= 512, and the list holds both
    possible = {tuple(tr for _, _, tr in R.slice_rule(k)) for k in range(257, 513)}
    mixed = {p for p in possible if p[0] != p[1]}
    assert mixed == {(12, 8), (16, 12)}
    have = {tuple(tr for _, _, tr in R.slice_rule(k)) for k in ks if k > 256}
    assert mixed <= have and {(12, 12), (16, 16)} <= have
    assert all(k in ks for k in R.STALE_SEQUENCE if k != 500) and len(R.slice_rule(500)) == 2
    for k in R.SINGLE_ENTRY_K:
        pairs = R.single_entry_pairs(k)
        assert all(0 <= a < k and 0 <= b < k for a, b in pairs) and len(set(pairs)) == len(pairs)
        for _, nc, _ in R.slice_rule(k)[:-1]:
            assert (nc - 1, nc) in pairs and (nc, nc - 1) in pairs  # either side of the slice edge


def test_exact_cases_are_exact():
    assert max(R.exact_partial_sum_limit(k) for k in R.K_LIST) == 512 * 3 * 512 * 9 < 2 ** 53
    n = 0
    for k in R.K_LIST:
        assert set(R.exact_ms(k)) == (set(R.M_LIST) if k <= R.K_SMALL_MAX else {129, 300})
        for m in R.exact_ms(k):
            U, S, want = R.exact_case(m, k)
            n += 1
            assert U.shape == (m, k) and S.shape == (k, k) and want.dtype == np.int64
            assert np.array_equal(U, np.rint(U)) and np.array_equal(S, np.rint(S))
            assert (np.abs(U).max(initial=0) <= 3) and (np.abs(S).max(initial=0) <= 3)
            assert k < 2 or not np.array_equal(S, S.T)
            assert np.abs(want).max(initial=0) <= R.exact_partial_sum_limit(k)
            # numpy in double, whatever its order of summation, gives the integers
            assert np.array_equal(R.rowquad_double(U, S), want.astype(np.float64))
            if m <= 129:  # ... and so does the longdouble reference
                assert np.array_equal(np.asarray(R.rowquad(U, S), dtype=np.float64), want.astype(np.float64))
    assert n == 9 * 8 + 11 * 2


def test_double_stays_inside_the_kernel_bound():
    for k in R.K_LIST:
        U, S, want, bound = R.bounded_case(R.BOUNDED_M, k)
        err = np.abs(np.asarray(R.rowquad_double(U, S) - want, dtype=np.float64))
        assert np.all(err <= bound), k
        if k:
            assert bound.min() > 0
            assert np.log10(np.abs(U).max(axis=1).max() / np.abs(U).max(axis=1).min()) > (4 if k > 1 else 3)  # rows over decades
    for m, k in R.WINDOW_CASES:
        U, S, want, bound = R.bounded_case(m, k)
        assert np.all(np.abs(np.asarray(R.rowquad_double(U, S) - want, dtype=np.float64)) <= bound)


def test_double_stays_inside_the_object_bounds():
    U, S = R.object_problem()
    m, k = U.shape
    assert (m, k) == (300, 40) and 0.9e2 < np.linalg.cond(U) < 1.1e2 and np.array_equal(S, S.T)
    assert np.all(np.abs(np.asarray(R.rowquad_double(U, S) - R.rowquad(U, S), dtype=np.float64)) <= R.rowquad_bound(U, S))
    assert abs(float(R.trace_double(U, S) - R.trace(U, S))) <= R.trace_bound(U, S)
    for nc in R.APPLY_NC:
        W = R.apply_rhs(m, nc)
        assert np.all(np.abs(np.asarray(R.apply_double(U, S, W) - R.apply(U, S, W), dtype=np.float64)) <= R.apply_bound(U, S, W)), nc
    for rows, cols in R.block_cases(m):
        err = np.abs(np.asarray(R.block_double(U, S, rows, cols) - R.block(U, S, rows, cols), dtype=np.float64))
        assert err.shape == (len(rows), len(cols)) and np.all(err <= R.block_bound(U, S, rows, cols))
    # the derived bound is far below the object-level one of test_object_against_dense_numpy (which grows with m on top)
    old = m * k * k * R.EPS * np.abs(U).max() ** 2 * np.abs(S).max()
    assert R.rowquad_bound(U, S).max() < old / 10


def test_longdouble_is_wider_than_double():
    """the references need a format that is more precise than the one under test"""
    assert np.finfo(R.LD).eps <= 2.0 ** -63


def test_special_data_holds_every_kind():
    X = R.special_data(np.random.default_rng(0), 17, 15)
    u = R.bits(X)
    assert X.shape == (17, 15) and X.flags.f_contiguous
    assert (u == 0x8000000000000000).any() and np.isposinf(X).any() and np.isneginf(X).any()
    nan = u[np.isnan(X)]
    assert nan.size >= 4 and np.unique(nan).size == nan.size and (nan >> 63).any() and not (nan >> 63).all()
    sub = (u & 0x7FF0000000000000 == 0) & (u & 0x000FFFFFFFFFFFFF != 0)
    assert sub.any()
    assert R.special_data(np.random.default_rng(1), 1, 1).shape == (1, 1)


def test_last_plan_is_declared_and_bound():
    import rails_amd
    from rails_amd import _solution_sigs as Sg

    text = open(os.path.join(ROOT, "include", "rails_solution.h")).read()
    assert re.search(r"\bint\s+rails_panel_rowquad_last_plan\s*\(\s*const\s+rails_ctx\s*\*\s*ctx\s*,\s*int\s*\*\s*nslices\s*,\s*int\s*\*\s*tr\s*,\s*int\s+cap\s*\)\s*;", text)
    ip = C.POINTER(C.c_int)
    assert Sg.SOLUTION_SIGNATURES["rails_panel_rowquad_last_plan"] == (C.c_int, [C.c_void_p, ip, ip, C.c_int])
    lib = rails_amd.load()
    assert lib.rails_panel_rowquad_last_plan(None, None, None, 0) != 0 and b"null argument" in lib.rails_last_error()
