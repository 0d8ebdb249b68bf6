"""The host part of the sparse right-hand side, no GPU: rails_csr_transpose_host and rails_csr_gram_norm2_host of librails_hip.so against
scipy and numpy, the same checks in a stand-alone program (tests/cpp/sparse_rhs_host.cpp, linked against sprhs_host.o alone), and the
numpy emulation of rails_resid_lanczos_sparse's step order (tests/sparse_rhs_reference.py) against the step-local bounds of
tests/lanczos_reference.py: a quarter of every bound on every case, and five seeded mistakes that each exceed a bound tenfold."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import lanczos_reference as R
import sparse_rhs_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rails_amd", "lib", "sparse_rhs_host")
RAILS_EINVAL = -1


def _host():
    from rails_amd import sparse_rhs

    return sparse_rhs


def _raw(m, p, rows):
    """CSR with the entries exactly as given (unsorted columns, duplicates): rows = list of lists of (col, val)"""
    rowptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    col = np.array([c for r in rows for c, _ in r], dtype=np.int32)
    val = np.array([v for r in rows for _, v in r], dtype=np.float64)
    return sp.csr_matrix((val, col, rowptr), shape=(m, p))


def _matrices():
    rng = np.random.default_rng(3)
    out = {"tall": S.make_B("random3", 300, 40), "wide": S.make_B("random3", 40, 300), "mixed": S.make_B("mixed", 741, 300, lanczos=True),
           "selection": S.make_B("selection", 330, 200), "nnz0": sp.csr_matrix((20, 7)), "p0": sp.csr_matrix((9, 0)),
           "m0": sp.csr_matrix((0, 5))}
    E = sp.random(257, 65, density=0.05, format="lil", random_state=rng)
    E[3::4, :] = 0.0  # empty rows
    E[:, 2::5] = 0.0  # empty columns
    E = sp.csr_matrix(E)
    E.eliminate_zeros()
    out["empty_rows_cols"] = E
    out["duplicates"] = _raw(4, 4, [[(2, 1.0), (2, -3.0), (0, 0.5), (2, 7.0)], [], [(3, 2.0), (2, 4.0), (2, -5.0), (0, 1.5), (0, 2.5)], [(1, 9.0), (1, -9.5)]])
    return out


MATS = _matrices()


@pytest.mark.parametrize("name", sorted(MATS))
def test_transpose_is_scipys_and_stable(name):
    B = MATS[name]
    m, p = B.shape
    rc, tp, tc, tv = _host().csr_transpose_host(m, p, *S.csr_arrays(B))
    assert rc == 0
    want = sp.csr_matrix((B.data, B.indices, B.indptr), shape=B.shape).T.tocsr()  # a stable counting sort: nothing is summed or sorted
    assert np.array_equal(tp, want.indptr) and np.array_equal(tc, want.indices) and np.array_equal(tv, want.data)
    assert all(np.all(np.diff(tc[tp[j]:tp[j + 1]]) >= 0) for j in range(p))  # increasing original row inside a transposed row
    if name == "duplicates":  # column 2: rows 0, 0, 0, 2, 2 with the values in the order they were given
        assert list(tc[tp[2]:tp[3]]) == [0, 0, 0, 2, 2] and list(tv[tp[2]:tp[3]]) == [1.0, -3.0, 7.0, 4.0, -5.0]


@pytest.mark.parametrize("name", sorted(MATS))
def test_gram_norm_matches_numpy(name):
    B = MATS[name]
    m, p = B.shape
    rc, tp, tc, tv = _host().csr_transpose_host(m, p, *S.csr_arrays(B))
    assert rc == 0
    rc, got = _host().csr_gram_norm2_host(m, p, S.csr_arrays(B), (tp, tc, tv))
    assert rc == 0
    D = B.toarray().astype(np.longdouble)
    want = float(np.sum((D.T @ D) ** 2))
    assert abs(got - want) <= 1e-13 * want, (got, want)


def test_bad_input_is_refused_not_read():
    import rails_amd

    h = _host()
    B = MATS["tall"]
    m, p = B.shape
    rowptr, col, val = S.csr_arrays(B)
    good_t = h.csr_transpose_host(m, p, rowptr, col, val)[1:]
    for bad in (p, -1, 2 ** 31 - 1):
        c2 = col.copy()
        c2[17] = bad
        assert h.csr_transpose_host(m, p, rowptr, c2, val)[0] == RAILS_EINVAL
        assert "out of range" in rails_amd.load().rails_last_error().decode()
        assert h.csr_gram_norm2_host(m, p, (rowptr, c2, val), good_t)[0] == RAILS_EINVAL
    r2 = rowptr.copy()
    r2[20] = r2[19] - 1
    assert h.csr_transpose_host(m, p, r2, col, val)[0] == RAILS_EINVAL
    assert "monotone" in rails_amd.load().rails_last_error().decode()
    assert h.csr_gram_norm2_host(m, p, (r2, col, val), good_t)[0] == RAILS_EINVAL
    r3 = rowptr.copy()
    r3[0] = 1
    assert h.csr_transpose_host(m, p, r3, col, val)[0] == RAILS_EINVAL
    # a transposed form that is not one of this matrix
    assert h.csr_gram_norm2_host(m, p, (rowptr, col, val), (np.zeros(p + 1, dtype=np.int64), good_t[1][:0], good_t[2][:0]))[0] == RAILS_EINVAL


def test_stand_alone_program():
    if not os.path.exists(EXE):
        import rails_amd.build

        rails_amd.build.build()
    p = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0 and "ALL PASSED" in p.stdout, p.stdout[-4000:]
    assert [ln.split()[1] for ln in p.stdout.splitlines() if ln.startswith("PASS ")] == [
        "tall", "wide", "empty_rows_cols", "nnz0", "p0", "duplicates", "dense_row_and_column", "column_out_of_range", "column_negative",
        "rowptr_not_monotone", "rowptr_not_from_zero"]


# ------------------------------------------------------------------------------------------------------- the Lanczos emulation
_runs = {}


def _q0(oracle, c):
    return oracle.random(c["m"], 1, mode=1, seed=c["seed"], stream=c["stream"])[:, 0]


def _run(oracle, c, bug=None):
    key = (S.case_id(c), bug)
    if key not in _runs:
        if (S.case_id(c), "parts") not in _runs:
            _runs[(S.case_id(c), "parts")] = S.make_case(c)
        parts = _runs[(S.case_id(c), "parts")]
        _runs[key] = (parts, S.emulate(parts["AV"], parts["MV"], parts["Bs"], parts["T"], _q0(oracle, c), c["L"], bug=bug))
    return _runs[key]


def test_the_cases_hold_what_they_are_there_for():
    by = {S.case_id(c): S.make_case(c)["Bs"] for c in S.CASES}
    mixed = by["m741_k129_p300_mixed_L4"]
    lens = np.diff(mixed.indptr)
    assert lens.max() == 299 > 64 and not lens[:70].any() and np.diff(mixed.T.tocsr().indptr)[298] == 0  # a dense row, an empty group, an empty column
    assert np.diff(mixed.T.tocsr().indptr)[0] > S.CHUNK and np.diff(mixed.T.tocsr().indptr)[299] > 0  # a long transposed row in two items
    assert by["m64_k2_p3_mixed_L2"].nnz == 0 and by["m200_k4_p0_none_L3"].shape == (200, 0)
    assert by["m330_k37_p200_selection_L5"].nnz == 200 and by["m63_k2_p130_random3_L2"].shape == (63, 130)


@pytest.mark.parametrize("c", S.CASES, ids=S.case_id)
def test_emulation_stays_within_a_quarter_of_every_bound(oracle, c):
    parts, out = _run(oracle, c)
    worst = R.check_run(parts, c["L"], out["H"], out["steps"], out["Q"])
    print("%s: steps %d, error / bound: alpha %.3g, beta %.3g, r %.3g, norm %.3g" % (S.case_id(c), out["steps"], worst["alpha"], worst["beta"],
                                                                                 worst["r"], worst["norm"]))
    R.assert_within(worst, 0.25, S.case_id(c))


@pytest.mark.parametrize("c", [c for c in S.CASES if c["p"] <= 16 and c["L"] <= 2 * c["k"] + c["p"]], ids=S.case_id)
def test_emulation_agrees_with_the_dense_one(oracle, c):
    """the same recurrence as the dense form's emulation on B.toarray(): H to the project's 1e-9 max|H|"""
    parts, out = _run(oracle, c)
    ref = R.emulate(parts["AV"], parts["MV"], parts["B"], parts["T"], _q0(oracle, c), c["L"])
    assert out["steps"] == ref["steps"]
    np.testing.assert_allclose(out["H"], ref["H"], rtol=0, atol=1e-9 * max(np.abs(ref["H"]).max(), 1e-300))


@pytest.mark.parametrize("bug", S.BUGS)
def test_bounds_catch_a_seeded_mistake(oracle, bug):
    """each mistake seeded into the emulation exceeds a bound at least tenfold on the case made for it"""
    (c,) = [c for c in S.CASES if S.case_id(c) == "m741_k129_p300_mixed_L4"]
    parts, out = _run(oracle, c, bug=bug)
    worst = R.check_run(parts, c["L"], out["H"], out["steps"], out["Q"])
    print("%s: error / bound up to %.3g" % (bug, max(worst.values())))
    assert max(worst.values()) >= 10.0, (bug, worst)


@pytest.mark.parametrize("name", ["m741_k129_p300_mixed_L4", "m330_k37_p200_selection_L5", "m200_k0_p260_random3_L3"])
def test_the_reference_without_a_dense_B_is_the_same_reference(oracle, name):
    """step_local_sparse (for the grid-stride case of the device test, whose dense B would not fit) gives check_run's ratios, up to the
    two longdouble references' own rounding (1e-8 of a bound)"""
    (c,) = [c for c in S.CASES if S.case_id(c) == name]
    parts, out = _run(oracle, c)
    a = R.check_run(parts, c["L"], out["H"], out["steps"], out["Q"])
    b = S.check_run_sparse(parts, c["L"], out["H"], out["steps"], out["Q"])
    for key in a:
        assert abs(a[key] - b[key]) <= 1e-6 * a[key] + 1e-8, (key, a, b)
