"""The pair and map entries of the solution object without a GPU: tests/covariance_reference.py's restatement and bounds are consistent
and can be met (numpy in plain double stays inside them), the C++ fallback of rails::Solution (covariance, maps; element access, no
rowpair member) on the CPU back end agrees with it, and the new symbols are declared, exported and bound with the right ctypes, the
Python entry points validate their indices before any C call."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import covariance_reference as CR
import solution_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def test_patterns_cover_what_they_claim():
    for m in CR.PAIR_MS:
        for n in CR.pair_ns(m):
            for name in CR.PATTERNS:
                ia, ib, nn = CR.pattern(name, m, n)
                assert nn == (min(n, m) if name.endswith("_null") else n)
                for idx in (ia, ib):
                    assert idx is None or (idx.dtype == np.int32 and idx.size == nn and (nn == 0 or (idx.min() >= 0 and idx.max() < m)))
                assert (ia is None) == (name == "ia_null") and (ib is None) == (name == "ib_null")
        ia, ib, _ = CR.pattern("differ", m, 17)
        assert m == 1 or np.any(ia != ib)
        ia, _, _ = CR.pattern("last", m, 17)
        assert np.all(ia == m - 1)
    assert 2 * 129 in CR.pair_ns(129) and 0 in CR.pair_ns(129)


def test_exact_pairs_are_entries_of_the_dense_integer_solution():
    for m, k in ((17, 5), (129, 33), (128, 257)):
        U, S, _ = R.exact_case(m, k)
        X = U.astype(np.int64) @ S.astype(np.int64) @ U.astype(np.int64).T
        assert R.exact_partial_sum_limit(k) < 2 ** 53
        for name in CR.PATTERNS:
            ia, ib, n = CR.pattern(name, m, 2 * m)
            a = np.arange(n) if ia is None else ia
            b = np.arange(n) if ib is None else ib
            assert np.array_equal(CR.exact_pairs(U, S, ia, ib, n), X[a, b])
        # identity pairs are the variance's exact case
        assert np.array_equal(CR.exact_pairs(U, S, None, None, m), R.exact_case(m, k)[2])


@pytest.mark.parametrize("k", (1, 33, 257))
def test_numpy_double_meets_the_bounds(k):
    m = 129
    U, S = CR.pair_problem(m, k)
    for name in CR.PATTERNS:
        ia, ib, n = CR.pattern(name, m, 2 * m)
        err = np.abs(np.asarray(CR.pairs_double(U, S, ia, ib, n) - CR.pairs(U, S, ia, ib, n), dtype=np.float64))
        assert np.all(err <= CR.pairs_bound(U, S, ia, ib, n)), name
    rows = CR.map_rows(m, 17)
    err = np.abs(np.asarray(CR.maps_double(U, S, rows) - CR.maps(U, S, rows), dtype=np.float64))
    assert np.all(err <= CR.maps_bound(U, S, rows))
    # pairs (i, r) are column r of the maps, in longdouble to its own rounding
    i = np.arange(m, dtype=np.int32)
    for j, r in enumerate(rows):
        col = CR.pairs(U, S, i, np.full(m, r, dtype=np.int32))
        assert np.all(np.abs(np.asarray(col - CR.maps(U, S, rows)[:, j], dtype=np.float64)) <= CR.maps_bound(U, S, rows)[:, j] * 2.0 ** -8)


@pytest.mark.parametrize("m,k", [(1, 1), (129, 33), (129, 257)])
def test_correlations_and_their_bound(m, k):
    zero = 5 if m > 5 else None
    U, S = CR.corr_problem(m, k, zero)
    assert np.all(np.linalg.eigvalsh(S) >= 1.0 - 1e-9) and np.array_equal(S, np.round(S))  # L L' + I, integer
    ratio = CR.variance_ratio(U, S)
    print("m = %d, k = %d: max tau Vbar / v = %.3g" % (m, k, ratio.max()))
    assert ratio.max() < 1e-6  # the first-order bound's premise
    rows = CR.map_rows(m, 16) if zero is None else np.concatenate([CR.map_rows(m, 15), [zero]]).astype(np.int32)
    want, bound = CR.correlations(U, S, rows), CR.correlations_bound(U, S, rows)
    assert np.all(np.abs(want) <= 1 + 1e-15)  # S positive definite: Cauchy-Schwarz
    for j, r in enumerate(rows):
        assert want[r, j] == (0 if r == zero else 1)
    if zero is not None:
        assert np.all(want[zero] == 0) and np.all(want[:, -1] == 0) and np.all(bound[zero] == 0) and np.all(bound[:, -1] == 0)
    err = np.abs(np.asarray(CR.correlations_double(U, S, rows) - want, dtype=np.float64))
    assert np.all(err <= bound), (err / np.where(bound > 0, bound, 1)).max()


# ---- the C++ fallback on the CPU back end --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = tmp_path_factory.mktemp("cpu_covariance") / "covariance_cpu_driver"
    cmd = ["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "rails_amd", "include"),
           "-I" + os.path.join(ROOT, "tests", "cpu_backend"), os.path.join(ROOT, "tests", "cpu_backend", "covariance_cpu_driver.cpp"), "-o", str(out)]
    subprocess.check_call(cmd)
    return str(out)


@pytest.mark.parametrize("zero", [None, 7])
def test_cpp_fallback_matches_the_reference(driver, tmp_path, zero):
    m, k, q = 60, 12, 5
    U, S = CR.corr_problem(m, k, zero)  # S symmetric: the object symmetrises what it is given
    ia, ib, n = CR.pattern("differ", m, 50)
    rows = CR.map_rows(m, q) if zero is None else np.concatenate([CR.map_rows(m, q - 1), [zero]]).astype(np.int32)
    for name, a in (("U", U), ("S", S)):
        np.ascontiguousarray(a, dtype=np.float64).tofile(tmp_path / (name + ".bin"))
    for name, a in (("ia", ia), ("ib", ib), ("rows", rows)):
        np.ascontiguousarray(a, dtype=np.int32).tofile(tmp_path / (name + ".bin"))
    p = lambda s: str(tmp_path / s)
    subprocess.check_call([driver, p("U.bin"), p("S.bin"), str(m), str(k), p("ia.bin"), p("ib.bin"), str(n), p("rows.bin"), str(q), p("out")])
    get = lambda ext, shape: np.fromfile(p("out." + ext)).reshape(shape)
    err = lambda got, want: np.abs(np.asarray(got - want, dtype=np.float64))
    assert np.all(err(get("pairs", (n,)), CR.pairs(U, S, ia, ib)) <= CR.pairs_bound(U, S, ia, ib))
    assert np.all(err(get("pairs_b", (n,)), CR.pairs(U, S, None, ib, n)) <= CR.pairs_bound(U, S, None, ib, n))
    assert np.all(err(get("maps", (m, q)), CR.maps(U, S, rows)) <= CR.maps_bound(U, S, rows))
    corr = get("corr", (m, q))
    assert np.all(err(corr, CR.correlations(U, S, rows)) <= CR.correlations_bound(U, S, rows))
    for j, r in enumerate(rows):
        assert corr[r, j] == (0.0 if r == zero else 1.0)
    if zero is not None:
        assert np.all(corr[zero] == 0.0) and np.all(corr[:, -1] == 0.0)


# ---- header, exports, ctypes, argument checks ----------------------------------------------------------------------------------------------
NEW = {
    "rails_panel_rowpair": (C.c_int, "rails_ctx*, const rails_panel*, int, int, const double*, int, const int32_t*, const int32_t*, int64_t, rails_panel*, int"),
    "rails_allreduce_host": (C.c_int, "rails_ctx*, double*, int64_t"),
    "rails_panel_corr_scale": (C.c_int, "rails_ctx*, rails_panel*, int, int, const rails_panel*, int, const double*, const int32_t*"),
    "rails_solution_pairs": (C.c_int, "rails_solution*, const int32_t*, const int32_t*, int64_t, rails_panel*, int"),
    "rails_solution_maps": (C.c_int, "rails_solution*, const int32_t*, int, int, rails_panel*, int, int"),
}
CTYPE = {"int": C.c_int, "int64_t": C.c_int64, "double*": C.POINTER(C.c_double), "int32_t*": C.POINTER(C.c_int32)}


def test_new_symbols_are_declared_exported_and_bound():
    import rails_amd
    from rails_amd import _solution_sigs as Sg

    text = open(os.path.join(ROOT, "include", "rails_solution.h")).read()
    lib = rails_amd.load()
    for name, (res, params) in NEW.items():
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert decl, name
        # the declaration's parameter types, names and const dropped, are the restated ones
        types = []
        for prm in decl.group(1).split(","):
            t = re.sub(r"\bconst\b", "", prm).strip()
            t = re.sub(r"\s*\*\s*", "* ", t).split()
            types.append(t[0] if len(t) > 1 else t[0])
        want = [re.sub(r"\bconst\b", "", t).strip().replace(" ", "") for t in params.split(",")]
        assert [t.replace(" ", "") for t in types] == want, (name, types, want)
        got_res, got_args = Sg.SOLUTION_SIGNATURES[name]
        assert got_res is res
        assert got_args == [CTYPE.get(t, C.c_void_p) for t in want], name
        fn = getattr(lib, name)  # exported
        assert fn.restype is res and list(fn.argtypes) == got_args


def test_index_validation_happens_before_the_c_call():
    from rails_amd.wrappers import index_array

    assert index_array(None, 5, "ia") is None
    a = index_array(np.array([0, 4, 2], dtype=np.int64), 5, "ia")
    assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"] and a.tolist() == [0, 4, 2]
    assert index_array(np.arange(10)[::2], 9, "ia").tolist() == [0, 2, 4, 6, 8]  # a strided view is made contiguous
    assert index_array([], 5, "ia").size == 0
    assert index_array(np.array([-1, 3]), 5, "rows", lowest=-1).tolist() == [-1, 3]
    with pytest.raises(TypeError, match="ia: row indices must be integers"):
        index_array(np.array([0.0, 1.0]), 5, "ia")
    with pytest.raises(TypeError, match="integers"):
        index_array(np.array([True, False]), 5, "ia")
    with pytest.raises(IndexError, match=r"ib: index 5 at position 1 outside \[0, 5\)"):
        index_array(np.array([0, 5]), 5, "ib")
    with pytest.raises(IndexError, match=r"index -1 at position 0"):
        index_array(np.array([-1]), 5, "ia")
    with pytest.raises(IndexError, match=r"index -2"):
        index_array(np.array([-2]), 5, "rows", lowest=-1)
    with pytest.raises(IndexError):
        index_array(np.array([2 ** 31 + 1], dtype=np.int64), 2 ** 31 - 1, "ia")  # no wrap-around into range
    with pytest.raises(ValueError, match="one-dimensional"):
        index_array(np.zeros((2, 2), dtype=np.int32), 5, "ia")


def test_the_drivers_index_files_are_checked_before_anything_else(tmp_path):
    from rails_amd.main import read_pairs, read_refs

    f = tmp_path / "pairs.txt"
    f.write_text("% i j\n1 5\n\n# comment\n5 1\n3 3\n")
    ia, ib = read_pairs(str(f), 5)
    assert ia.tolist() == [0, 4, 2] and ib.tolist() == [4, 0, 2]  # 1-based in the file
    for text, word in (("0 1\n", "1-based"), ("1 6\n", "1-based"), ("1 2 3\n", "two integers"), ("1 x\n", "not an integer"), ("1.5 2\n", "not an integer")):
        f.write_text(text)
        with pytest.raises(SystemExit, match=word):
            read_pairs(str(f), 5)
    f.write_text("")
    assert read_pairs(str(f), 5)[0].size == 0
    assert read_refs("1, 5,3", 5).tolist() == [0, 4, 2]
    for text, word in (("0", "1-based"), ("6", "1-based"), ("", "between 1 and 64"), (",".join(["1"] * 65), "between 1 and 64"), ("a", "not an integer")):
        with pytest.raises(SystemExit, match=word):
            read_refs(text, 5)
