"""The host set-up of the smoothed-aggregation multigrid preconditioner, no GPU: the stand-alone program tests/cpp/amg_host.cpp (linked
against amg_host.o, sprhs_host.o and host_lapack.o alone) builds the hierarchies of the shared problems, and its aggregates and sparsity
patterns must equal those of the restatement tests/amg_reference.py exactly, its values and the dense inverse within the restatement's own
float64 error against longdouble; two builds must give the same bytes (checked inside the program); the stop rules, the cap of 1024 rows
and every refusal; and the restatement's preconditioned iteration counts, a fifth of Jacobi's at most."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import amg_reference as M
import cheb_reference as C
import iter_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rails_amd", "lib", "amg_host")
EPS = np.finfo(float).eps
PROBLEMS = ["lap9x8", "banded41", "neg_banded41", "one", "stencil27", "lap24", "lap7_12"]


class _Reader:
    def __init__(self, raw):
        self.raw, self.at = raw, 0

    def take(self, dtype, n=1):
        out = np.frombuffer(self.raw, dtype=dtype, count=n, offset=self.at)
        self.at += out.nbytes
        return out

    def csr(self):
        rows, cols, nnz = (int(v) for v in self.take(np.int64, 3))
        rowptr, col, val = self.take(np.int64, rows + 1), self.take(np.int32, nnz), self.take(np.float64, nnz)
        return sp.csr_matrix((val, col, rowptr), shape=(rows, cols))


def build(A, theta, coarse, tmp_path):
    """the program's hierarchy of A in the restatement's layout; (None, message) where it refuses"""
    A = sp.csr_matrix(A)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([A.shape[0], A.nnz], dtype=np.int64).tobytes())
        f.write(A.indptr.astype(np.int64).tobytes() + A.indices.astype(np.int32).tobytes() + A.data.astype(np.float64).tobytes())
    res = subprocess.run([EXE, "dump", src, dst, repr(float(theta)), str(int(coarse))], capture_output=True, text=True, timeout=120)
    if res.returncode == 3:
        return None, res.stdout
    assert res.returncode == 0, res.stdout + res.stderr
    assert "two builds identical" in res.stdout
    r = _Reader(open(dst, "rb").read())
    n_levels, defsign = int(r.take(np.int64)[0]), float(r.take(np.float64)[0])
    levels = []
    for _ in range(n_levels):
        lv = {"A": r.csr(), "P": r.csr(), "R": r.csr()}
        n = lv["A"].shape[0]
        lv["dinv"], lv["hi"], lv["agg"] = r.take(np.float64, n), float(r.take(np.float64)[0]), r.take(np.int32, n)
        levels.append(lv)
    coarse_m = r.csr()
    n = coarse_m.shape[0]
    Ainv = r.take(np.float64, n * n).reshape(n, n).T  # column-major
    assert r.at == len(r.raw)
    return {"levels": levels, "coarse": coarse_m, "Ainv": Ainv, "defsign": defsign}, res.stdout


def same_pattern(X, Y):
    return X.shape == Y.shape and np.array_equal(X.indptr, Y.indptr) and np.array_equal(X.indices, Y.indices)


def value_bound(err64, scale):
    """the rule of tests/test_gpu_iter_poly.py::expected: 4 times the float64 restatement's own error against its longdouble
    evaluation, at least 64 eps times the entry's scale"""
    return np.maximum(4 * err64, 64 * EPS * scale)


@pytest.mark.parametrize("tag", PROBLEMS)
def test_hierarchy_is_the_restatements(tag, tmp_path):
    A, coarse = M.problem(tag)
    got, out = build(A, M.THETA, coarse, tmp_path)
    assert got is not None, out
    want = M.setup(A, M.THETA, coarse, longdouble=True)
    assert M.rows_of(got) == M.rows_of(want) and got["defsign"] == want["defsign"]
    worst = 0.0
    for l, (g, w) in enumerate(zip(got["levels"], want["levels"])):
        assert np.array_equal(g["agg"], w["agg"]), (tag, l)
        for name in ("A", "P", "R"):
            assert same_pattern(g[name], w[name]), (tag, l, name)  # (the restatement's columns are sorted: so are these)
            assert w[name].has_sorted_indices
        assert np.array_equal(g["R"].data, sp.csr_matrix(g["P"].T).data)  # R is P' entry for entry
        # values: P against (|I| + omega |D^-1| |A|) |T| entry-wise, A_l against |R| |A| |P|
        hi_err = abs(g["hi"] - w["hi"])
        assert hi_err <= 4 * EPS * w["hi"]
        assert np.all(np.abs(g["dinv"] - w["dinv"]) <= EPS * np.abs(w["dinv"]))
        Pabs = abs(w["P"]).data + 1.0
        bound = value_bound(np.abs(w["P"].data - w["P_ld"]).astype(float), Pabs)
        err = np.abs(g["P"].data - w["P_ld"]).astype(float)
        worst = max(worst, (err / bound).max())
        assert np.all(err <= bound), (tag, l, "P", (err / bound).max())
        if l > 0:
            prev = want["levels"][l - 1]
            scale = (abs(prev["R"]) @ abs(prev["A"]) @ abs(prev["P"])).tocsr()
            scale.sort_indices()
            assert same_pattern(scale, w["A"])
            bound = value_bound(np.abs(w["A"].data - w["A_ld"]).astype(float), scale.data)
            err = np.abs(g["A"].data - w["A_ld"]).astype(float)
            worst = max(worst, (err / bound).max())
            assert np.all(err <= bound), (tag, l, "A", (err / bound).max())
        else:
            assert np.array_equal(g["A"].data, sp.csr_matrix(A).data)
    assert same_pattern(got["coarse"], want["coarse"])
    if want["levels"]:
        prev = want["levels"][-1]
        scale = (abs(prev["R"]) @ abs(prev["A"]) @ abs(prev["P"])).tocsr()
        scale.sort_indices()
        bound = value_bound(np.abs(want["coarse"].data - want["coarse_ld"]).astype(float), scale.data)
        err = np.abs(got["coarse"].data - want["coarse_ld"]).astype(float)
        worst = max(worst, (err / bound).max())
        assert np.all(err <= bound), (tag, "coarse", (err / bound).max())
    # the dense inverse: at least 64 eps ||Ainv||_max times the condition number
    exact = want["Ainv_exact"]
    cond = np.linalg.cond(want["coarse"].toarray())
    bound = max(4 * float(np.abs(want["Ainv"] - exact).max()), 64 * EPS * float(np.abs(exact).max()) * cond)
    err = float(np.abs(got["Ainv"] - exact).max())
    print("problem %s: rows %s, operator complexity %.2f, largest value error / allowed %.3f, inverse %.3f (condition %.1f)" % (
        tag, M.rows_of(got), M.operator_complexity(got), worst, err / bound, cond))
    assert err <= bound


def test_the_levels_the_problems_are_chosen_for():
    """what the shapes are for: three levels at 24 x 24 with coarse 16, long rows below the top in 3D and in the banded problem"""
    assert M.rows_of(M.hierarchy("lap24")[1]) == [576, 102, 14]
    h = M.hierarchy("lap7_12")[1]
    assert len(h["levels"]) == 2 and h["levels"][1]["A"].getnnz(1).max() >= 40 and h["levels"][1]["P"].getnnz(1).max() > 8
    h = M.hierarchy("banded41")[1]
    assert M.rows_of(h) == [130, 65, 2] and h["levels"][0]["P"].getnnz(1).max() > 16
    assert M.rows_of(M.hierarchy("stencil27")[1]) == [60] and M.rows_of(M.hierarchy("one")[1]) == [1]
    assert 1.3 < M.operator_complexity(M.hierarchy("lap24")[1]) < 1.4


def test_rules_and_refusals():
    res = subprocess.run([EXE, "rules"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "FAILED" not in res.stdout and " 0 failed" in res.stdout, res.stdout + res.stderr


def test_refusals_through_the_dump(tmp_path):
    """a matrix from a file takes the same road: indefinite, and not coarsening past the cap"""
    got, out = build(sp.csr_matrix(np.array([[1.0, 3.0], [3.0, 1.0]])), M.THETA, 8, tmp_path)
    assert got is None and "not definite" in out
    got, out = build(sp.diags(np.arange(1.0, 1101.0)).tocsr(), M.THETA, 256, tmp_path)
    assert got is None and "does not coarsen" in out
    with pytest.raises(ValueError, match="does not coarsen"):
        M.setup(sp.diags(np.arange(1.0, 1101.0)).tocsr())


@pytest.mark.parametrize("tag", ["lap64", "lap128"])
def test_iteration_counts_do_not_grow_with_the_grid(tag):
    """conjugate gradients with the cycle in the restatement: below a fifth of Jacobi's count (64 x 64: 10 against 226; 128 x 128: 12
    against 446), and nearly the same on both grids"""
    A, Bm, X, c = M.reference(tag, 3)
    _, cj = R.cg(A, Bm, tol=1e-10, maxit=5000)
    print("problem %s: rows %s, cycle %s, Jacobi %s" % (tag, M.rows_of(M.hierarchy(tag)[1]), c.iter, cj.iter))
    assert np.all(c.flags == R.CONVERGED) and np.all(cj.flags == R.CONVERGED)
    assert R.true_relres(A, X, Bm).max() <= 1e-9
    assert np.all(5 * c.iter < cj.iter)
    assert c.iter.max() <= 14


def test_the_cycle_is_symmetric_and_has_the_operators_sign():
    """x' M y = y' M x for the cycle M, and x' M x of the sign of the operator, for every smoother degree"""
    for tag in ("lap24", "neg_banded41", "banded41"):
        A, h = M.hierarchy(tag)
        Xm = R.rhs(A.shape[0], 4, seed=11)
        for S in (0, 1, 2):
            Z = M.vcycle(h, Xm, S, dtype=np.longdouble)
            G = (Xm.astype(np.longdouble).T @ Z).astype(float)
            assert np.abs(G - G.T).max() <= 1e-13 * np.abs(G).max(), (tag, S)
            assert np.all(np.sign(np.diag(G)) == h["defsign"]), (tag, S)
