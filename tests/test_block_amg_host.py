"""The host set-up of the block multigrid preconditioner and the launch decision of its cycle, no GPU: the stand-alone program
tests/cpp/block_amg_host.cpp (linked against block_amg_host.o and the host objects it stands on alone) builds the hierarchies of
block_diffusion7, and its aggregates and sparsity patterns must equal those of the restatement tests/block_amg_reference.py exactly, its
values the restatement's within the restatement's own float64 error against longdouble; two builds must give the same bytes (checked
inside the program); every refusal; the program again under the address and undefined-behaviour sanitizers; the launch decision against
its Python restatement; and the scalar set-up, which now shares three functions with the block one, against digests of what it produced
before."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import amg_reference as M
import block_amg_reference as B
from test_amg_host import _Reader, same_pattern

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rails_amd", "lib", "block_amg_host")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
EPS = np.finfo(float).eps
# (cells, coarse): 48 cells with a coarse low enough for two matrices at every b; the larger grids at the default
GRIDS = (((4, 4, 3), None), ((6, 6, 6), 256), ((8, 8, 8), 256))
BS = (2, 3, 4, 5, 6, 7, 8)


def built():
    if not os.path.exists(EXE):
        import rails_amd.build

        rails_amd.build.build()
    return EXE


def write_input(triple, path):
    ip, ix, dt = triple
    with open(path, "wb") as f:
        f.write(np.array([len(ip) - 1, dt.shape[1], len(ix)], dtype=np.int64).tobytes())
        f.write(np.asarray(ip, dtype=np.int64).tobytes() + np.asarray(ix, dtype=np.int32).tobytes() + np.ascontiguousarray(dt, dtype=np.float64).tobytes())


def read_bsr(r, b):
    mb, nnzb = (int(v) for v in r.take(np.int64, 2))
    return r.take(np.int64, mb + 1), r.take(np.int32, nnzb).astype(np.int64), r.take(np.float64, nnzb * b * b).reshape(nnzb, b, b)


def build(triple, theta, coarse, tmp_path, exe=None):
    """the program's hierarchy in the restatement's layout; (None, message) where it refuses"""
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    write_input(triple, src)
    res = subprocess.run([exe or built(), "dump", src, dst, repr(float(theta)), str(int(coarse))], capture_output=True, text=True, timeout=300)
    if res.returncode == 3:
        return None, res.stdout
    assert res.returncode == 0, res.stdout + res.stderr
    assert "two builds identical" in res.stdout
    r = _Reader(open(dst, "rb").read())
    n_levels, b = (int(v) for v in r.take(np.int64, 2))
    defsign = float(r.take(np.float64)[0])
    levels = []
    for _ in range(n_levels):
        lv = {"bsr": read_bsr(r, b)}
        lv["P"], lv["R"] = r.csr(), r.csr()
        mb = len(lv["bsr"][0]) - 1
        lv["G"], lv["hi"], lv["agg"] = r.take(np.float64, mb * b * b).reshape(mb, b, b), float(r.take(np.float64)[0]), r.take(np.int32, mb)
        levels.append(lv)
    coarse_bsr = read_bsr(r, b)
    n = (len(coarse_bsr[0]) - 1) * b
    Ainv = r.take(np.float64, n * n).reshape(n, n).T  # column-major
    assert r.at == len(r.raw)
    return {"b": b, "levels": levels, "coarse_bsr": coarse_bsr, "Ainv": Ainv, "defsign": defsign}, res.stdout


def same_blocks(g, w):
    return np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]) and g[2].shape == w[2].shape


def galerkin_scale(prev):
    return (abs(prev["R"]) @ abs(prev["A"]) @ abs(prev["P"])).tocsr()


def block_scale(S, w_bsr, b):
    """|R| |A| |P| on the block layout of w_bsr"""
    (ip, ix, data), _ = B.block_up(S, b)
    assert np.array_equal(ip, w_bsr[0]) and np.array_equal(ix, w_bsr[1])
    return data


@pytest.mark.parametrize("b", BS)
@pytest.mark.parametrize("grid,coarse", GRIDS)
def test_hierarchy_is_the_restatements(grid, coarse, b, tmp_path):
    (ip, ix, dt), _ = B.P.block_diffusion7(*grid, b, 100.0, 0.01)
    coarse = coarse or 8 * b
    triple = (ip.astype(np.int64), ix.astype(np.int64), dt)
    got, out = build(triple, B.THETA, coarse, tmp_path)
    assert got is not None, out
    want = B.setup(triple, B.THETA, coarse, longdouble=True)
    assert got["b"] == b and got["defsign"] == want["defsign"] == -1.0
    assert len(got["levels"]) == len(want["levels"]) >= 1
    rows = [(len(lv["bsr"][0]) - 1) * b for lv in got["levels"]] + [(len(got["coarse_bsr"][0]) - 1) * b]
    assert rows == B.rows_of(want) and all(r % b == 0 for r in rows)
    worst, equal_bytes = 0.0, True
    mats = [lv["bsr"] for lv in got["levels"]] + [got["coarse_bsr"]]
    for l, (g, w) in enumerate(zip(got["levels"], want["levels"])):
        mb = len(g["bsr"][0]) - 1
        # the aggregates: every cell in exactly one, every aggregate used, T'T diagonal with the aggregate sizes times I_b
        assert np.array_equal(g["agg"], w["agg"]), (l,)
        n_agg = int(g["agg"].max()) + 1
        assert np.array_equal(np.unique(g["agg"]), np.arange(n_agg)) and g["agg"].size == mb
        tcol = np.repeat(g["agg"].astype(np.int64), b) * b + np.tile(np.arange(b), mb)
        T = sp.csr_matrix((np.ones(mb * b), tcol, np.arange(mb * b + 1)), shape=(mb * b, n_agg * b))
        TT = (T.T @ T).tocsr()
        assert TT.nnz == n_agg * b and np.array_equal(TT.diagonal(), np.repeat(np.bincount(g["agg"], minlength=n_agg), b))
        assert same_blocks(g["bsr"], w["bsr"]), (l, "A")
        for name in ("P", "R"):
            assert same_pattern(g[name], w[name]), (l, name)
        assert g["P"].shape == (mb * b, n_agg * b)
        assert np.array_equal(g["R"].data, sp.csr_matrix(g["P"].T).data)  # R is P' entry for entry
        # The values.  Below the top a level matrix is the program's own, the restatement's within rounding only, and G -- an inverse --
        # amplifies that by the blocks' condition; so every level is held to one step of the restatement from the program's own matrix
        # of that level, in float64 and in longdouble: the same aggregates and patterns, G, hi, P and the next matrix.
        step = B.setup(g["bsr"], B.THETA, rows[l + 1], longdouble=True, first_level=l, one_level=True)
        s0 = step["levels"][0]
        assert np.array_equal(s0["agg"], g["agg"]) and same_pattern(s0["P"], g["P"]) and same_blocks(step["coarse_bsr"], mats[l + 1])
        assert np.all(np.abs(g["G"] - s0["G_ld"]).astype(float) <= s0["G_bound"]), (l, "G")
        hi_bound = max(4 * abs(s0["hi"] - float(s0["hi_ld"])), 64 * EPS * s0["hi"])
        assert abs(g["hi"] - float(s0["hi_ld"])) <= hi_bound and abs(g["hi"] - w["hi"]) <= 1e-9 * w["hi"], (l, "hi")
        if mb * b <= 648:
            Gm = sp.block_diag(list(g["G"])).toarray()
            lam = np.linalg.eigvals(Gm @ B.expand(*g["bsr"]).toarray())
            assert np.abs(lam.imag).max() <= 1e-9 * g["hi"] and lam.real.min() > 0
            assert g["hi"] >= lam.real.max() * (1 - 1e-12)
        Pabs = abs(s0["P"]).data + 1.0
        bound = B.value_bound(np.abs(s0["P"].data - s0["P_ld"]).astype(float), Pabs)
        err = np.abs(g["P"].data - s0["P_ld"]).astype(float)
        worst = max(worst, (err / bound).max())
        assert np.all(err <= bound), (l, "P", (err / bound).max())
        scale = block_scale(galerkin_scale(s0), step["coarse_bsr"], b)
        bound = B.value_bound(np.abs(step["coarse_bsr"][2] - step["coarse_ld"]).astype(float), scale)
        err = np.abs(mats[l + 1][2] - step["coarse_ld"]).astype(float)
        worst = max(worst, (err / bound).max())
        assert np.all(err <= bound), (l, "the next matrix", (err / bound).max())
        # symmetric to within that bound (the exact Galerkin product of a symmetric matrix is)
        nxt, sym = B.expand(*mats[l + 1]), B.expand(mats[l + 1][0], mats[l + 1][1], bound)
        assert np.all(np.abs((nxt - nxt.T).toarray()) <= (sym + sym.T).toarray()), (l, "symmetry")
        # and the whole hierarchy stays with the restatement's own, loosely (the conditioning of the blocks is in between)
        assert np.all(np.abs(mats[l + 1][2] - (want["levels"][l + 1]["bsr"] if l + 1 < len(want["levels"]) else want["coarse_bsr"])[2]) <= 1e-9 * scale)
        equal_bytes = equal_bytes and np.array_equal(g["P"].data, s0["P"].data) and np.array_equal(g["G"], s0["G"]) and g["hi"] == s0["hi"] and np.array_equal(
            mats[l + 1][2], step["coarse_bsr"][2])
    assert np.array_equal(mats[0][2], dt)
    # the dense inverse, of the program's own last matrix
    dense = B.expand(*got["coarse_bsr"]).toarray()
    want = {"Ainv": np.linalg.inv(dense), "coarse": sp.csr_matrix(dense)}
    want["Ainv_exact"] = M._refined_inverse(dense, want["Ainv"])
    exact = want["Ainv_exact"]
    cond = np.linalg.cond(want["coarse"].toarray())
    bound = max(4 * float(np.abs(want["Ainv"] - exact).max()), 64 * EPS * float(np.abs(exact).max()) * cond)
    err = float(np.abs(got["Ainv"] - exact).max())
    print("cells %s, b = %d: rows %s, operator complexity %.2f, largest value error / allowed %.3f, inverse %.3f (condition %.1f), values %s" % (
        grid, b, rows, sum(m[2].size for m in mats) / mats[0][2].size, worst, err / bound, cond, "equal to the restatement's bytes" if equal_bytes else "within the bounds"))
    assert err <= bound


def test_rules_and_refusals():
    res = subprocess.run([built(), "rules"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "FAILED" not in res.stdout and " 0 failed" in res.stdout, res.stdout + res.stderr


def test_the_same_program_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "block_amg_host_san")
    csrc = os.path.join(ROOT, "rails_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "cpp", "block_amg_host.cpp")] + [os.path.join(csrc, f) for f in (
        "block_amg_host.cpp", "amg_host.cpp", "block_jacobi_host.cpp", "bsr_host.cpp", "sprhs_host.cpp", "host_lapack.cpp")]
    # host code only: the program has no device part, and -fno-gpu-sanitize says so to the compiler driver as well
    cmd = [HIPCC, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=all", "-I" + csrc,
           "-I" + os.path.join(ROOT, "include"), "-x", "c++"] + srcs + ["-o", exe, "-ldl", "-lpthread"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:]
    res = subprocess.run([exe, "rules"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and " 0 failed" in res.stdout, res.stdout + res.stderr
    (ip, ix, dt), _ = B.P.block_diffusion7(6, 6, 6, 3, 100.0, 0.01)
    got, out = build((ip, ix, dt), B.THETA, 64, tmp_path, exe=exe)
    assert got is not None and len(got["levels"]) == 2, out


def test_refusals_through_the_dump(tmp_path):
    (ip, ix, dt), _ = B.P.block_diffusion7(3, 3, 2, 2, 100.0, 0.01)
    bad = dt.copy()
    bad[3, 1, 0] = np.inf
    got, out = build((ip, ix, bad), B.THETA, 8, tmp_path)
    assert got is None and "not finite" in out
    got, out = build((ip, ix[::-1].copy(), dt), B.THETA, 8, tmp_path)
    assert got is None and ("not strictly increasing" in out or "no stored diagonal block" in out)
    eye = np.arange(600)
    got, out = build((np.arange(601), eye, np.tile(np.eye(2), (600, 1, 1)) * (1.0 + eye % 5)[:, None, None]), B.THETA, 256, tmp_path)
    assert got is None and "does not coarsen" in out
    with pytest.raises(ValueError, match="does not coarsen"):
        B.setup((np.arange(601), eye, np.tile(np.eye(2), (600, 1, 1)) * (1.0 + eye % 5)[:, None, None]))
    got, out = build((np.array([0, 1]), np.array([0]), np.array([[[1.0, 3.0], [3.0, 1.0]]])), B.THETA, 8, tmp_path)
    assert got is None and "not definite" in out


def test_launch_decision_is_the_restatements():
    res = subprocess.run([built(), "choice"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr
    steps = rows = 0
    for line in res.stdout.splitlines():
        left, right = line.split(" -> ")
        kind, *args = left.split()
        vals = [int(v) for v in right.split()]
        if kind == "rows":
            m, b = (int(v) for v in args)
            assert vals == [1 if B.rows_ok(m, b) else 0], line
            rows += 1
            continue
        b, nc, mb, mx, ld, want = (int(v) for v in args)
        ok, fused, lds = B.step_choice(b, nc, mb, mx, ld, want)
        k = B.bsr_choice(b, nc, mb, mx) if ok else None
        expect = [1, 1 if fused else 0, k[0], k[1], k[2], k[5], lds] if ok else [0, 0, 0, 0, 0, 0, 0]
        assert vals == expect, (line, expect)
        if ok:
            assert fused == bool(want) and lds <= 64 * 1024 and k[5] % 8 == 0 and k[5] * k[3] // 8 * 8 >= mb
        steps += 1
    assert steps > 30000 and rows == 99


def test_scalar_set_up_gives_the_bytes_it_gave(tmp_path):
    """rails_amg_build_host shares its aggregation, its sparse product and its dense inverse with the block set-up: everything it
    produces before the dense inverse (which goes through the host's LAPACK) has the digest recorded before the functions were shared"""
    exe = os.path.join(ROOT, "rails_amd", "lib", "amg_host")
    built()
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "amg_host_hierarchies_sha256.json")))
    assert sorted(golden) == sorted(["lap9x8", "banded41", "neg_banded41", "one", "stencil27", "lap24", "lap7_12"])
    for tag, rec in golden.items():
        A, coarse = M.problem(tag)
        assert coarse == rec["coarse"] and M.THETA == rec["theta"]
        A = sp.csr_matrix(A)
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(src, "wb") as f:
            f.write(np.array([A.shape[0], A.nnz], dtype=np.int64).tobytes())
            f.write(A.indptr.astype(np.int64).tobytes() + A.indices.astype(np.int32).tobytes() + A.data.astype(np.float64).tobytes())
        res = subprocess.run([exe, "dump", src, dst, repr(float(M.THETA)), str(int(coarse))], capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stdout + res.stderr
        raw = open(dst, "rb").read()
        assert hashlib.sha256(raw[:rec["bytes_before_inverse"]]).hexdigest() == rec["sha256"], tag
