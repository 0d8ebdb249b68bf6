"""The host part of the block-CSR operator (rails_amd/csrc/bsr_host.cpp: the b x b blocking of a CSR matrix, the stable block transpose,
their refusals) and the launch rule of its kernel (rails_amd/csrc/bsr_choice.h), checked on the CPU by a stand-alone program
(tests/cpp/bsr_host.cpp, built by rails_amd/csrc/Makefile into rails_amd/lib/bsr_host: no HIP, no library) against a dense reference and
over every shape of the rule's ranges, and once more built with the address and undefined-behaviour sanitizers.  The Python side of the
conversion (rails_amd.csr_to_bsr, problems.block_stencil7) is checked against scipy."""
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rails_amd", "lib", "bsr_host")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def run(exe):
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0 and "ALL PASSED" in p.stdout, p.stdout[-4000:]
    assert " 0 failed" in p.stdout


def built():
    if not os.path.exists(EXE):
        import rails_amd.build

        rails_amd.build.build()
    return EXE


def test_conversion_transpose_refusals_and_rule_on_the_host():
    run(built())


def test_the_same_program_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "bsr_host_san")
    # host code only: the program has no device part, and -fno-gpu-sanitize says so to the compiler driver as well
    cmd = [HIPCC, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "rails_amd", "csrc"),
           "-I" + os.path.join(ROOT, "include"), "-x", "c++", os.path.join(ROOT, "tests", "cpp", "bsr_host.cpp"), os.path.join(ROOT, "rails_amd", "csrc", "bsr_host.cpp"), "-o", exe]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:]
    run(exe)


def test_table_names_every_instantiation_once_at_its_smallest_shape():
    p = subprocess.run([built(), "--table"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:]
    rows = [json.loads(line) for line in p.stdout.splitlines()]
    keys = [tuple(r["inst"]) for r in rows]
    assert len(keys) == len(set(keys)) == 21
    assert sorted(keys) == [(b, lpr) for b in range(2, 9) for lpr in (8, 16, 32)]
    for r in rows:
        b, lpr = r["inst"]
        assert r["b"] == b and r["mb"] == 1 and r["nc"] == {8: 1, 16: 17, 32: 33}[lpr]
        assert r["rows"] == r["threads"] // lpr  # one round of block rows at the smallest shape


def test_csr_to_bsr_agrees_with_scipy():
    import scipy.sparse as sp

    import rails_amd

    for b in (2, 3, 5, 8):
        m = 6 * b
        A = sp.random(m, m, density=0.15, random_state=np.random.RandomState(b), format="csr")
        indptr, indices, data = rails_amd.csr_to_bsr(m, m, b, A.indptr, A.indices, A.data)
        S = sp.bsr_matrix(A, blocksize=(b, b))
        S.sort_indices()
        assert np.array_equal(indptr, S.indptr) and np.array_equal(indices, S.indices) and np.array_equal(data, S.data)
        assert data.shape == (indices.size, b, b) and indptr.dtype == np.int64 and indices.dtype == np.int32
    try:
        rails_amd.csr_to_bsr(7, 7, 2, np.zeros(8, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0))
    except rails_amd.RailsError as e:
        assert "no multiple of the block size" in str(e)
    else:
        raise AssertionError("7 rows in blocks of 2 were accepted")


def test_block_stencil7_is_one_matrix_in_two_forms():
    import scipy.sparse as sp

    from rails_amd import problems as P

    for (nx, ny, nz, b) in ((4, 3, 2, 2), (3, 3, 3, 6)):
        (indptr, indices, data), (rowptr, col, val) = P.block_stencil7(nx, ny, nz, b, seed=2)
        mb = nx * ny * nz
        S = sp.bsr_matrix((data, indices, indptr), shape=(mb * b, mb * b))
        A = sp.csr_matrix((val, col, rowptr), shape=(mb * b, mb * b))
        assert np.array_equal(S.toarray(), A.toarray())
        assert rowptr[-1] == indices.size * b * b and np.all(np.diff(indptr) <= 7) and indptr[-1] == 7 * mb - 2 * (nx * ny + ny * nz + nx * nz)
        # stable: the block diagonal dominates every row (Gershgorin discs in the left half plane)
        D = A.toarray()
        off = np.abs(D).sum(1) - np.abs(np.diag(D))
        assert np.all(np.diag(D) < 0) and np.all(-np.diag(D) > off)
        again = P.block_stencil7(nx, ny, nz, b, seed=2)
        assert np.array_equal(again[0][2], data) and not np.array_equal(P.block_stencil7(nx, ny, nz, b, seed=3)[0][2], data)
