"""The rule of the iterative solve's preconditioners (rails_amd/csrc/iter_precond.h: which request is granted and with what refusal, what
is in effect for a call), checked on the CPU by a stand-alone program (tests/cpp/iter_precond_host.cpp, built by rails_amd/csrc/Makefile
into rails_amd/lib/iter_precond_host from the header alone: no HIP, no library) against the restatement of tests/iter_precond_reference.py
over the whole product of facts and requests, line by line; and once more built with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import iter_precond_reference as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rails_amd", "lib", "iter_precond_host")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def built():
    if not os.path.exists(EXE):
        import rails_amd.build

        rails_amd.build.build()
    return EXE


def run(exe):
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0 and "ALL PASSED" in p.stdout, p.stdout[-4000:]
    assert " 0 failed" in p.stdout


def table(exe):
    p = subprocess.run([exe, "--table"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-4000:]
    return p.stdout.splitlines()


def compare(lines):
    """every line of the program's table against the restatement's: granted or refused, the exact text, the effect, the sign, the panels"""
    want = list(P.table())
    assert len(lines) == len(want) == 2 * 7 * 4 * 4 * 8 * 32 + 2 * 7 * 4 * 4 * 4 * 32 * 8, (len(lines), len(want))
    wrong = [(got, exp) for got, exp in zip(lines, want) if got != exp]
    assert not wrong, "%d lines differ, the first:\n%s\n%s" % (len(wrong), wrong[0][0], wrong[0][1])
    refused = sum(1 for ln in want if ln.startswith("R ") and not ln.endswith("| granted"))
    assert 0 < refused < sum(1 for ln in want if ln.startswith("R "))
    # 4 of "poly_degree", 4 of "block_jacobi", 3 of the install, 9 of "amg" and 7 of "block_amg" under two names each, one of the scalar
    # set-up alone; the row counts of the product make 2 + 4 more
    assert len({ln.split(" | ")[2] for ln in want if ln.startswith("R ") and not ln.endswith("| granted")}) == 50


def test_the_rule_on_the_host():
    run(built())


def test_the_rule_against_the_restatement():
    compare(table(built()))


def test_the_same_program_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "iter_precond_host_san")
    # host code only: the program has no device part, and -fno-gpu-sanitize says so to the compiler driver as well
    cmd = [HIPCC, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "rails_amd", "csrc"), "-x", "c++",
           os.path.join(ROOT, "tests", "cpp", "iter_precond_host.cpp"), "-o", exe]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:]
    run(exe)
    compare(table(exe))
