"""Runs tests/cpp/solution_capi.cpp (built by rails_amd/csrc/Makefile into rails_amd/lib/solution_capi): a C++ program on the C ABI alone
makes a solution object from a solver and checks its variance, trace and leading eigenpairs against the dense X = V T V'."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rails_amd", "lib", "solution_capi")


@pytest.mark.gpu
def test_cpp_solution_through_the_c_abi():
    if not os.path.exists(EXE):
        import rails_amd.build

        rails_amd.build.build()
    p = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("OK"), p.stdout[-4000:]
    assert "5 eigenpairs" in p.stdout
