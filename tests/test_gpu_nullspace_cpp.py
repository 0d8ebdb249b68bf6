"""Runs tests/cpp/nullspace_capi.cpp (built by rails_amd/csrc/Makefile into rails_amd/lib/nullspace_capi): a C++ program on the C ABI alone
solves a pure Neumann 2D Laplace problem with rails_solver_set_nullspace on both back ends."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rails_amd", "lib", "nullspace_capi")


@pytest.mark.gpu
def test_cpp_nullspace_through_the_c_abi():
    if not os.path.exists(EXE):
        import rails_amd.build

        rails_amd.build.build()
    p = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("OK"), p.stdout[-4000:]
    assert "direct back end, nullspace rank 1: return 0" in p.stdout and "coordinate-space back end, nullspace rank 1: return 0" in p.stdout
