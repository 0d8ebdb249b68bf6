"""Runs tests/cpp/start_space_capi.cpp (built by rails_amd/csrc/Makefile into rails_amd/lib/start_space_capi): a C++ program on the C ABI
alone hands the solution panel of one solve to a second solver on a perturbed problem (rails_solver_set_start_space with "Restart upon
start") on both back ends."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rails_amd", "lib", "start_space_capi")


@pytest.mark.gpu
def test_cpp_start_space_through_the_c_abi():
    if not os.path.exists(EXE):
        import rails_amd.build

        rails_amd.build.build()
    p = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("OK"), p.stdout[-4000:]
    assert "direct back end: start rank" in p.stdout and "coordinate-space back end: start rank" in p.stdout
