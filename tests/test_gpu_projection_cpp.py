"""Runs tests/cpp/projection_lu.cpp (built by rails_amd/csrc/Makefile into rails_amd/lib/projection_lu): a C++ program on the header-only
classes and the C ABI alone builds a rails_lu from factors it computes itself and solves a 2D Laplace problem with "Projection method"
2.2 on both back ends."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rails_amd", "lib", "projection_lu")


@pytest.mark.gpu
def test_cpp_lu_and_extended_projection():
    if not os.path.exists(EXE):
        import rails_amd.build

        rails_amd.build.build()
    p = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("OK"), p.stdout[-4000:]
    assert "direct back end, projection 2.2: return 0" in p.stdout and "coordinate-space back end, projection 2.2: return 0" in p.stdout
