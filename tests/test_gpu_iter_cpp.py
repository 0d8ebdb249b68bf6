"""Runs tests/cpp/iter_projection.cpp (built by rails_amd/csrc/Makefile into rails_amd/lib/iter_projection): a C++ program on the header-only
classes and the C ABI alone makes a rails_iter (conjugate gradients) for a 2D Laplacian, checks A (A^-1 x) = x and solves a Lyapunov
problem with "Projection method" 2.2 on both back ends with it as the inverse."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rails_amd", "lib", "iter_projection")


@pytest.mark.gpu
def test_cpp_iterative_inverse_and_extended_projection():
    if not os.path.exists(EXE):
        import rails_amd.build

        rails_amd.build.build()
    p = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("OK"), p.stdout[-4000:]
    assert "direct back end, projection 2.2: return 0" in p.stdout and "coordinate-space back end, projection 2.2: return 0" in p.stdout
    assert "unconverged columns 0" in p.stdout
