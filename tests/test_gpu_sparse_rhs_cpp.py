"""Runs tests/cpp/sparse_rhs_capi.cpp and tests/cpp/sparse_rhs_classes.cpp (built by rails_amd/csrc/Makefile into rails_amd/lib/): the
reference's known answer with B = -I as a CSR operator (test/LyapunovSolverEpetra_test.cpp:109-177), once through the C ABI alone and
once through the drop-in classes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
@pytest.mark.parametrize("name,line", [("sparse_rhs_capi", "known answer: return 0"), ("sparse_rhs_classes", "known answer through the classes: return 0")])
def test_cpp_known_answer_with_a_sparse_B(name, line):
    exe = os.path.join(ROOT, "rails_amd", "lib", name)
    if not os.path.exists(exe):
        import rails_amd.build

        rails_amd.build.build()
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("OK"), p.stdout[-4000:]
    assert line in p.stdout
