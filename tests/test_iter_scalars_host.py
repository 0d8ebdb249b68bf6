"""The scalar step of the iterative A^-1 operator (rails_amd/csrc/iter_scalars.h: coefficients, guards against dividing by zero, breakdown
rules, the non-finite test, the freeze), checked on the CPU by a stand-alone program (tests/cpp/iter_scalars_host.cpp, built by
rails_amd/csrc/Makefile into rails_amd/lib/iter_scalars_host from the header alone: no HIP, no library)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rails_amd", "lib", "iter_scalars_host")


def test_iterative_solve_scalar_step_on_the_host():
    if not os.path.exists(EXE):
        import rails_amd.build

        rails_amd.build.build()
    p = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0 and "ALL PASSED" in p.stdout, p.stdout[-4000:]
    assert " 0 failed" in p.stdout
