"""The host arithmetic of the coordinate back end's block orthogonalisation (rails_amd/include/rails/BlockOrthHost.hpp), checked on the
CPU by a stand-alone program (tests/cpp/block_orth_host.cpp, built by rails_amd/csrc/Makefile into rails_amd/lib/block_orth_host from the
header and host_lapack.o only: no HIP, no library).

The program makes its inputs from an integer hash and its expected values in long double arithmetic of its own: the scaled Cholesky
factor, the triangular inverse and product, the DGKS rule, the overlapped form's prediction and re-base end to end (with the device's
part played in plain loops) and its three rejections, and the coefficient store's "column in use" query."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rails_amd", "lib", "block_orth_host")


def test_block_orthogonalisation_arithmetic_on_the_host():
    if not os.path.exists(EXE):
        import rails_amd.build

        rails_amd.build.build()
    p = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0 and "ALL PASSED" in p.stdout, p.stdout[-4000:]
    assert " 0 failed" in p.stdout
