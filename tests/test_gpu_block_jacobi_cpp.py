"""Runs tests/cpp/iter_block_jacobi_capi.cpp (built by rails_amd/csrc/Makefile into rails_amd/lib/iter_block_jacobi_capi): a program on the
C ABI alone makes a rails_iter (conjugate gradients) for a chain of stiff 3 x 3 cells, installs the block-Jacobi preconditioner from the
CSR arrays and from explicit blocks, reads rails_iter_block_jacobi_info, solves in fewer than half of point Jacobi's iterations, toggles
and clears the setting, and meets the refusals."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rails_amd", "lib", "iter_block_jacobi_capi")


@pytest.mark.gpu
def test_c_abi_block_jacobi_preconditioner():
    if not os.path.exists(EXE):
        import rails_amd.build

        rails_amd.build.build()
    p = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("OK"), p.stdout[-4000:]
    assert "unconverged columns 0" in p.stdout and "FAILED" not in p.stdout
