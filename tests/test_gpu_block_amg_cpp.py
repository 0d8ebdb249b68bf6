"""Runs tests/cpp/iter_block_amg_capi.cpp (built by rails_amd/csrc/Makefile into rails_amd/lib/iter_block_amg_capi): a program on the C ABI
alone makes a rails_iter (conjugate gradients) for a block-CSR grid operator, turns the block multigrid preconditioner on through
rails_iter_set, runs rails_iter_block_amg_setup, reads rails_iter_block_amg_info, solves, and meets the refusals."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rails_amd", "lib", "iter_block_amg_capi")


@pytest.mark.gpu
def test_c_abi_block_multigrid_preconditioner():
    if not os.path.exists(EXE):
        import rails_amd.build

        rails_amd.build.build()
    p = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("OK"), p.stdout[-4000:]
    assert "unconverged columns 0" in p.stdout and "FAILED" not in p.stdout
