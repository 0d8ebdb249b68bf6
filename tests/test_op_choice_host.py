"""Which kernel takes a product (rails_amd/csrc/op_choice.h: the whole-operator rule of rails_spmm, serial and halo-overlapped, and what
rails_csr_prepare builds ahead; rails_amd/csrc/row_choice.h: the row-kernel rule), checked on the CPU by a stand-alone program
(tests/cpp/op_choice_host.cpp, built by rails_amd/csrc/Makefile into rails_amd/lib/op_choice_host from the two headers alone: no HIP, no
library)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rails_amd", "lib", "op_choice_host")


def test_kernel_choice_rules_on_the_host():
    if not os.path.exists(EXE):
        import rails_amd.build

        rails_amd.build.build()
    p = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0 and "ALL PASSED" in p.stdout, p.stdout[-4000:]
    assert " 0 failed" in p.stdout
