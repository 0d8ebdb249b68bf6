"""What the projected Lyapunov solve decides without computing (rails_amd/csrc/lyap_route.h: the gates of the four routes, which of the
iterative routes a call attempts and how long a failed one rests, whether the factored ADI route may build on the call before, Wachspress'
shifts), checked on the CPU by a stand-alone program (tests/cpp/lyap_route_host.cpp, built by rails_amd/csrc/Makefile into
rails_amd/lib/lyap_route_host from the header alone: no HIP, no library, no LAPACK), and once more built with the address and
undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rails_amd", "lib", "lyap_route_host")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def run(exe):
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0 and "ALL PASSED" in p.stdout, p.stdout[-4000:]
    assert " 0 failed" in p.stdout


def test_route_rule_on_the_host():
    if not os.path.exists(EXE):
        import rails_amd.build

        rails_amd.build.build()
    run(EXE)


def test_the_same_program_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "lyap_route_host_san")
    # host code only: the program has no device part, and -fno-gpu-sanitize says so to the compiler driver as well
    cmd = [HIPCC, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "rails_amd", "csrc"), "-x", "c++",
           os.path.join(ROOT, "tests", "cpp", "lyap_route_host.cpp"), "-o", exe]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:]
    run(exe)
