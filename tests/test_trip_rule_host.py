"""What the solver's outer loop decides without computing (rails_amd/include/rails/TripRule.hpp: how a trip ends, how much an expansion
adds and how much room it asks for, the opening capacity, the size of the coordinate back end's basis, the two eigenvalue selections) and
which back end takes a solve (rails_amd/csrc/solve_choice.h), checked on the CPU by a stand-alone program (tests/cpp/trip_rule_host.cpp,
built by rails_amd/csrc/Makefile into rails_amd/lib/trip_rule_host from the two headers alone: no HIP, no library, no LAPACK), and once
more built with the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rails_amd", "lib", "trip_rule_host")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def run(exe):
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0 and "ALL PASSED" in p.stdout, p.stdout[-4000:]
    assert " 0 failed" in p.stdout


def test_trip_rule_on_the_host():
    if not os.path.exists(EXE):
        import rails_amd.build

        rails_amd.build.build()
    run(EXE)


def test_the_same_program_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "trip_rule_host_san")
    # host code only: the program has no device part, and -fno-gpu-sanitize says so to the compiler driver as well
    cmd = [HIPCC, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "rails_amd", "include"),
           "-I" + os.path.join(ROOT, "rails_amd", "csrc"), "-x", "c++", os.path.join(ROOT, "tests", "cpp", "trip_rule_host.cpp"), "-o", exe]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:]
    run(exe)
