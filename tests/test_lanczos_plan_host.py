"""What the fused residual Lanczos decides without computing (rails_amd/csrc/lanczos_plan.h: the argument checks and their texts, the
instantiation of the pass kernel and its grid, widths and bytes, the layout of the small device block, the side launches' grids and the
assembly of H), checked on the CPU by a stand-alone program (tests/cpp/lanczos_plan_host.cpp, built by rails_amd/csrc/Makefile into
rails_amd/lib/lanczos_plan_host from the header alone: no HIP, no library) against the rules as they stood inside lanczos.hip before the
header, over every value of its ranges, and once more built with the address and undefined-behaviour sanitizers."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rails_amd", "lib", "lanczos_plan_host")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def run(exe):
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0 and "ALL PASSED" in p.stdout, p.stdout[-4000:]
    assert " 0 failed" in p.stdout


def built():
    if not os.path.exists(EXE):
        import rails_amd.build

        rails_amd.build.build()
    return EXE


def test_plan_rules_on_the_host():
    run(built())


def test_the_same_program_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "lanczos_plan_host_san")
    # host code only: the program has no device part, and -fno-gpu-sanitize says so to the compiler driver as well
    cmd = [HIPCC, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "rails_amd", "csrc"), "-x", "c++",
           os.path.join(ROOT, "tests", "cpp", "lanczos_plan_host.cpp"), "-o", exe]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:]
    run(exe)


def test_table_names_every_instantiation_once_per_form():
    p = subprocess.run([built(), "--table"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:]
    rows = [json.loads(line) for line in p.stdout.splitlines()]
    keys = [(r["kernel"], tuple(r["inst"])) for r in rows]
    assert len(keys) == len(set(keys))
    ten = {(1, 1), (1, 2), (1, 4), (2, 1), (2, 2), (2, 4), (3, 1), (3, 2), (4, 1), (4, 2)}
    for kernel in ("k_lanczos_pass", "k_lanczos_pass_sparse"):
        assert sorted(inst for kern, inst in keys if kern == kernel) == sorted(ten), kernel
    assert len(keys) == 20
    # the k a row names reaches its NCH, the first k of that range
    assert all(r["k"] == {1: 0, 2: 129, 3: 257, 4: 385}[r["inst"][0]] for r in rows)
