"""Which dense kernel takes a call (rails_amd/csrc/dense_choice.h: instantiation, slabs, grid and slices of the Gram products, the fused
update + second projection, the panel GEMM and the one-pass wide GEMM), checked on the CPU by a stand-alone program
(tests/cpp/dense_choice_host.cpp, built by rails_amd/csrc/Makefile into rails_amd/lib/dense_choice_host from the header alone: no HIP, no
library) against the launch chains as they stood before the header, over every shape and switch setting of its ranges, and once more built
with the address and undefined-behaviour sanitizers."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rails_amd", "lib", "dense_choice_host")
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


def test_choice_rule_on_the_host():
    run(built())


def test_the_same_program_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "dense_choice_host_san")
    # host code only: the program has no device part, and -fno-gpu-sanitize says so to the compiler driver as well
    cmd = [HIPCC, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "rails_amd", "csrc"), "-x", "c++",
           os.path.join(ROOT, "tests", "cpp", "dense_choice_host.cpp"), "-o", exe]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:]
    run(exe)


def test_table_names_every_instantiation_once():
    p = subprocess.run([built(), "--table"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:]
    rows = [json.loads(line) for line in p.stdout.splitlines()]
    keys = [(r["kernel"], tuple(r["inst"])) for r in rows]
    assert len(keys) == len(set(keys))
    count = {}
    for kernel, _ in keys:
        count[kernel] = count.get(kernel, 0) + 1
    # the tables of dense_choice.h (the program itself checks that what is reached equals them)
    assert count == {"k_gram": 6, "k_gram2": 3, "k_gram_cols": 9, "k_gram_cols2": 9, "k_update_gram": 8, "k_update_gram_p": 8, "k_panel_gemm": 5, "k_panel_gemm2": 2,
                     "k_panel_gemm_wide": 10}
    # a row says which switches it needs; only the older schedule of the fused pass needs one off
    off = [r["kernel"] for r in rows if any(v == 0 for v in r.get("switches", {}).values())]
    assert sorted(set(off)) == ["k_update_gram"] and len(off) == 8
