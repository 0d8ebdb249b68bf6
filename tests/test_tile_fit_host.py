"""The switch of the dense kernels' fitted tile counts (rails_dense_set_tile_fit, RAILS_DENSE_TILE_FIT), without a device: declared in
include/rails_hip.h, exported, bound in rails_amd/_lib.py, on by default, off with the variable, and the setter wins over the variable
whether it comes before or after the first use.  The variable is read once per process, so each case is a process of its own that
loads the library alone (no torch, no device)."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "rails_amd", "lib", "librails_hip.so")


def test_declared_exported_and_bound():
    import rails_amd
    import rails_amd._lib as L

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rails_hip.h")).read(), flags=re.S)
    assert re.search(r"\bvoid\s+rails_dense_set_tile_fit\s*\(\s*int\s+on\s*\)\s*;", text)
    assert re.search(r"\bint\s+rails_dense_tile_fit\s*\(\s*void\s*\)\s*;", text)
    assert re.search(r"\bint\s+rails_dense_last_tiles\s*\(\s*const\s+rails_ctx\s*\*\s*ctx\s*,\s*int\s*\*\s*update_gram_nbw\s*,\s*int\s*\*\s*gram_cols_ti\s*,"
                     r"\s*int\s*\*\s*gemm_wide_tr\s*\)\s*;", text)
    ip = C.POINTER(C.c_int)
    assert L.SIGNATURES["rails_dense_set_tile_fit"] == (None, [C.c_int])
    assert L.SIGNATURES["rails_dense_tile_fit"] == (C.c_int, [])
    assert L.SIGNATURES["rails_dense_last_tiles"] == (C.c_int, [C.c_void_p, ip, ip, ip])
    lib = rails_amd.load()
    assert lib.rails_dense_last_tiles(None, None, None, None) != 0 and b"null context" in lib.rails_last_error()


# (variable or None, calls before the value is read; s0 / s1: the setter with 0 / 1, g: a first use) -> the value read at the end
CASES = [(None, "", 1), ("0", "", 0), ("0", "s1", 1), (None, "s0", 0), ("0", "gs1", 1)]


@pytest.mark.parametrize("var,calls,want", CASES)
def test_default_variable_and_setter(var, calls, want):
    prog = ("import ctypes, sys\n"
            "lib = ctypes.CDLL(sys.argv[1])\n"
            "for c in sys.argv[2].split(','):\n"
            "    if c == 'g': lib.rails_dense_tile_fit()\n"
            "    elif c: lib.rails_dense_set_tile_fit(int(c[1]))\n"
            "print(lib.rails_dense_tile_fit())\n")
    env = {k: v for k, v in os.environ.items() if k != "RAILS_DENSE_TILE_FIT"}
    if var is not None:
        env["RAILS_DENSE_TILE_FIT"] = var
    steps = ",".join(re.findall(r"g|s\d", calls))
    out = subprocess.run([sys.executable, "-c", prog, LIB, steps], env=env, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    assert int(out.stdout.strip()) == want
