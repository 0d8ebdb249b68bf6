"""The switch of the fused update + second projection's schedule (rails_dense_set_update_gram_pipeline, RAILS_UPDATE_GRAM_PIPELINE),
without a device: declared in include/rails_hip.h, exported, bound in rails_amd/_lib.py, on by default, off with the variable, and the
setter wins over the variable whether it comes before or after the first use.  The variable is read once per process, so each case is
a process of its own that loads the library alone (no torch, no device)."""
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
    assert re.search(r"\bvoid\s+rails_dense_set_update_gram_pipeline\s*\(\s*int\s+on\s*\)\s*;", text)
    assert re.search(r"\bint\s+rails_dense_update_gram_pipeline\s*\(\s*void\s*\)\s*;", text)
    assert re.search(r"\bint\s+rails_dense_last_update_gram_form\s*\(\s*const\s+rails_ctx\s*\*\s*ctx\s*,\s*int\s*\*\s*form\s*\)\s*;", text)
    assert L.SIGNATURES["rails_dense_set_update_gram_pipeline"] == (None, [C.c_int])
    assert L.SIGNATURES["rails_dense_update_gram_pipeline"] == (C.c_int, [])
    assert L.SIGNATURES["rails_dense_last_update_gram_form"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_int)])
    lib = rails_amd.load()
    form = C.c_int(-1)
    assert lib.rails_dense_last_update_gram_form(None, C.byref(form)) != 0 and b"null argument" in lib.rails_last_error()


# (variable or None, calls before the value is read; s0 / s1: the setter with 0 / 1, g: a first use) -> the value read at the end
CASES = [(None, "", 1), ("0", "", 0), ("1", "", 1), ("0", "s1", 1), (None, "s0", 0), ("0", "gs1", 1), (None, "gs0", 0)]


@pytest.mark.parametrize("var,calls,want", CASES)
def test_default_variable_and_setter(var, calls, want):
    prog = ("import ctypes, sys\n"
            "lib = ctypes.CDLL(sys.argv[1])\n"
            "for c in sys.argv[2].split(','):\n"
            "    if c == 'g': lib.rails_dense_update_gram_pipeline()\n"
            "    elif c: lib.rails_dense_set_update_gram_pipeline(int(c[1]))\n"
            "print(lib.rails_dense_update_gram_pipeline())\n")
    env = {k: v for k, v in os.environ.items() if k != "RAILS_UPDATE_GRAM_PIPELINE"}
    if var is not None:
        env["RAILS_UPDATE_GRAM_PIPELINE"] = var
    steps = ",".join(re.findall(r"g|s\d", calls))
    out = subprocess.run([sys.executable, "-c", prog, LIB, steps], env=env, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    assert int(out.stdout.strip()) == want
