"""The entry points behind the block's scratch panel, without a device: include/rails_hip.h declares them, the library exports them,
and the ctypes table (rails_amd/_lib.py) binds them with the types the header states -- argument by argument, parsed from the
declaration, so that a parameter added on one side only is caught here and not as a crash on the GPU."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_DP, _VP = C.POINTER(C.c_double), C.c_void_p
# C parameter type (spaces removed) -> ctypes type, as rails_amd/_lib.py writes them
CTYPES = {
    "rails_ctx*": _VP, "rails_panel*": _VP, "constrails_panel*": _VP, "rails_panel**": C.POINTER(_VP),
    "double": C.c_double, "int": C.c_int, "int64_t": C.c_int64, "constdouble*": _DP, "double*": _DP,
}


def _declaration(name):
    """(return type, [parameter types], [parameter names]) of the declaration of `name` in include/rails_hip.h"""
    text = open(os.path.join(ROOT, "include", "rails_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    found = re.findall(r"(\w[\w\s\*]*?)\b%s\s*\(([^)]*)\)\s*;" % re.escape(name), text)
    assert len(found) == 1, (name, found)
    ret, params = found[0]
    types, names = [], []
    for p in params.split(","):
        mt = re.fullmatch(r"\s*(.*?)(\w+)\s*", p, flags=re.S)
        types.append(re.sub(r"\s+", "", mt.group(1)))
        names.append(mt.group(2))
    return re.sub(r"\s+", "", ret), types, names


def _check_binding(name):
    import rails_amd
    import rails_amd._lib as L

    ret, types, names = _declaration(name)
    assert ret == "int"
    res, args = L.SIGNATURES[name]
    assert res is C.c_int
    assert len(args) == len(types), (names, args)
    for a, t, n in zip(args, types, names):
        assert CTYPES[t] is a, (name, n, t, a)
    fn = getattr(rails_amd.load(), name)  # exported, and bound with these types
    assert fn.restype is C.c_int and list(fn.argtypes) == list(args)
    return types, names


def test_update_gram_deferred_out_is_declared_exported_and_bound():
    types, names = _check_binding("rails_update_gram_deferred_out")
    assert names == ["ctx", "alpha", "X", "xc0", "k", "C_host", "ldc", "r", "Y", "yc0", "Yout", "oc0", "r2", "slot"]
    assert types[names.index("Y")] == "constrails_panel*" and types[names.index("Yout")] == "rails_panel*"  # Y is only read


def test_update_gram_deferred_keeps_its_signature():
    """the in-place call is the new one with Yout = Y: same parameters as before, and the new one has exactly two more (Yout, oc0)"""
    types, names = _check_binding("rails_update_gram_deferred")
    assert names == ["ctx", "alpha", "X", "xc0", "k", "C_host", "ldc", "r", "Y", "yc0", "r2", "slot"]
    _, out_names = _check_binding("rails_update_gram_deferred_out")
    assert [n for n in out_names if n not in ("Yout", "oc0")] == names


def test_panel_create_ld_is_declared_exported_and_bound():
    types, names = _check_binding("rails_panel_create_ld")
    assert names == ["ctx", "m_local", "capacity", "ld", "out"]
    _, plain = _check_binding("rails_panel_create")
    assert [n for n in names if n != "ld"] == plain


def test_bad_arguments_are_refused_before_any_device_work():
    """null handles and a leading dimension below the capacity come back as errors (no context exists on a host without a GPU)"""
    import rails_amd

    lib = rails_amd.load()
    h = C.c_void_p()
    assert lib.rails_panel_create_ld(None, 10, 4, 4, C.byref(h)) != 0 and not h.value
    z = (C.c_double * 4)()
    assert lib.rails_update_gram_deferred_out(None, -1.0, None, 0, 2, z, 2, 2, None, 2, None, 0, 2, 0) != 0
    assert b"null argument" in lib.rails_last_error()
