"""ctypes signatures of include/rails_solution.h."""
import ctypes as C

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_i32p = C.POINTER(C.c_int32)
_vp = C.c_void_p

SOLUTION_SIGNATURES = {
    "rails_panel_move_rows": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _i32p, C.c_int64, C.c_int, _vp, C.c_int]),
    "rails_panel_rowquad": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _dp, C.c_int, _vp, C.c_int]),
    "rails_panel_rowquad_last_plan": (C.c_int, [_vp, _ip, _ip, C.c_int]),
    "rails_panel_rowpair": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _dp, C.c_int, _i32p, _i32p, C.c_int64, _vp, C.c_int]),
    "rails_allreduce_host": (C.c_int, [_vp, _dp, C.c_int64]),
    "rails_panel_corr_scale": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, C.c_int, _dp, _i32p]),
    "rails_solution_pairs": (C.c_int, [_vp, _i32p, _i32p, C.c_int64, _vp, C.c_int]),
    "rails_solution_maps": (C.c_int, [_vp, _i32p, C.c_int, C.c_int, _vp, C.c_int, C.c_int]),
    "rails_solution_create": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _dp, C.c_int, C.c_int, C.POINTER(_vp)]),
    "rails_solution_from_solver": (C.c_int, [_vp, C.POINTER(_vp)]),
    "rails_solution_destroy": (C.c_int, [_vp]),
    "rails_solution_rank": (C.c_int, [_vp]),
    "rails_solution_rows": (C.c_int64, [_vp]),
    "rails_solution_panel": (_vp, [_vp, _ip]),
    "rails_solution_small": (_dp, [_vp]),
    "rails_solution_variance": (C.c_int, [_vp, _vp, C.c_int]),
    "rails_solution_trace": (C.c_int, [_vp, _dp]),
    "rails_solution_apply": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, C.c_int]),
    "rails_solution_eigs": (C.c_int, [_vp, C.c_int, C.c_double, _dp, _vp, _ip]),
    "rails_solution_block": (C.c_int, [_vp, _i32p, C.c_int, _i32p, C.c_int, _dp, C.c_int]),
}


def bind(lib):
    for name, (res, args) in SOLUTION_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
