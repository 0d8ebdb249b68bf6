// Which back end takes a solve of the C ABI (include/rails_solver.h; rails_solver_solve in solver_capi.cpp): the direct one
// (rails/HipWrappers.hpp: every multivector a device panel) or the coordinate-space one (rails/SubspaceWrappers.hpp: every multivector
// as coordinates in one orthonormal device basis).  One pure function of six facts about the solve; standard C++ only, checked over all
// its inputs by tests/cpp/trip_rule_host.cpp.
#ifndef RAILS_SOLVE_CHOICE_H
#define RAILS_SOLVE_CHOICE_H

namespace rails
{

enum SolveBackend { DirectBackend, CoordinateBackend };

// The coordinate back end is the default and takes every solve it can express:
//  * `subspace_option` (rails_solver_set_option "subspace", default 1): 0 asks for the direct back end.
//  * `sparse_b` (rails_solver_create_sparse): the coordinate back end needs B inside its basis, as a panel it can absorb; B as an
//    operator has no columns to absorb, so such a solver always runs the direct back end and the option is accepted and ignored.
//  * `restart_from_solution` (the parameter "Restart from solution") without a space to start from -- neither `caller_v`
//    (rails_solver_set_V) nor `start_space` (rails_solver_set_start_space): a warm start needs the caller's V; without one it is the
//    direct back end's business, which starts from the column the solver object holds, like the reference.  (After a solve V holds the
//    result, and a later warm start that passes no V continues from it there.)
//  * `start_space` together with `nullspace_columns` > 0: the direct back end, whose orthonormalisation of the raw start space projects
//    the nullspace out as it goes, column block by column block; the coordinate back end orthonormalises the start space before it is
//    absorbed, without the nullspace.  (A caller's V with a nullspace, or a cold start with one, stays on the coordinate back end.)
inline SolveBackend choose_backend(bool subspace_option, bool sparse_b, bool caller_v, bool start_space, int nullspace_columns, bool restart_from_solution)
{
    if (!subspace_option || sparse_b) return DirectBackend;
    if (restart_from_solution && !caller_v && !start_space) return DirectBackend;
    if (start_space && nullspace_columns > 0) return DirectBackend;
    return CoordinateBackend;
}

} // namespace rails

#endif
