// What the solver's outer loop decides without computing (rails_amd/include/rails/TripRule.hpp) and which back end takes a solve
// (rails_amd/csrc/solve_choice.h) alone, on the host: no HIP, no library.  Built by rails_amd/csrc/Makefile into
// rails_amd/lib/trip_rule_host, run by tests/test_trip_rule_host.py (which also builds it once more, as host code, under the address and
// undefined-behaviour sanitizers).  Prints ALL PASSED at the end.
//
// The rules the two headers replaced are written out below as they stood inside Run::go(), shrink_due(), shrink(), expand() and open() of
// rails/LyapunovSolver.hpp, in find_largest_eigenvalues() and compute_restart_vectors() (as templates over a matrix class, run here on
// the same arrays), and in rails_solver_solve() and solve_in_coordinates() of solver_capi.cpp (old_*), and the headers' answers are
// compared with them over the ranges of main().  Beside that, named cases for the lines of the reference the rules are cited for.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <numeric>
#include <string>
#include <vector>

#include "rails/TripRule.hpp"
#include "solve_choice.h"

using namespace rails;
using namespace rails::trip;

static long failed = 0, checks = 0;
static char where[256] = "";
#define AT(...) std::snprintf(where, sizeof where, __VA_ARGS__)
#define CHECK(cond)                                                                                                                            \
    do {                                                                                                                                       \
        ++checks;                                                                                                                              \
        if (!(cond)) {                                                                                                                         \
            ++failed;                                                                                                                          \
            if (failed <= 20) std::printf("line %d (%s): %s\n", __LINE__, where, #cond);                                                       \
        }                                                                                                                                      \
    } while (0)

// ------------------------------------------------------------------------------------------------- the rules as they stood ---
// the body of the loop of Run::go() after the estimate, with shrink_due() and the reason shrink() worked out for its message
struct OldVerdict {
    enum What { Finish, Failed, Budget, Shrink, Expand } what;
    int code;
    const char *reason;
    bool converged_once;
    int failure_asked; // times the failure check was called
};
static OldVerdict old_verdict(Settings const &opt_, int trip_, int width, int n_, int last_shrink_, bool converged, bool converged_once_, int trips_,
                              int trip_budget_, bool broken)
{
    OldVerdict v = {OldVerdict::Expand, 0, "", converged_once_, 0};
    if (converged || trip_ + 1 >= opt_.trip_limit || width >= n_) {
        if (converged && opt_.shrink_on_convergence && !converged_once_)
            v.converged_once = true;
        else {
            v.what = OldVerdict::Finish;
            v.code = converged ? 0 : -1;
            return v;
        }
    }
    ++v.failure_asked;
    if (broken) {
        v.what = OldVerdict::Failed;
        v.code = -1;
        return v;
    }
    if (trip_budget_ > 0 && trips_ >= trip_budget_) {
        v.what = OldVerdict::Budget;
        v.code = 2;
        return v;
    }
    const bool at_start = opt_.shrink_at_start && trip_ == 0 && width > 1;
    if (at_start || (opt_.shrink_at > 0 && width >= opt_.shrink_at) || (opt_.shrink_every > 0 && trip_ - last_shrink_ >= opt_.shrink_every) || converged) {
        v.what = OldVerdict::Shrink;
        v.reason = converged ? "converged" : (opt_.shrink_at > 0 && width >= opt_.shrink_at ? "size limit" : "trip count");
    }
    return v;
}

// the arithmetic of expand() and the capacity line of open()
struct OldExpansion {
    int add, grow, capacity;
    bool pair, replace, reserved;
};
static OldExpansion old_expansion(Settings const &opt_, Projection const &proj, int width, int n_, int ritz_values, int capacity_)
{
    const int room = (opt_.shrink_at > 0 ? opt_.shrink_at : n_) - width;
    int add = std::min(std::min(opt_.expand_by, ritz_values), room);
    bool pair = proj.uses_inverse() && proj.pair;
    const bool replace = proj.uses_inverse() && !proj.pair;
    if (pair && room >= 2)
        add = std::min(add, room / 2);
    else
        pair = false;
    const int grow = pair ? 2 * add : add;
    bool reserved = false;
    if (width + grow > capacity_) {
        capacity_ += std::max(100, width + grow - capacity_);
        reserved = true;
    }
    return {add, grow, capacity_, pair, replace, reserved};
}
static int old_opening_capacity(Settings const &opt_, int width, int n_) { return std::max(width, std::min(opt_.shrink_at > 0 ? opt_.shrink_at : 100, n_)); }
static int old_basis_rows(int restart, int expand, bool pair, bool have_start, int start_n, int p)
{
    const int kmax = std::max(restart > 0 ? restart : 100, 1) + (pair ? 2 : 1) * expand + 100 + (have_start ? start_n : 0);
    return 2 * kmax + p + 128;
}

// a column of values behind the two accessors the templates used
struct Column {
    std::vector<double> v;
    int M() const { return (int)v.size(); }
    double operator()(int i) const { return v[i]; }
    double operator()(int i, int) const { return v[i]; }
};
template <class DenseMatrix>
static int old_find_largest_eigenvalues(DenseMatrix const &values, std::vector<int> &positions, int count)
{
    std::vector<int> order(values.M());
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&values](int a, int b) { return std::abs(values(a)) > std::abs(values(b)); });
    positions.insert(positions.end(), order.begin(), order.begin() + count);
    return 0;
}
// the selection inside compute_restart_vectors(): for every candidate column the eigenvector it was filled from (-1: left empty), and the width
template <class DenseMatrix>
static int old_restart_selection(DenseMatrix const &values, int k, int num, double tol, std::vector<int> &filled_from)
{
    const int wanted = num > 0 ? num : k;
    std::vector<int> leading;
    old_find_largest_eigenvalues(values, leading, wanted);
    filled_from.assign(wanted, -1);
    int kept = 0;
    for (int c = 0; c < wanted; ++c) {
        if (!(std::abs(values(leading[c], 0)) > tol)) continue;
        filled_from[c] = leading[c];
        ++kept;
    }
    return kept;
}

// the boolean of rails_solver_solve(), with the option as rails_solver_set_option and rails_solver_create_sparse stored it
static bool old_last_was_subspace(bool option, bool sprhs, bool have_V0, bool have_start, int null_q, bool restart_from_solution)
{
    const bool subspace = option && !sprhs;
    return subspace && !sprhs && (have_V0 || have_start || !restart_from_solution) && !(have_start && null_q > 0);
}

// ------------------------------------------------------------------------------------------------------------ the checks ---
static int asked = 0;
static Verdict ask(Settings const &o, int trip, int width, int n, int last, bool conv, bool once, int done, int budget, bool broken)
{
    asked = 0;
    return verdict(o, trip, width, n, last, conv, once, done, budget, [&]() {
        ++asked;
        return broken;
    });
}

static void verdict_over_the_range()
{
    const int limits[] = {1, 2, 5}, ns[] = {6, 8}, ats[] = {-1, 0, 3, 6}, everys[] = {-1, 0, 1, 3}, budgets[] = {0, 2};
    for (int limit : limits)
        for (int trip = 0; trip <= 5; ++trip)
            for (int n : ns)
                for (int width = 1; width <= 8; ++width)
                    for (int at : ats)
                        for (int every : everys)
                            for (int last = 0; last <= trip; ++last)
                                for (int flags = 0; flags < 32; ++flags)
                                    for (int budget : budgets) {
                                        Settings o;
                                        o.trip_limit = limit;
                                        o.shrink_at = at;
                                        o.shrink_every = every;
                                        o.shrink_on_convergence = flags & 1;
                                        o.shrink_at_start = flags & 2;
                                        const bool conv = flags & 4, once = flags & 8, broken = flags & 16;
                                        const int done = trip + 1;
                                        AT("limit %d trip %d n %d width %d at %d every %d last %d flags %d budget %d", limit, trip, n, width, at, every, last, flags, budget);
                                        const OldVerdict was = old_verdict(o, trip, width, n, last, conv, once, done, budget, broken);
                                        const Verdict is = ask(o, trip, width, n, last, conv, once, done, budget, broken);
                                        CHECK((int)is.action == (int)was.what); // (the two enumerations list the outcomes in one order)
                                        CHECK(is.converged_once == was.converged_once);
                                        CHECK(asked == was.failure_asked);
                                        if (was.what == OldVerdict::Finish || was.what == OldVerdict::Failed || was.what == OldVerdict::Budget) CHECK(is.code == was.code);
                                        if (was.what == OldVerdict::Shrink) CHECK(std::string(text(is.reason)) == was.reason);
                                        if (was.what != OldVerdict::Shrink) CHECK(is.reason == NoShrink);
                                    }
}

static const double methods[7] = {1.0, 1.1, 1.2, 1.3, 2.1, 2.2, 2.3};

static void expansion_over_the_range()
{
    for (double method : methods) {
        Projection proj;
        AT("method %g", method);
        CHECK(parse_projection(method, proj));
        CHECK(proj.pair == (method > 2.0) && proj.start == (int)std::lround(10.0 * (method - std::floor(method))));
        for (int expand : {1, 3, 5})
            for (int ritz : {2, 10})
                for (int at : {-1, 12})
                    for (int n : {12, 40})
                        for (int room = 1; room <= 12; ++room) {
                            const int width = (at > 0 ? at : n) - room;
                            if (width < 1) continue;
                            Settings o;
                            o.expand_by = expand;
                            o.shrink_at = at;
                            const OldExpansion probe = old_expansion(o, proj, width, n, ritz, 1 << 20);
                            const int need = width + probe.grow;
                            for (int capacity : {need, need - 1, std::max(need - 150, 1), need + 7}) { // exactly at, one below, far below, above
                                AT("method %g expand %d ritz %d at %d n %d room %d capacity %d", method, expand, ritz, at, n, room, capacity);
                                const OldExpansion was = old_expansion(o, proj, width, n, ritz, capacity);
                                const Expansion is = plan_expansion(o, proj, width, n, ritz, capacity);
                                CHECK(is.add == was.add && is.grow == was.grow && is.pair == was.pair && is.replace == was.replace);
                                CHECK(is.capacity == was.capacity);
                                CHECK((is.capacity != capacity) == was.reserved); // expand() reserves exactly when the old test fired
                                CHECK(width + is.grow <= is.capacity);
                            }
                        }
    }
    Projection none;
    for (double bad : {0.0, 1.05, 1.4, 2.0, 2.4, 3.0, -1.0}) {
        AT("method %g", bad);
        CHECK(!parse_projection(bad, none));
    }
    for (int at : {-1, 0, 3, 100, 250})
        for (int n : {6, 99, 100, 101, 1000})
            for (int width : {1, 5, 150}) {
                Settings o;
                o.shrink_at = at;
                AT("opening at %d n %d width %d", at, n, width);
                CHECK(opening_capacity(o, width, n) == old_opening_capacity(o, width, n));
            }
    for (int restart : {-1, 0, 1, 32, 500})
        for (int expand : {1, 3, 50})
            for (int pair = 0; pair < 2; ++pair)
                for (int start : {0, 7})
                    for (int p : {1, 16}) {
                        AT("basis restart %d expand %d pair %d start %d p %d", restart, expand, pair, start, p);
                        CHECK(coordinate_basis_rows(restart, expand, pair, start, p) == old_basis_rows(restart, expand, pair, start > 0, start, p));
                    }
}

static void selections()
{
    const std::vector<std::vector<double>> columns = {
        {3.0, -3.0, 1.0, -1.0, 0.5, -0.5, 2.0, -2.0, 0.0, 0.0},                        // +- pairs, as Ritz values of the residual come
        {1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0},                                      // all tied
        {-2.0, 2.0, -2.0, 2.0, 5.0, 1e-9, -1e-9, 0.0, 5.0, -5.0, 2.0, 1e-3, -1e-3},    // ties of three and four
        {0.25},
        {1e-7, -4.0, 4.0, 1e-5, -1e-5, 4.0, 3.0, 3.0, -3.0, 1e-6, 2.0, -2.0, 2.0, -2.0, 2.0, -2.0, 2.0, -2.0, 1.0, 0.5, -0.5, 0.5, 7.0, -7.0}, // past the sort's small-range threshold
    };
    for (size_t which = 0; which < columns.size(); ++which) {
        Column col{columns[which]};
        const int m = col.M();
        for (int count = 0; count <= m; ++count) {
            AT("column %zu count %d", which, count);
            std::vector<int> was = {-7}, is = {-7}; // both append
            old_find_largest_eigenvalues(col, was, count);
            largest_moduli(col.v.data(), m, count, is);
            CHECK(was == is);
            CHECK((int)is.size() == count + 1 && is[0] == -7);
        }
        for (int count = -1; count <= m; ++count)
            for (double tol : {0.0, 1e-6, 0.75, 2.0, 10.0}) {
                AT("column %zu restart count %d tol %g", which, count, tol);
                std::vector<int> was, is = {99};
                const int kept_was = old_restart_selection(col, m, count, tol, was);
                const int kept_is = restart_columns(col.v.data(), m, count, tol, is);
                CHECK(kept_was == kept_is);
                CHECK(was == is);
            }
    }
}

static void backend_choice()
{
    for (int flags = 0; flags < 32; ++flags)
        for (int null_q : {0, 2}) {
            const bool option = flags & 1, sparse = flags & 2, v = flags & 4, start = flags & 8, restart = flags & 16;
            AT("flags %d nullspace %d", flags, null_q);
            CHECK((choose_backend(option, sparse, v, start, null_q, restart) == CoordinateBackend) == old_last_was_subspace(option, sparse, v, start, null_q, restart));
        }
    // the rows by name
    AT("rows");
    CHECK(choose_backend(true, false, false, false, 0, false) == CoordinateBackend); // default
    CHECK(choose_backend(false, false, false, false, 0, false) == DirectBackend);    // subspace = 0
    CHECK(choose_backend(true, true, false, false, 0, false) == DirectBackend);      // sparse B
    CHECK(choose_backend(true, false, true, false, 0, true) == CoordinateBackend);   // caller's V
    CHECK(choose_backend(true, false, true, false, 2, true) == CoordinateBackend);   // caller's V with a nullspace
    CHECK(choose_backend(true, false, false, true, 0, false) == CoordinateBackend);  // start space
    CHECK(choose_backend(true, false, false, true, 2, false) == DirectBackend);      // start space with a nullspace
    CHECK(choose_backend(true, false, false, false, 0, true) == DirectBackend);      // "Restart from solution" without a V
}

// the whole loop of go() over a scripted sequence of (converged) flags, widths following the verdicts: the code solve() returns
static int run_loop(Settings const &o, int n, int start_width, std::vector<bool> const &converged_at, int budget, std::vector<Action> *trace = nullptr)
{
    int width = start_width, last_shrink = 0, trips = 0;
    bool once = false;
    for (int trip = 0; trip < o.trip_limit; ++trip) {
        ++trips;
        const bool conv = trip < (int)converged_at.size() && converged_at[trip];
        const Verdict v = ask(o, trip, width, n, last_shrink, conv, once, trips, budget, false);
        once = v.converged_once;
        if (trace) trace->push_back(v.action);
        if (v.action == Finish || v.action == Failed || v.action == OutOfBudget) return v.code;
        if (v.action == Shrink) {
            width = std::max(1, o.shrink_to > 0 ? std::min(o.shrink_to, width) : width);
            last_shrink = trip;
        } else
            width += plan_expansion(o, Projection(), width, n, o.lanczos_steps, 1 << 20).add;
    }
    return TripsUsedUp;
}

static void named_cases()
{
    Settings o; // the defaults: minimise the space, shrink every 20 trips
    // src/LyapunovSolver.hpp:223-241 -- convergence ends the run, unless the space is to be minimised first
    AT(":223-241");
    o.shrink_on_convergence = false;
    Verdict v = ask(o, 3, 5, 20, 0, true, false, 4, 0, false);
    CHECK(v.action == Finish && v.code == 0 && asked == 0);
    o.shrink_on_convergence = true;
    v = ask(o, 3, 5, 20, 0, true, false, 4, 0, false);
    CHECK(v.action == Shrink && v.reason == OnConvergence && v.converged_once && asked == 1);
    v = ask(o, 4, 5, 20, 3, true, true, 5, 0, false);
    CHECK(v.action == Finish && v.code == 0);
    // out of trips (iter + 1 >= max_iter) and out of dimensions (V.N() >= n): -1
    o.trip_limit = 4;
    v = ask(o, 3, 5, 20, 0, false, false, 4, 0, false);
    CHECK(v.action == Finish && v.code == -1);
    o.trip_limit = 1000;
    v = ask(o, 3, 20, 20, 0, false, false, 4, 0, false);
    CHECK(v.action == Finish && v.code == -1);
    // :245-247 -- shrink by size, by trips since the last shrink; else expand
    AT(":245-247");
    o.shrink_at = 6;
    v = ask(o, 3, 6, 20, 0, false, false, 4, 0, false);
    CHECK(v.action == Shrink && v.reason == SizeLimit);
    v = ask(o, 3, 5, 20, 0, false, false, 4, 0, false);
    CHECK(v.action == Expand);
    o.shrink_at = -1;
    v = ask(o, 25, 9, 40, 5, false, false, 26, 0, false);
    CHECK(v.action == Shrink && v.reason == TripCount);
    v = ask(o, 24, 9, 40, 5, false, false, 25, 0, false);
    CHECK(v.action == Expand);
    // the extensions, in their order: a latched failure before the budget, neither on a trip that finishes
    AT("extensions");
    v = ask(o, 2, 5, 20, 0, false, false, 3, 3, true);
    CHECK(v.action == Failed && v.code == -1);
    v = ask(o, 2, 5, 20, 0, false, false, 3, 3, false);
    CHECK(v.action == OutOfBudget && v.code == 2);
    v = ask(o, 2, 5, 20, 0, false, false, 3, 4, false);
    CHECK(v.action == Expand);
    // :306-307 -- expand_vectors = min(min(expand_size, eigenvalues.M()), (restart_size > 0 ? restart_size : n) - V.N())
    AT(":306-307");
    Settings e;
    Expansion x = plan_expansion(e, Projection(), 4, 20, 10, 100);
    CHECK(x.add == 3 && x.grow == 3 && !x.pair && !x.replace && x.capacity == 100);
    x = plan_expansion(e, Projection(), 4, 20, 2, 100);
    CHECK(x.add == 2);
    x = plan_expansion(e, Projection(), 18, 20, 10, 100);
    CHECK(x.add == 2);
    e.shrink_at = 19;
    x = plan_expansion(e, Projection(), 18, 20, 10, 100);
    CHECK(x.add == 1);
    // :311-332 -- room for 100 more columns at a time
    x = plan_expansion(Settings(), Projection(), 99, 400, 10, 100);
    CHECK(x.add == 3 && x.capacity == 200);
    // matlab/RAILSsolver.m:520-530 -- 1.x replaces W by A^-1 W, 2.x adds [W, A^-1 W] in half the room; one column of room: W alone
    AT("RAILSsolver.m:520-530");
    Projection p11, p21;
    CHECK(parse_projection(1.1, p11) && parse_projection(2.1, p21));
    e = Settings();
    x = plan_expansion(e, p11, 4, 20, 10, 100);
    CHECK(x.add == 3 && x.grow == 3 && x.replace && !x.pair);
    x = plan_expansion(e, p21, 4, 20, 10, 100);
    CHECK(x.add == 3 && x.grow == 6 && x.pair && !x.replace);
    x = plan_expansion(e, p21, 15, 20, 10, 100); // room 5: two pairs
    CHECK(x.add == 2 && x.grow == 4 && x.pair);
    x = plan_expansion(e, p21, 19, 20, 10, 100); // room 1
    CHECK(x.add == 1 && x.grow == 1 && !x.pair && !x.replace);
    // matlab/RAILSsolver.m:455 -- `i == 1 && restart_upon_start`: the first trip of a start space ends in a shrink, printed as "trip count"
    AT("RAILSsolver.m:455");
    o = Settings();
    o.shrink_at_start = true;
    v = ask(o, 0, 7, 20, 0, false, false, 1, 0, false);
    CHECK(v.action == Shrink && v.reason == TripCount && std::string(text(v.reason)) == "trip count");
    v = ask(o, 1, 7, 20, 0, false, false, 2, 0, false);
    CHECK(v.action == Expand);
    // a single start column with restart upon start: nothing to give up, the trip expands
    AT("single column, restart upon start");
    v = ask(o, 0, 1, 20, 0, false, false, 1, 0, false);
    CHECK(v.action == Expand);
    // first convergence on the last permitted trip: the shrink is made, the loop runs out, solve() returns 1
    AT("first convergence on the last permitted trip");
    o = Settings();
    o.trip_limit = 3;
    v = ask(o, 2, 7, 20, 0, true, false, 3, 0, false);
    CHECK(v.action == Shrink && v.reason == OnConvergence && v.converged_once);
    std::vector<Action> trace;
    CHECK(run_loop(o, 20, 1, {false, false, true}, 0, &trace) == TripsUsedUp);
    CHECK(trace.size() == 3 && trace[0] == Expand && trace[1] == Expand && trace[2] == Shrink);
    CHECK(run_loop(o, 20, 1, {false, true, true}, 0) == Converged); // one trip earlier: shrink, then the second convergence ends it
    CHECK(run_loop(o, 20, 1, {false, false, false}, 0) == StoppedShort);
    CHECK(run_loop(o, 20, 1, {false, false, false}, 2) == BudgetSpent);
    o.trip_limit = 1; // a trip limit of 1: the first trip finishes, converged or not -- unless it is a first convergence to be minimised
    CHECK(run_loop(o, 20, 1, {false}, 0) == StoppedShort);
    CHECK(run_loop(o, 20, 1, {true}, 0) == TripsUsedUp);
    o.shrink_on_convergence = false;
    CHECK(run_loop(o, 20, 1, {true}, 0) == Converged);
}

int main()
{
    verdict_over_the_range();
    expansion_over_the_range();
    selections();
    backend_choice();
    named_cases();
    std::printf("%ld checks, %ld failed\n", checks, failed);
    if (failed == 0) std::printf("ALL PASSED\n");
    return failed ? 1 : 0;
}
