// What the outer loop of rails::Solver (rails/LyapunovSolver.hpp) decides without computing, as pure functions of plain numbers: how a
// trip ends, how many columns an expansion adds and how much room it asks for, the capacity a solve opens with, the size of the coordinate
// back end's basis, and which eigenvalues a selection picks.  Standard C++ only -- no back-end type, no HIP, no LAPACK, no I/O -- so that
// a stand-alone program (tests/cpp/trip_rule_host.cpp) can walk every rule over its full small range.  The decisions are the
// reference's; each cites the lines it restates.
#ifndef RAILS_TRIPRULE_HPP
#define RAILS_TRIPRULE_HPP

#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

namespace rails
{
namespace trip
{

// What a solve is asked to do; names and defaults of the reference's parameters (src/LyapunovSolver.hpp:27-36).
struct Settings {
    int trip_limit = 1000;            // "Maximum iterations"
    double tolerance = 1e-3;          // "Tolerance": on the residual estimate relative to ||B||^2
    int expand_by = 3;                // "Expand size": residual directions added per trip
    int lanczos_steps = 10;           // "Lanczos iterations"
    int shrink_at = -1;               // "Restart size": space dimension that triggers a shrink (<= 0: never by size)
    int shrink_to = -1;               // "Reduced size": dimension kept (<= 0: whatever passes keep_above)
    int shrink_every = 20;            // "Restart iterations": trips between shrinks (<= 0: never by count)
    double keep_above = 1e-3 * 1e-3;  // "Restart tolerance": |eigenvalue of T| a kept direction must exceed (absolute, :471)
    bool shrink_on_convergence = true; // "Minimize solution space"
    bool warm_start = false;          // "Restart from solution": V holds an orthonormal basis to continue from
    bool shrink_at_start = false;     // "Restart upon start": shrink right after the first projected solve (opts.restart_upon_start)
    double projection_method = 1.0;   // "Projection method": opts.projection_method of matlab/RAILSsolver.m:7-16 (see Projection)
};

// The projection method, opts.projection_method of matlab/RAILSsolver.m:7-16,288-314,520-530: `pair` = the 2.x methods (every
// expansion adds [W, A^-1 W]; else 1.x adds A^-1 W), `start` = the decimal: 1 start from [V0, A^-1 V0] (2.1) or A^-1 V0 (1.1), 2 from
// [B, A^-1 B] or A^-1 B, 3 from V0 as method 1 does.  Method 1 (`start` 0) adds the Ritz vectors W themselves and never uses A^-1.
struct Projection {
    bool pair = false;
    int start = 0;
    bool uses_inverse() const { return start != 0; }
};

// the method named by `value`, false if there is none (1, 1.1, 1.2, 1.3, 2.1, 2.2, 2.3)
inline bool parse_projection(double value, Projection &out)
{
    for (int family = 1; family <= 2; ++family)
        for (int decimal = 0; decimal <= 3; ++decimal) {
            if (family == 2 && decimal == 0) continue;
            if (std::abs(value - (family + 0.1 * decimal)) < 1.5e-8) { // sqrt(eps), the reference's comparison (:293-304)
                out.pair = family == 2;
                out.start = decimal;
                return true;
            }
        }
    return false;
}

// ---- the verdict of a trip ------------------------------------------------------------------------------------------------------------
// Return codes of a solve: the reference's 0 / -1 / 1 (src/LyapunovSolver.hpp:239-240,345) and the two of this library's extensions.
enum Code { Converged = 0, StoppedShort = -1, TripsUsedUp = 1, BudgetSpent = 2, Refused = -2 };

enum Action {
    Finish,      // the run ends here: code 0 (converged) or -1 (out of trips or of dimensions)
    Failed,      // the back end has latched a failure: -1, no point in running on (the caller reports it)
    OutOfBudget, // the bounded run (set_max_trips) has made its trips: 2
    Shrink,      // the space shrinks to the dominant part of the solution; the next trip multiplies nothing
    Expand       // the leading residual directions join the space
};

// Why a shrink: what the verbose line prints.  A restart upon start is none of the first two and prints "trip count", as it always has.
enum ShrinkReason { NoShrink, OnConvergence, SizeLimit, TripCount };
inline const char *text(ShrinkReason r) { return r == OnConvergence ? "converged" : r == SizeLimit ? "size limit" : "trip count"; }

struct Verdict {
    Action action;
    int code;            // for Finish, Failed and OutOfBudget: what solve() returns
    ShrinkReason reason; // for Shrink
    bool converged_once; // the caller's flag, updated
};

// How trip `trip` (0-based) ends once its residual estimate is known.  `width` is the space's dimension, `n` the problem's, `last_shrink`
// the trip of the last shrink (0 before any), `trips_done` the estimates made so far in this solve (trip + 1) and `budget` the bound of
// set_max_trips (<= 0: none).  In this order:
//  1. Stop?  Convergence (:223) ends the run unless the space is to be minimised first: then the first convergence only triggers a shrink
//     and the second one ends it.  Running out of trips or of dimensions ends it either way (:224-241).  When the first convergence falls
//     on the last permitted trip, the shrink is still made and the loop then runs out: the solve returns 1 with the shrunk space.
//  2. A latched failure of the back end, then the trip budget (extensions).  `failed` is asked only here, on a trip that does not finish.
//  3. Shrink (:245-247): by size, by trips since the last shrink, on (first) convergence, or upon start -- opts.restart_upon_start
//     (matlab/RAILSsolver.m:53-57,455): the first trip of a start space of more than one column ends in a shrink.  (A single column --
//     every cold start -- has nothing to give up, and a shrink would only cost it a trip.)
//  4. Else expand.
template <class FailureCheck>
Verdict verdict(Settings const &opt, int trip, int width, int n, int last_shrink, bool converged, bool converged_once, int trips_done, int budget,
                FailureCheck &&failed)
{
    Verdict v = {Expand, 0, NoShrink, converged_once};
    if (converged || trip + 1 >= opt.trip_limit || width >= n) {
        if (converged && opt.shrink_on_convergence && !converged_once)
            v.converged_once = true;
        else {
            v.action = Finish;
            v.code = converged ? Converged : StoppedShort;
            return v;
        }
    }
    if (failed()) {
        v.action = Failed;
        v.code = StoppedShort;
        return v;
    }
    if (budget > 0 && trips_done >= budget) {
        v.action = OutOfBudget;
        v.code = BudgetSpent;
        return v;
    }
    const bool by_size = opt.shrink_at > 0 && width >= opt.shrink_at;
    const bool by_count = opt.shrink_every > 0 && trip - last_shrink >= opt.shrink_every;
    const bool at_start = opt.shrink_at_start && trip == 0 && width > 1;
    if (at_start || by_size || by_count || converged) {
        v.action = Shrink;
        v.reason = converged ? OnConvergence : by_size ? SizeLimit : TripCount;
    }
    return v;
}

// ---- how much room, how much to add ---------------------------------------------------------------------------------------------------
// Columns a solve opens with room for: min(shrink_at or 100, n) (:106), or the caller's columns if those are more.
inline int opening_capacity(Settings const &opt, int width, int n) { return std::max(width, std::min(opt.shrink_at > 0 ? opt.shrink_at : 100, n)); }

// The Ritz vectors of the `add` largest |Ritz values| join V: add = min(expand_by, Ritz values on offer, room up to shrink_at or n)
// (:306-307).  Methods other than 1 replace W by A^-1 W (`replace`, 1.x) or add [W, A^-1 W] (`pair`, 2.x: then at most half the room goes
// to Ritz vectors; with one column of room left only W joins) (matlab/RAILSsolver.m:520-530).  V grows by `grow` columns before the
// orthogonalisation, and where that passes the capacity, the capacity grows by 100 columns at a time (:311-332).
struct Expansion {
    int add;
    bool pair, replace;
    int grow;
    int capacity; // the capacity after this expansion (the one passed in where it suffices)
};
inline Expansion plan_expansion(Settings const &opt, Projection const &proj, int width, int n, int ritz_values, int capacity)
{
    Expansion e;
    const int room = (opt.shrink_at > 0 ? opt.shrink_at : n) - width;
    e.add = std::min(std::min(opt.expand_by, ritz_values), room);
    e.pair = proj.uses_inverse() && proj.pair;
    e.replace = proj.uses_inverse() && !proj.pair;
    if (e.pair && room >= 2)
        e.add = std::min(e.add, room / 2);
    else
        e.pair = false;
    e.grow = e.pair ? 2 * e.add : e.add;
    e.capacity = capacity;
    if (width + e.grow > capacity) e.capacity += std::max(100, width + e.grow - capacity);
    return e;
}

// Rows of the coordinate back end's basis: every panel of a solve (V, AV and what a trip adds to each before a shrink), B's columns and
// slack.  `shrink_at`, `expand_by` as in Settings; `pair`: a 2.x method, which adds twice per trip; `start_columns`: a raw start space's.
inline int coordinate_basis_rows(int shrink_at, int expand_by, bool pair, int start_columns, int rhs_columns)
{
    const int kmax = std::max(shrink_at > 0 ? shrink_at : 100, 1) + (pair ? 2 : 1) * expand_by + 100 + start_columns;
    return 2 * kmax + rhs_columns + 128;
}

// ---- the two selections ---------------------------------------------------------------------------------------------------------------
// Positions of the `count` entries of largest modulus among values[0..m), appended to `positions` in the order the reference's selection
// produces them (src/StlTools.hpp:12-30: std::sort by decreasing |value|; Ritz values come in +- pairs, so ties are common and the order
// among them is whatever that sort yields -- an index sort with the same comparison makes the same moves).
inline void largest_moduli(const double *values, int m, int count, std::vector<int> &positions)
{
    std::vector<int> order(m);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [values](int a, int b) { return std::abs(values[a]) > std::abs(values[b]); });
    positions.insert(positions.end(), order.begin(), order.begin() + count);
}

// The directions a shrink keeps among the k eigenvalues of T: the `count` of largest modulus (<= 0: all k), those above `threshold`
// (absolute) only (:449-482).  One entry of `columns` per candidate: the eigenvalue's position where it passes, -1 where not.  Returns
// the number that pass, which is the width that remains (:468-478).
inline int restart_columns(const double *values, int k, int count, double threshold, std::vector<int> &columns)
{
    const int wanted = count > 0 ? count : k;
    columns.clear();
    largest_moduli(values, k, wanted, columns);
    int kept = 0;
    for (int c = 0; c < wanted; ++c) {
        if (std::abs(values[columns[c]]) > threshold)
            ++kept;
        else
            columns[c] = -1;
    }
    return kept;
}

} // namespace trip
} // namespace rails

#endif
