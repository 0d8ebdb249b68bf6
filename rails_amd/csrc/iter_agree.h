// iter_agree.h -- what the ranks of a row partition must agree on before an iterative A^-1 object (iter_setup.hip: rails_iter_create) may run: whether the
// Jacobi diagonal exists, the sign of the operator's diagonal, and the two Gershgorin bounds of the polynomial preconditioner.  Ranks
// that disagree run different recurrences, and the all-reduced inner products mean nothing.  The library's only collective is a sum, so
// the values are gathered through it: every rank writes RAILS_AGREE_SLOT doubles into its own slot of a zeroed vector of nranks slots,
// one sum all-reduce follows (zeros plus one value: the value itself, a NaN included), and every rank runs rails_iter_agree on the same
// vector and so reaches the same answer.  No HIP in here: tests/cpp/iter_agree_host.cpp stands alone on it.
#ifndef RAILS_ITER_AGREE_H
#define RAILS_ITER_AGREE_H

constexpr int RAILS_AGREE_SLOT = 4; // state, all-negative, hi_plain, hi_jacobi

// state of a rank: it has a Jacobi diagonal (found stored, nonzero and finite, or given), it has none, or it refuses its arguments (a
// zero in the diagonal it was given, a rectangular block): then every rank refuses, after the collective and not before it
constexpr double RAILS_AGREE_DIAG = 1.0, RAILS_AGREE_NO_DIAG = 0.0, RAILS_AGREE_REFUSED = -1.0;

struct rails_iter_agreed {
    bool refused;     // some rank refused its arguments
    bool jacobi;      // every rank has a diagonal
    double defsign;   // -1 only when every rank's diagonal is there and all negative
    double hi_plain;  // the largest of the ranks' bounds; 0 (none) when a rank has none; a NaN shows
    double hi_jacobi; // the same for D^-1 A; 0 without an agreed diagonal
};

inline void rails_iter_agree_fill(double *slot, double state, bool all_negative, double hi_plain, double hi_jacobi)
{
    slot[0] = state;
    slot[1] = all_negative ? 1.0 : 0.0;
    slot[2] = hi_plain;
    slot[3] = hi_jacobi;
}

// the largest of n bounds at stride RAILS_AGREE_SLOT; a rank without a bound (0) leaves none, a NaN shows
inline double rails_iter_agree_max(const double *first, int nranks)
{
    double hi = 0.0;
    bool none = false;
    for (int r = 0; r < nranks; ++r) {
        const double v = first[r * RAILS_AGREE_SLOT];
        none = none || v == 0.0;
        if (hi == hi && !(v <= hi)) hi = v; // a NaN shows, and stays
    }
    return (none && hi == hi) ? 0.0 : hi;
}

inline rails_iter_agreed rails_iter_agree(const double *slots, int nranks)
{
    rails_iter_agreed a = {false, true, 1.0, 0.0, 0.0};
    bool negative = true;
    for (int r = 0; r < nranks; ++r) {
        const double *s = slots + r * RAILS_AGREE_SLOT;
        a.refused = a.refused || !(s[0] == RAILS_AGREE_DIAG || s[0] == RAILS_AGREE_NO_DIAG);
        a.jacobi = a.jacobi && s[0] == RAILS_AGREE_DIAG;
        negative = negative && s[1] == 1.0;
    }
    a.defsign = (a.jacobi && negative) ? -1.0 : 1.0;
    a.hi_plain = rails_iter_agree_max(slots + 2, nranks);
    a.hi_jacobi = a.jacobi ? rails_iter_agree_max(slots + 3, nranks) : 0.0;
    return a;
}

#endif
