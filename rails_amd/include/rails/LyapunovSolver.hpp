// rails::Solver<Matrix, MultiVector, DenseMatrix> -- the RAILS outer loop for the duck-typed backend contract of the
// reference (src/LyapunovSolverDecl.hpp:9-51).  The public surface is the reference's -- constructor (A, B, M),
// set_parameters, solve(V, T), dense_solve, resid_lanczos, compute_restart_vectors, the same parameter names and defaults
// (src/LyapunovSolver.hpp:27-36,76-87) and return codes (0 converged / -1 stopped without converging / 1 trips used up,
// :239-240,345; set_parameters 0 / 1, :89-97) -- and every DECISION is the reference's, cited where it is taken:
// convergence (:223), when to stop (:224-241), when to shrink the space (:245-247), how many vectors to add (:306-307),
// which (:336-339).  What a trip decides without computing -- how it ends, how much an expansion adds, which eigenvalues a selection
// picks -- is rails/TripRule.hpp: pure functions, checked alone on the host.  The organisation is this library's own: a solve is a Run
// object that owns the search space (V, A V, M V, B'V), the reduced matrices (V'AV, V'BB'V, V'MV) and the settings, and advances by
// trips of four steps --
//
//     border    A (and M) applied to the columns added last; the reduced matrices get their new border
//     reduce    the projected Lyapunov equation, on the host (rails_sb03md)
//     estimate  largest Ritz values / vectors of the residual operator (Lanczos)
//     adapt     stop, shrink the space to the dominant part of the solution, or add the leading residual directions
//
// Three customisation points (struct SolverOps, specialised in rails/HipSolverOps.hpp and rails/SubspaceSolverOps.hpp) let a
// backend replace member-by-member sequences by fused work: apply_append (A W straight into AV's tail), lanczos (the
// residual estimate) and multiply_inplace (V <- V X when the space shrinks).
// Unlike the reference's C++ (which stores M and never reads it, src/LyapunovSolver.hpp:26) a mass matrix can be switched
// on with use_mass_matrix(true); the generalized iteration follows matlab/RAILSsolver.m:368-395,499-504.
#ifndef RAILS_LYAPUNOVSOLVER_HPP
#define RAILS_LYAPUNOVSOLVER_HPP

#include <algorithm>
#include <cctype>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <iostream>
#include <map>
#include <numeric>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "rails/TripRule.hpp"
#include "rails_hip.h"

namespace rails
{

// Whether a MultiVector offers `orthogonalize(MultiVector const &N)`: the columns past its watermark orthonormalised against the orthonormal
// columns of N and against all columns before them, with N projected out inside every round (a back end's own deflated orthogonalisation).
template <class MultiVector, class = void>
struct has_deflated_orthogonalize : std::false_type {
};
template <class MultiVector>
struct has_deflated_orthogonalize<MultiVector, decltype(std::declval<MultiVector &>().orthogonalize(std::declval<MultiVector const &>()), void())>
    : std::true_type {
};

// V's columns from `first` on, orthonormalised against N and against V's columns before `first`.  A back end with the deflated member does it
// itself; any other goes through the contract: twice "project N out of the new columns, move the watermark back to `first`, orthogonalize()",
// so that what orthogonalize() invents for a dependent column (normalised rounding noise) loses its part along N as well.
template <class MultiVector>
void orthogonalize_deflated(MultiVector &V, MultiVector const &N, int first, std::true_type)
{
    const int n = V.N();
    V.resize(first); // (the contract's resize keeps the data: this only moves the watermark)
    V.resize(n);
    V.orthogonalize(N);
}
template <class MultiVector>
void orthogonalize_deflated(MultiVector &V, MultiVector const &N, int first, std::false_type)
{
    const int n = V.N();
    if (n <= first) return;
    for (int round = 0; round < 2; ++round) {
        MultiVector W = V.view(first, n - 1);
        W -= N * N.dot(W);
        V.resize(first);
        V.resize(n);
        V.orthogonalize();
    }
}

// Whether a MultiVector offers `int orthogonalize_range(MultiVector const *N, double tol)`: ALL its columns, which need be neither
// orthonormal nor independent, replaced by an orthonormal basis of their range with N (orthonormal columns; null: none) projected out,
// in column order; the object is resized to the columns kept, marks them orthogonalised and returns their number.
template <class MultiVector, class = void>
struct has_range_orthogonalize : std::false_type {
};
template <class MultiVector>
struct has_range_orthogonalize<MultiVector,
                               decltype(std::declval<MultiVector &>().orthogonalize_range(std::declval<MultiVector const *>(), std::declval<double>()), void())>
    : std::true_type {
};

// `V = Morth(V0, [], nullspace, [])` for a start space V0 = opts.space (matlab/RAILSsolver.m:160-204,310-314,567-580): every column is
// scaled to unit length, loses -- twice -- its part along N and along the columns kept before it, and is dropped when less than `tol` of
// it survives (a column of norm zero, or not finite, is dropped too); the later columns move up.  Returns the columns kept.
// A back end with the member does it itself; any other goes through the contract, column by column, like Solver::prepare_nullspace.  The
// contract moves a watermark only in orthogonalize(), so the generic form ends with one such call on the columns it kept: they are
// orthonormal by then and stay what they are up to rounding.
template <class MultiVector>
int orthogonalize_range(MultiVector &V, MultiVector const *N, double tol, std::true_type)
{
    const int n = V.N();
    V.resize(0); // from column 0 (the contract's resize keeps the data: this only moves the watermark)
    V.resize(n);
    return V.orthogonalize_range(N, tol);
}
template <class MultiVector>
int orthogonalize_range(MultiVector &V, MultiVector const *N, double tol, std::false_type)
{
    int n = V.N(), j = 0;
    while (j < n) {
        MultiVector v = V.view(j);
        const double n0 = v.norm();
        double nrm = 0.0;
        if (n0 > 0.0 && std::isfinite(n0)) {
            v /= n0;
            for (int pass = 0; pass < 2; ++pass) {
                if (N) v -= *N * N->dot(v);
                if (j > 0) {
                    MultiVector const before = V.view(0, j - 1);
                    v -= before * before.dot(v);
                }
            }
            nrm = v.norm();
        }
        if (!(nrm >= tol)) { // nothing new in this column: the later ones move up
            for (int l = j + 1; l < n; ++l) V.view(l - 1) = V.view(l);
            V.resize(--n);
            continue;
        }
        v /= nrm;
        ++j;
    }
    if (n > 0) {
        V.resize(0); // (the watermark goes back to the first column)
        V.resize(n);
        V.orthogonalize();
    }
    return n;
}

// The right-hand side factor B, given either as an operator (Matrix) or as a tall panel (MultiVector) -- the two forms the
// reference accepts through its B adaptor (src/MatrixOrMultiVectorWrapper.hpp:7-98).  Both members exist (the contract asks
// for default-constructible types, :11-12); `kind_` says which one is in use.
template <class Matrix, class MultiVector>
class BOperand
{
public:
    enum Kind { Operator, Panel };

    BOperand(Matrix const &op) : kind_(Operator), op_(op) {}
    BOperand(MultiVector const &panel) : kind_(Panel), panel_(panel) {}

    bool given_as_operator() const { return kind_ == Operator; }
    MultiVector const &panel() const { return panel_; }
    Matrix const &op() const { return op_; }
    // ||B||_2, the scale of the stopping test (src/LyapunovSolver.hpp:134)
    double norm2() const { return kind_ == Operator ? op_.norm() : panel_.norm(); }
    // B X and B'X
    MultiVector times(MultiVector const &X) const { return kind_ == Operator ? op_ * X : panel_ * X; }
    MultiVector transposed_times(MultiVector const &X) const { return kind_ == Operator ? op_.transpose() * X : panel_.transpose() * X; }

private:
    Kind kind_;
    Matrix op_;
    MultiVector panel_;
};

// One class plays both roles (the Stl-style backends, src/StlWrapper.hpp): there is nothing to choose.
template <class Both>
class BOperand<Both, Both>
{
public:
    BOperand(Both const &b) : b_(b) {}
    bool given_as_operator() const { return false; }
    Both const &panel() const { return b_; }
    Both const &op() const { return b_; }
    double norm2() const { return b_.norm(); }
    Both times(Both const &X) const { return b_ * X; }
    Both transposed_times(Both const &X) const { return b_.transpose() * X; }

private:
    Both b_;
};

// a column of values as a plain array, for the selections of rails/TripRule.hpp
template <class DenseMatrix>
std::vector<double> plain_values(DenseMatrix const &values)
{
    std::vector<double> plain(values.M());
    for (int i = 0; i < values.M(); ++i) plain[i] = values(i);
    return plain;
}

// Positions of the `count` entries of largest modulus, in the order the reference's selection produces them (trip::largest_moduli).
template <class DenseMatrix>
int find_largest_eigenvalues(DenseMatrix const &values, std::vector<int> &positions, int count)
{
    const std::vector<double> plain = plain_values(values);
    trip::largest_moduli(plain.data(), (int)plain.size(), count, positions);
    return 0;
}

// A parameter under any of the spellings the reference accepts (src/LyapunovSolver.hpp:40-70): as written, upper case,
// lower case, and capitalised words; later spellings override earlier ones.
template <class ParameterList, class Value>
Value lookup_parameter(ParameterList &params, std::string const &name, Value fallback)
{
    std::string upper(name), lower(name), title(name);
    bool word_start = true;
    for (size_t i = 0; i < name.size(); ++i) {
        const unsigned char ch = (unsigned char)name[i];
        upper[i] = (char)std::toupper(ch);
        lower[i] = (char)std::tolower(ch);
        title[i] = word_start ? (char)std::toupper(ch) : name[i];
        word_start = !std::isalpha(ch);
    }
    Value value = fallback;
    const std::string *spellings[4] = {&name, &upper, &lower, &title};
    for (const std::string *spelling : spellings) value = params.get(*spelling, value);
    return value;
}

// Wall-clock time per part of a trip, under the section names of the reference's profiler (src/Timer.hpp:101-106), so that
// reports stay comparable.  Host time between synchronisation points; the device side is profiled with rocprofv3.
class ScopedTimer
{
    double *slot_;
    std::chrono::steady_clock::time_point start_;

public:
    ScopedTimer(std::map<std::string, double> *sections, const char *name) : slot_(&(*sections)[name]), start_(std::chrono::steady_clock::now()) {}
    ~ScopedTimer() { *slot_ += std::chrono::duration<double>(std::chrono::steady_clock::now() - start_).count(); }
};

// RAILS_SOLVER_TRIP_TRACE=x: after every trip that took more than x ms, its time per section on stderr.  lap() at the start of every trip.
class TripTrace
{
    std::map<std::string, double> before_;
    std::chrono::steady_clock::time_point start_ = std::chrono::steady_clock::now();

public:
    void lap(int trip, std::map<std::string, double> const &sections)
    {
        static const double trace_ms = getenv("RAILS_SOLVER_TRIP_TRACE") ? atof(getenv("RAILS_SOLVER_TRIP_TRACE")) : 0.0;
        if (!(trace_ms > 0.0)) return;
        const double ms = 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - start_).count();
        if (trip > 0 && ms > trace_ms) {
            std::cerr << "[rails trip " << trip << "] " << ms << " ms:";
            for (auto const &kv : sections) std::cerr << " " << kv.first << " " << 1e3 * (kv.second - before_[kv.first]);
            std::cerr << std::endl;
        }
        before_ = sections;
        start_ = std::chrono::steady_clock::now();
    }
};

template <class Matrix, class MultiVector, class DenseMatrix>
class Solver;

// ---- customisation points; the generic versions go through the backend contract member by member -----------------------
// SolverOps<...> is what the solver calls; it derives from GenericSolverOps, and a back end's specialisation does too and redefines
// the members it replaces.
template <class Matrix, class MultiVector, class DenseMatrix>
struct GenericSolverOps {
    typedef Solver<Matrix, MultiVector, DenseMatrix> SolverT;

    // result of one residual estimate: Ritz values and a way to append selected Ritz vectors to V
    struct Lanczos {
        DenseMatrix eigenvalues;
        MultiVector eigenvectors;
        void append_to(MultiVector &V, std::vector<int> const &indices, int count) const
        {
            for (auto it = indices.begin(); it != indices.begin() + count; ++it) V.push_back(eigenvectors.view(*it)); // src/LyapunovSolver.hpp:338-339
        }
    };

    // AV <- [AV, A*W]; returns A*W                                        (src/LyapunovSolver.hpp:146,203)
    static MultiVector apply_append(Matrix const &A, MultiVector const &W, MultiVector &AV)
    {
        MultiVector AW = A * W;
        AV.push_back(AW);
        return AW;
    }

    // per-solve scratch of the backend (nothing for the generic form)
    struct State {
    };

    // the residual estimate by Solver::resid_lanczos, into any result that has `eigenvalues` and `eigenvectors`
    template <class Result>
    static int lanczos_by_members(SolverT &solver, MultiVector const &AV, MultiVector const &MV, DenseMatrix const &T, int max_iter, Result &out)
    {
        DenseMatrix H(max_iter + 1, max_iter + 1);
        out.eigenvalues = DenseMatrix(max_iter, 1);
        return solver.resid_lanczos(AV, MV, T, H, out.eigenvectors, out.eigenvalues, max_iter);
    }

    // VAV and BV (the reduced operator and B'V) are passed along for backends that can use them
    static int lanczos(SolverT &solver, State &, MultiVector const &AV, MultiVector const &MV, DenseMatrix const &T, DenseMatrix const &,
                       MultiVector const &, int max_iter, Lanczos &out)
    {
        return lanczos_by_members(solver, AV, MV, T, max_iter, out);
    }

    // after V <- V X and AV <- AV X (:265-291)
    static void on_restart(State &, DenseMatrix const &, MultiVector &, MultiVector &) {}

    // V <- V * X (first X.N() columns), as `V.view(0, X.N()-1) = V * X; V.resize(X.N())`   (:265-266)
    static void multiply_inplace(MultiVector &V, DenseMatrix const &X)
    {
        const int kept = X.N();
        MultiVector product = V * X;
        V.view(0, kept - 1) = product;
        V.resize(kept);
    }
};

template <class Matrix, class MultiVector, class DenseMatrix>
struct SolverOps : GenericSolverOps<Matrix, MultiVector, DenseMatrix> {
};

template <class Matrix, class MultiVector, class DenseMatrix>
class Solver
{
public:
    typedef SolverOps<Matrix, MultiVector, DenseMatrix> Ops;
    typedef BOperand<Matrix, MultiVector> BType;

    // what a solve is asked to do, the projection method and its parser: rails/TripRule.hpp
    typedef trip::Settings Settings;
    typedef trip::Projection Projection;
    static bool parse_projection(double value, Projection &out) { return trip::parse_projection(value, out); }
    Projection projection() const
    {
        Projection p;
        parse_projection(settings_.projection_method, p);
        return p;
    }

    template <class RightHandSide>
    Solver(Matrix const &A, RightHandSide const &B, Matrix const &M) : op_A_(A), rhs_(BType(B)), op_M_(M) {}

    virtual ~Solver() {}

    template <class ParameterList>
    int set_parameters(ParameterList &params)
    {
        Settings &s = settings_;
        s.trip_limit = lookup_parameter(params, "Maximum iterations", s.trip_limit);
        s.tolerance = lookup_parameter(params, "Tolerance", s.tolerance);
        s.expand_by = lookup_parameter(params, "Expand size", s.expand_by);
        s.lanczos_steps = lookup_parameter(params, "Lanczos iterations", s.lanczos_steps);
        s.shrink_at = lookup_parameter(params, "Restart size", s.shrink_at);
        s.shrink_to = lookup_parameter(params, "Reduced size", s.shrink_to);
        s.shrink_every = lookup_parameter(params, "Restart iterations", s.shrink_every);
        s.keep_above = lookup_parameter(params, "Restart tolerance", s.tolerance * 1e-3); // default follows the tolerance (:84)
        s.shrink_on_convergence = lookup_parameter(params, "Minimize solution space", s.shrink_on_convergence);
        s.warm_start = lookup_parameter(params, "Restart from solution", s.warm_start);
        s.shrink_at_start = lookup_parameter(params, "Restart upon start", s.shrink_at_start);
        const double method = lookup_parameter(params, "Projection method", s.projection_method);
        Projection unused;
        if (!parse_projection(method, unused)) {
            std::cerr << "rails::Solver: 'Projection method' " << method << " is none of 1, 1.1, 1.2, 1.3, 2.1, 2.2, 2.3" << std::endl;
            return 2;
        }
        s.projection_method = method;
        if (s.lanczos_steps <= s.expand_by) { // the estimate must offer more directions than a trip adds (:89-95)
            std::cerr << "rails::Solver: 'Lanczos iterations' (" << s.lanczos_steps << ") has to exceed 'Expand size' (" << s.expand_by << ")" << std::endl;
            return 1;
        }
        return 0;
    }

    // extensions (not in the reference): generalized M, quiet mode, bounded runs, instrumentation
    void use_mass_matrix(bool on) { mass_ = on; }
    // `opts.ortho = 'M'` of matlab/RAILSsolver.m:38-41,538-618: V is kept M-orthonormal (V'MV = I), so the projected equation is the
    // standard one (`lyap(VAV, VBV)`, :384) instead of the generalized one; needs use_mass_matrix(true) and a symmetric definite M
    void use_mass_orthogonalisation(bool on) { ortho_m_ = on; }
    bool mass_orthogonalisation() const { return mass_ && ortho_m_; }
    // opts.Ainv of matlab/RAILSsolver.m:18-22: the operator applied as A^-1 by the projection methods other than 1 (exact or not;
    // any Matrix: a sparse LU solve, a Schur complement's inverse, a callback).  The solver keeps a copy of the handle.
    void set_inverse(Matrix const &Ainv)
    {
        op_Ainv_ = Ainv;
        has_inverse_ = true;
    }
    bool has_inverse() const { return has_inverse_; }
    // opts.nullspace of matlab/RAILSsolver.m:33-34,221-222,311-313,527-529,538-616: a space projected out of every space that joins V
    // (the known kernel of a singular A: a pure Neumann operator, disconnected parts, a pressure mode).  The solver keeps a copy of N (A's
    // rows, any number of columns).  solve() orthonormalises it -- M-orthonormalises it under mass_orthogonalisation(), where the
    // reference's Euclidean basis would not make its M-projection a projector -- and drops dependent columns.
    void set_nullspace(MultiVector const &N)
    {
        nullspace_ = MultiVector(N);
        has_nullspace_ = true;
    }
    void clear_nullspace()
    {
        nullspace_ = MultiVector();
        null_basis_ = MultiVector();
        has_nullspace_ = false;
        null_rank_ = 0;
    }
    bool has_nullspace() const { return has_nullspace_; }
    // columns of the nullspace the last solve kept (0 without one)
    int nullspace_rank() const { return null_rank_; }
    // opts.space of matlab/RAILSsolver.m:25-28,160-204,310-314: with "Restart from solution" the caller's V is ANY start space -- a previous
    // solution's V, [V_prev, B], the union of two earlier solutions -- neither orthonormal nor independent.  The solve orthonormalises it
    // from column 0 with the nullspace projected out and drops every column of which less than 1e-8 survives (orthogonalize_range above;
    // gram_schmidt in M's inner product under mass_orthogonalisation()); it is refused (-2, V and T unchanged) when no column survives.
    void set_raw_start_space(bool on) { raw_start_ = on; }
    bool raw_start_space() const { return raw_start_; }
    // columns the last solve kept of its start space (1 after a cold start)
    int start_rank() const { return start_rank_; }
    void set_verbose(bool on) { verbose_ = on; }
    void set_max_trips(int n) { trip_budget_ = n; }
    // residual Lanczos carried in the (2k+p+1)-dimensional coefficient space where the backend supports it
    void set_projected_lanczos(bool on) { projected_lanczos_ = on; }
    bool projected_lanczos() const { return projected_lanczos_; }
    bool mass_matrix_in_use() const { return mass_; }
    void set_trip_callback(std::function<void(int)> cb) { on_trip_ = cb; }
    // asked once per trip: true ends the run with the code of "stopped without converging" (a back end whose device work has failed)
    void set_failure_check(std::function<bool()> f) { broken_ = f; }
    int trips() const { return trips_; }
    // ||B||_2^2 as the last solve computed it: the scale of its stopping test (src/LyapunovSolver.hpp:134)
    double scale() const { return scale_; }
    std::vector<double> const &residual_history() const { return estimates_; }
    std::map<std::string, double> const &profile() const { return sections_; }
    void reset_profile() { sections_.clear(); }
    BType const &B() const { return rhs_; }
    Settings const &settings() const { return settings_; }
    int lanczos_iterations() const { return settings_.lanczos_steps; }

    // Low-rank solution X = V T V' of A X + X A' + B B' = 0 (A X M' + M X A' + B B' = 0 with a mass matrix)   (src/LyapunovSolver.hpp:100-346)
    // A projection method other than 1 needs set_inverse(), and one that starts from B (x.2) needs B as a multivector: then the
    // solve is refused (-2) and V, T are left as they are.  So is a nullspace (set_nullspace) with a row count other than A's, with no
    // independent column, or with as many as the problem has dimensions; and a raw start space (set_raw_start_space) without one.
    int solve(MultiVector &V, DenseMatrix &T)
    {
        null_rank_ = 0;
        if (has_nullspace_) {
            const int rank = prepare_nullspace(V.M());
            if (rank < 0) return rank;
        }
        const Projection proj = projection();
        if (proj.uses_inverse() && !has_inverse_) {
            std::cerr << "rails::Solver: 'Projection method' " << settings_.projection_method << " needs an inverse (set_inverse)" << std::endl;
            return -2;
        }
        if (proj.start == 2 && rhs_.given_as_operator()) {
            std::cerr << "rails::Solver: 'Projection method' " << settings_.projection_method << " starts from B, which is given as an operator" << std::endl;
            return -2;
        }
        Run run(*this, V, T);
        return run.go();
    }

    // A X + X A' + B = 0 for small dense A, B                                (src/LyapunovSolver.hpp:348-365)
    int dense_solve(DenseMatrix const &Ar, DenseMatrix const &Br, DenseMatrix &Xr)
    {
        // rails_sb03md (SLICOT's interface, src/SlicotWrapper.hpp:14-16) overwrites both arguments: work on copies.  With TRANS = 'T' it
        // returns the solution of A X + X A' = scale * C, so the sign flips; info == n + 1 only warns of a perturbed spectrum (:361).
        DenseMatrix schur_work = Ar.copy();
        Xr = Br.copy();
        const int order = Ar.M(), lda = schur_work.LDA(), ldx = Xr.LDA();
        double scale = 1.0;
        int status = 0;
        rails_sb03md('C', 'X', 'N', 'T', order, schur_work, lda, Xr, ldx, &scale, &status);
        const bool failed = status != 0 && status != order + 1;
        Xr *= -1.0;
        if (failed) std::cerr << "rails::Solver: the projected Lyapunov solve failed (sb03md info " << status << ")" << std::endl;
        return status;
    }

    // A X M' + M X A' + B = 0 for small dense A, B, M: `lyap(VAV, VBV, [], VMV)` of matlab/RAILSsolver.m:382 (SLICOT sg03ad through
    // matlab/mex/lyap.c:125-133), here by congruence with the Cholesky factor M = L L':  (L^-1 A L^-T) Y + Y (..)' + L^-1 B L^-T = 0,
    // X = L^-T Y L^-1.  M symmetric definite; a negative definite one (the reference's MOC data, matlab/DataErik/Bp1.co) is the
    // positive case with the signs of A and M flipped, which leaves the equation unchanged.
    int generalized_dense_solve(DenseMatrix const &A, DenseMatrix const &B, DenseMatrix const &Mm, DenseMatrix &X)
    {
        const int k = A.M();
        DenseMatrix L(k, k), Ahat(k, k), Bhat(k, k);
        int info = 0;
        for (double sign : {1.0, -1.0}) {
            for (int j = 0; j < k; ++j)
                for (int i = 0; i < k; ++i) {
                    L(i, j) = sign * 0.5 * (Mm(i, j) + Mm(j, i));
                    Ahat(i, j) = sign * A(i, j);
                    Bhat(i, j) = B(i, j);
                }
            rails_dpotrf('L', k, L, L.LDA(), &info);
            if (info == 0) break;
        }
        if (info) {
            std::cerr << "rails::Solver: the projected mass matrix is not definite (dpotrf info " << info << ")" << std::endl;
            return info;
        }
        for (DenseMatrix *S : {&Ahat, &Bhat}) { // S <- L^-1 S L^-T
            rails_dtrsm('L', 'L', 'N', 'N', k, k, 1.0, L, L.LDA(), *S, S->LDA());
            rails_dtrsm('R', 'L', 'T', 'N', k, k, 1.0, L, L.LDA(), *S, S->LDA());
        }
        DenseMatrix Y;
        const int ret = dense_solve(Ahat, Bhat, Y);
        rails_dtrsm('L', 'L', 'T', 'N', k, k, 1.0, L, L.LDA(), Y, Y.LDA());
        rails_dtrsm('R', 'L', 'N', 'N', k, k, 1.0, L, L.LDA(), Y, Y.LDA());
        X = Y;
        return ret;
    }

    // Ritz pairs of the residual operator R = AV T V' + V T AV' + B B' (never formed) from max_iter steps of Lanczos started at a
    // random unit vector                                                   (src/LyapunovSolver.hpp:367-447).
    // This member goes through the backend contract only; the HIP backends' solve() takes the fused forms (SolverOps::lanczos) but
    // this one stays available and equivalent.  The order of the additions into the new vector is the reference's (:389-402).
    int resid_lanczos(MultiVector const &image, MultiVector const &basis, DenseMatrix const &reduced, DenseMatrix &tridiagonal,
                      MultiVector &ritz_vectors, DenseMatrix &ritz_values, int steps_wanted)
    {
        MultiVector const &AV = image, &V = basis;
        DenseMatrix const &T = reduced;
        DenseMatrix &H = tridiagonal;
        const int max_iter = steps_wanted;
        MultiVector Q(basis, steps_wanted + 1); // the Lanczos vectors, one column per step (+ the one being built)
        Q.resize(1);
        Q.random();
        Q.view(0) /= Q.norm();
        H = 0.0;

        int steps = 0;
        double off_diagonal = 0.0;
        while (steps < max_iter) {
            const int j = steps++;
            Q.resize(j + 2);
            // column j + 1 <- R q_j, term by term (views are written through; a view passed by value would be a deep copy)
            Q.view(j + 1) = rhs_.times(rhs_.transposed_times(Q.view(j)));
            Q.view(j + 1) += AV * DenseMatrix(T * V.dot(Q.view(j)));
            Q.view(j + 1) += V * DenseMatrix(T * AV.dot(Q.view(j)));
            const double diagonal = Q.view(j + 1).dot(Q.view(j))(0, 0);
            H(j, j) = diagonal;
            Q.view(j + 1) -= diagonal * Q.view(j);
            if (j > 0) Q.view(j + 1) -= off_diagonal * Q.view(j - 1);
            off_diagonal = Q.view(j + 1).norm();
            if (off_diagonal < 1e-14) break; // invariant subspace found: the step counts, the recurrence ends (:419-426)
            H(j + 1, j) = off_diagonal;
            H(j, j + 1) = off_diagonal;
            Q.view(j + 1) /= off_diagonal;
        }
        H.resize(steps, steps);
        Q.resize(steps);
        DenseMatrix ritz(steps, steps);
        H.eigs(ritz, ritz_values);
        ritz_vectors = Q * ritz;
        return 0;
    }

    // The directions a shrink keeps: eigenvectors of T for the `num` eigenvalues of largest modulus, those above `tol` (absolute) only
    // (src/LyapunovSolver.hpp:449-482); num <= 0 asks for all.
    int compute_restart_vectors(DenseMatrix &kept_vectors, DenseMatrix const &reduced, int count, double threshold)
    {
        DenseMatrix &X = kept_vectors;
        DenseMatrix const &T = reduced;
        const int num = count;
        const double tol = threshold;
        const int k = T.N();
        DenseMatrix vectors = T.copy(), values(k, 1);
        int info = 0;
        rails_dsyev('V', 'U', k, vectors, vectors.LDA(), values, &info);
        std::vector<int> columns;
        const int kept = trip::restart_columns(plain_values(values).data(), k, num, tol, columns);
        // a column per candidate, filled where the eigenvalue passes; the count of passes is the width that remains (:468-478)
        X = DenseMatrix(k, (int)columns.size());
        for (int c = 0; c < (int)columns.size(); ++c)
            for (int r = 0; r < k && columns[c] >= 0; ++r) X(r, c) = vectors(r, columns[c]);
        X.resize(k, kept);
        return 0;
    }

private:
    // Modified Gram-Schmidt on X's columns from `first` on, in the M inner product (`in_M`) or the Euclidean one (matlab/RAILSsolver.m:583-597,
    // Morth): every column is scaled to unit length, projected against all columns before it (twice: the reference's single sweep leaves a
    // component of relative size eps * cond, and V'MV = I is what makes the projected equation the standard one), normalised in the inner
    // product, and DROPPED when less than 1e-8 of it is left (:592-594; a column of norm zero, or not finite, is dropped too) -- the later
    // columns move up and X ends with fewer columns than it came with.  With N (orthonormal in the same inner product) every pass
    // projects it out first, with the same M v: `v -= n_i (n_i' M v)` (:600-616).  Returns the columns kept from `first` on.
    int gram_schmidt(MultiVector &X, int first, bool in_M, MultiVector const *N)
    {
        int n = X.N(), j = first;
        while (j < n) {
            MultiVector v = X.view(j);
            const double n0 = v.norm();
            double nrm = 0.0;
            if (n0 > 0.0 && std::isfinite(n0)) {
                v /= n0;
                for (int pass = 0; pass < 2 && (N || j > 0); ++pass) {
                    MultiVector const Mv = in_M ? MultiVector(op_M_ * v) : MultiVector(v);
                    if (N) v -= *N * N->dot(Mv);
                    if (j > 0) {
                        MultiVector const before = X.view(0, j - 1);
                        v -= before * before.dot(Mv);
                    }
                }
                MultiVector const Mv = in_M ? MultiVector(op_M_ * v) : MultiVector(v);
                nrm = std::sqrt(std::abs(v.dot(Mv)(0, 0))); // (a definite M of either sign: the MOC data's mass entries are negative)
            }
            if (!(nrm >= 1e-8)) { // nothing new in this column: the later ones move up
                for (int l = j + 1; l < n; ++l) X.view(l - 1) = X.view(l);
                X.resize(--n);
                continue;
            }
            v /= nrm;
            ++j;
        }
        return n - first;
    }

    // `nullspace = Morth(opts.nullspace, [])` (matlab/RAILSsolver.m:221-222) into null_basis_: gram_schmidt in the inner product of V (M's
    // under mass_orthogonalisation()).  Returns the rank kept, or -2 (with a message) when the solve has to be refused.
    int prepare_nullspace(int n)
    {
        if (nullspace_.M() != n) {
            std::cerr << "rails::Solver: the nullspace has " << nullspace_.M() << " rows, A has " << n << std::endl;
            return -2;
        }
        MultiVector Q(nullspace_);
        const int q = gram_schmidt(Q, 0, mass_orthogonalisation(), nullptr);
        if (q == 0) {
            std::cerr << "rails::Solver: the nullspace has no independent column" << std::endl;
            return -2;
        }
        if (q >= n) {
            std::cerr << "rails::Solver: the nullspace has rank " << q << ", the problem dimension is " << n << ": nothing is left to solve on" << std::endl;
            return -2;
        }
        null_basis_ = Q;
        null_rank_ = q;
        return q;
    }

    // One solve.  Everything the reference keeps in locals of solve() lives here, named for what it is.
    class Run
    {
        Solver &s_;
        Settings const &opt_;
        MultiVector &V_;  // orthonormal basis of the search space (the caller's, in place)
        DenseMatrix &T_;  // reduced solution
        MultiVector fresh_; // the columns of V the operators have not been applied to yet
        MultiVector AV_, MV_, BtV_; // A V, M V (generalized form), B'V
        DenseMatrix a_, b_, m_;     // V'AV, V'B B'V, V'MV
        typename Ops::State backend_state_;
        int n_;         // problem dimension
        int capacity_;  // columns the panels and reduced matrices have room for
        int trip_ = 0;
        int last_shrink_ = 0;
        bool converged_once_ = false;
        double scale_ = 1.0; // ||B||_2^2

    public:
        Run(Solver &s, MultiVector &V, DenseMatrix &T) : s_(s), opt_(s.settings_), V_(V), T_(T), n_(V.M()) {}

        int go()
        {
            if (!open()) return trip::Refused;
            TripTrace trace;
            for (trip_ = 0; trip_ < opt_.trip_limit; ++trip_) {
                trace.lap(trip_, s_.sections_);
                s_.notify();
                const int width_before = V_.N();
                if (fresh_.N()) border();
                reduce();
                typename Ops::Lanczos ritz;
                const double estimate = estimate_residual(ritz);
                const bool converged = std::abs(estimate) < opt_.tolerance * scale_; // :223
                const trip::Verdict end = trip::verdict(opt_, trip_, V_.N(), n_, last_shrink_, converged, converged_once_, s_.trips_, s_.trip_budget_,
                                                        [this]() { return s_.broken_ && s_.broken_(); });
                converged_once_ = end.converged_once;
                switch (end.action) {
                case trip::Finish:
                    finish(converged, estimate);
                    return end.code;
                case trip::Failed:
                case trip::OutOfBudget:
                    s_.notify();
                    return end.code;
                case trip::Shrink:
                    shrink(end.reason);
                    break;
                case trip::Expand:
                    expand(ritz, width_before);
                    break;
                }
            }
            s_.notify();
            return trip::TripsUsedUp;
        }

    private:
        // Room for min(shrink_at or 100, n) columns (:106); a cold start draws one random unit vector (:110-114), a warm start keeps
        // the caller's columns (:116-121) -- orthonormalised with rank detection first when they are a raw start space.  False: the
        // solve is refused (no column of the raw start space survived); V is as it was.
        bool open()
        {
            s_.trips_ = 0;
            s_.estimates_.clear();
            s_.start_rank_ = 0;
            if (opt_.warm_start && s_.raw_start_ && !orthonormalise_start_space()) return false;
            capacity_ = trip::opening_capacity(opt_, V_.N(), n_);
            if (!opt_.warm_start) {
                V_.resize(capacity_);
                V_.resize(1);
                V_.random();
                orthonormalise(0);
            } else {
                if (V_.N() != capacity_) reserve_columns(V_, capacity_);
                if (deflating() && !s_.raw_start_) orthonormalise(0); // the caller's V loses its part along the nullspace like any start space (matlab/RAILSsolver.m:311-313)
            }
            const Projection proj = s_.projection();
            if (proj.uses_inverse() && proj.start != 3) open_with_inverse(proj);
            s_.start_rank_ = V_.N();
            fresh_ = MultiVector(V_); // a deep copy: every column is still to be multiplied (:123)
            AV_ = MultiVector(V_, capacity_);
            AV_.resize(0);
            a_ = DenseMatrix(capacity_, capacity_);
            b_ = DenseMatrix(capacity_, capacity_);
            if (s_.mass_) {
                MV_ = MultiVector(V_, capacity_);
                MV_.resize(0);
                m_ = DenseMatrix(capacity_, capacity_);
            }
            const double nb = s_.rhs_.norm2();
            scale_ = nb * nb;
            s_.scale_ = scale_;
            return true;
        }

        // The caller's V as a raw start space, orthonormalised in place; a copy taken first is what V goes back to when the solve is refused.
        bool orthonormalise_start_space()
        {
            MultiVector const saved(V_);
            int kept = 0;
            if (s_.mass_orthogonalisation())
                kept = orthonormalise(0);
            else
                kept = orthogonalize_range(V_, deflating() ? &s_.null_basis_ : (MultiVector const *)nullptr, 1e-8, has_range_orthogonalize<MultiVector>());
            if (kept < 1) {
                std::cerr << "rails::Solver: no column of the start space is left after orthonormalisation" << std::endl;
                V_ = saved;
                return false;
            }
            return true;
        }

        // The start space of methods x.1 and x.2 (matlab/RAILSsolver.m:288-314): V0 (the columns open() made, x.1) or B (x.2), then
        // V = A^-1 V0 (1.x) or [V0, A^-1 V0] (2.x), orthonormalised like any start space.
        void open_with_inverse(Projection const &proj)
        {
            MultiVector V0 = proj.start == 2 ? MultiVector(s_.rhs_.panel()) : MultiVector(V_);
            MultiVector inv;
            {
                ScopedTimer t(&s_.sections_, "Apply Ainv");
                inv = s_.op_Ainv_ * V0;
            }
            const int width = (proj.pair ? V0.N() : 0) + inv.N();
            capacity_ = std::max(capacity_, width);
            reserve_columns(V_, capacity_);
            V_.resize(0);
            if (proj.pair) V_.push_back(V0);
            V_.push_back(inv);
            orthonormalise(0);
        }

        bool deflating() const { return s_.null_rank_ > 0; }

        // V's columns from `first` on (the ones past the watermark), orthonormalised; with a nullspace, against it as well (:556-579).  Under
        // mass_orthogonalisation() in the M inner product (gram_schmidt), where dependent columns are dropped.  Returns the columns kept.
        int orthonormalise(int first)
        {
            MultiVector const *N = deflating() ? &s_.null_basis_ : nullptr;
            if (s_.mass_orthogonalisation()) return s_.gram_schmidt(V_, first, true, N);
            const int added = V_.N() - first;
            if (N)
                orthogonalize_deflated(V_, *N, first, has_deflated_orthogonalize<MultiVector>());
            else
                V_.orthogonalize();
            return added;
        }

        // capacity change that keeps the columns in use (resize up, then back: the contract's resize preserves data, src/StlWrapper.cpp:225-263)
        static void reserve_columns(MultiVector &X, int columns)
        {
            const int in_use = X.N();
            X.resize(columns);
            X.resize(in_use);
        }
        static void reserve_order(DenseMatrix &S, int order)
        {
            const int in_use = S.M();
            S.resize(order, order);
            S.resize(in_use, in_use);
        }

        // RAILS_DEBUG_DUMP_PROJECTED=file (diagnostics): the projected matrices of every trip appended to it, as text
        static void dump_projected(DenseMatrix const &a, DenseMatrix const &b)
        {
            const char *dump = getenv("RAILS_DEBUG_DUMP_PROJECTED");
            FILE *f = dump ? fopen(dump, "a") : nullptr;
            if (!f) return;
            const int k = a.M();
            fprintf(f, "%d\n", k);
            for (int j = 0; j < k; ++j)
                for (int i = 0; i < k; ++i) fprintf(f, "%.17g %.17g\n", (double)a(i, j), (double)b(i, j));
            fclose(f);
        }

        // block (r0.., c0..) of S <- G
        static void put(DenseMatrix &S, int r0, int c0, DenseMatrix const &G)
        {
            for (int j = 0; j < G.N(); ++j)
                for (int i = 0; i < G.M(); ++i) S(r0 + i, c0 + j) = G(i, j);
        }

        // A, B' (and M) applied to the fresh columns W; with k = columns multiplied before, the reduced matrices grow from k to k + w:
        // new rows W'[AV] and new columns V'[A W] of V'AV (:171-192), the symmetric border of V'BB'V (:174-200), likewise V'MV
        // (matlab/RAILSsolver.m:375-381).
        void border()
        {
            const int k = AV_.N(), w = fresh_.N();
            MultiVector AW, BtW, MW;
            {
                ScopedTimer t(&s_.sections_, "Apply A");
                AW = Ops::apply_append(s_.op_A_, fresh_, AV_);
            }
            {
                ScopedTimer t(&s_.sections_, "Apply B");
                BtW = s_.rhs_.transposed_times(fresh_);
            }
            if (s_.mass_) MW = Ops::apply_append(s_.op_M_, fresh_, MV_);
            if (trip_ == 0) { // B'V has the shape of B', not of V: made from the first B'W (:154-158)
                BtV_ = MultiVector(BtW, capacity_);
                BtV_.resize(0);
            }
            ScopedTimer t(&s_.sections_, "Compute VAV");
            a_.resize(k + w, k + w);
            b_.resize(k + w, k + w);
            if (s_.mass_) m_.resize(k + w, k + w);
            if (k > 0) {
                put(a_, k, 0, fresh_.dot(AV_.view(0, k - 1)));
                const DenseMatrix cross = BtW.dot(BtV_);
                put(b_, k, 0, cross);
                for (int j = 0; j < cross.N(); ++j)
                    for (int i = 0; i < cross.M(); ++i) b_(j, k + i) = cross(i, j);
                if (s_.mass_ && !s_.ortho_m_) put(m_, k, 0, fresh_.dot(MV_.view(0, k - 1)));
            }
            put(a_, 0, k, V_.dot(AW));
            if (s_.mass_ && !s_.ortho_m_) put(m_, 0, k, V_.dot(MW));
            put(b_, k, k, BtW.dot(BtW));
            BtV_.push_back(BtW);
        }

        void reduce()
        {
            ScopedTimer t(&s_.sections_, "dense_solve");
            dump_projected(a_, b_);
            if (s_.mass_ && !s_.ortho_m_)
                s_.generalized_dense_solve(a_, b_, m_, T_);
            else
                s_.dense_solve(a_, b_, T_); // :209; with V'MV = I the generalized equation projects to the standard one (RAILSsolver.m:384)
        }

        // largest modulus among the Ritz values of the residual operator (:211-221)
        double estimate_residual(typename Ops::Lanczos &ritz)
        {
            {
                ScopedTimer t(&s_.sections_, "Residual Lanczos");
                Ops::lanczos(s_, backend_state_, AV_, s_.mass_ ? MV_ : V_, T_, a_, BtV_, opt_.lanczos_steps, ritz);
            }
            const double estimate = ritz.eigenvalues.norm_inf();
            s_.estimates_.push_back(estimate);
            s_.trips_++;
            if (s_.verbose_)
                std::cout << "trip " << trip_ + 1 << ": space " << V_.N() << ", residual estimate " << estimate << " (" << std::abs(estimate) / scale_
                          << " of ||B||^2)" << std::endl;
            return estimate;
        }

        void finish(bool converged, double estimate)
        {
            if (s_.verbose_)
                std::cout << "rails::Solver: " << (converged ? "converged" : "stopped without converging") << " after " << trip_ + 1
                          << " trips, residual estimate " << estimate / scale_ << " of ||B||^2, " << V_.N() << " basis vectors" << std::endl;
            s_.notify();
        }

        // V <- V X with X the dominant eigenvectors of T; everything expressed in V follows (:263-298, matlab/RAILSsolver.m:499-504).
        // The next trip multiplies nothing (no fresh columns, :284) and V is not re-orthogonalised (X has orthonormal columns, :270).
        void shrink(trip::ShrinkReason reason)
        {
            if (s_.verbose_)
                std::cout << "rails::Solver: shrinking the space (" << trip::text(reason) << "), asking for " << (opt_.shrink_to > 0 ? opt_.shrink_to : V_.N())
                          << " of " << V_.N() << " vectors" << std::endl;
            ScopedTimer t(&s_.sections_, "Restart");
            DenseMatrix X;
            s_.compute_restart_vectors(X, T_, std::min(opt_.shrink_to, V_.N()), opt_.keep_above);
            const int kept = X.N();
            auto congruence = [&](DenseMatrix &S) { // S <- X' S X
                DenseMatrix reducedS = X.transpose() * (S * X);
                S.resize(kept, kept);
                S.view() = reducedS;
            };
            Ops::multiply_inplace(V_, X);
            fresh_.resize(0);
            congruence(a_);
            Ops::multiply_inplace(AV_, X);
            Ops::on_restart(backend_state_, X, V_, AV_);
            congruence(b_);
            BtV_.view(0, kept - 1) = BtV_ * X;
            BtV_.resize(kept);
            if (s_.mass_) {
                congruence(m_);
                Ops::multiply_inplace(MV_, X);
            }
            if (s_.verbose_) std::cout << "rails::Solver: " << kept << " vectors kept" << std::endl;
            last_shrink_ = trip_;
        }

        // The Ritz vectors of the `add` largest |Ritz values| join V, as they are, replaced by A^-1 W or paired with it, in the room
        // that trip::plan_expansion works out; only the new columns are orthogonalised (:340) and they are the fresh ones of the next
        // trip (:342).
        void expand(typename Ops::Lanczos const &ritz, int width_before)
        {
            const trip::Expansion plan = trip::plan_expansion(opt_, s_.projection(), V_.N(), n_, ritz.eigenvalues.M(), capacity_);
            const int add = plan.add;
            if (plan.capacity != capacity_) {
                capacity_ = plan.capacity;
                reserve_columns(V_, capacity_);
                reserve_columns(AV_, capacity_);
                reserve_order(a_, capacity_);
                reserve_columns(BtV_, capacity_);
                reserve_order(b_, capacity_);
                if (s_.mass_) {
                    reserve_columns(MV_, capacity_);
                    reserve_order(m_, capacity_);
                }
            }
            std::vector<int> leading;
            find_largest_eigenvalues(ritz.eigenvalues, leading, add);
            {
                ScopedTimer t(&s_.sections_, "Expand");
                ritz.append_to(V_, leading, add);
            }
            if ((plan.pair || plan.replace) && add > 0) {
                MultiVector inv;
                {
                    ScopedTimer t(&s_.sections_, "Apply Ainv");
                    inv = s_.op_Ainv_ * V_.view(width_before, width_before + add - 1);
                }
                if (plan.replace) V_.resize(width_before);
                V_.push_back(inv);
            }
            int kept = 0;
            {
                ScopedTimer t(&s_.sections_, "Orthogonalize");
                kept = orthonormalise(width_before);
            }
            fresh_ = V_.view(width_before, width_before + kept - 1);
        }
    };
    friend class Run;

    void notify()
    {
        if (on_trip_) on_trip_(trips_);
    }

protected:
    Matrix op_A_;
    BType rhs_;
    double scale_ = 0.0;
    Matrix op_M_;
    Matrix op_Ainv_;
    bool has_inverse_ = false;
    MultiVector nullspace_;  // the caller's N (set_nullspace)
    MultiVector null_basis_; // its orthonormal basis for the current solve (prepare_nullspace)
    bool has_nullspace_ = false;
    int null_rank_ = 0;
    Settings settings_;

    bool mass_ = false;
    bool ortho_m_ = false;
    bool raw_start_ = false;
    int start_rank_ = 0;
    bool verbose_ = true;
    int trip_budget_ = 0;
    int trips_ = 0;
    std::vector<double> estimates_;
    std::function<void(int)> on_trip_;
    std::function<bool()> broken_;
    std::map<std::string, double> sections_;
    bool projected_lanczos_ = false;
};

} // namespace rails

#endif
