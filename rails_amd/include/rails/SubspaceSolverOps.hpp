// SolverOps specialisation for the coordinate-space back end (rails/SubspaceWrappers.hpp): the solver's member-by-member
// sequences are already cheap there (host coefficient operations); the only customisation is what happens at a restart.
#ifndef RAILS_SUBSPACESOLVEROPS_HPP
#define RAILS_SUBSPACESOLVEROPS_HPP

#include "rails/LyapunovSolver.hpp"
#include "rails/SubspaceWrappers.hpp"

namespace rails
{

// the restart products are coefficient GEMMs; afterwards the basis is re-based on what is still alive
template <>
struct SolverOps<SubspaceOperator, SubspaceMultiVector, HostDenseMatrix> : GenericSolverOps<SubspaceOperator, SubspaceMultiVector, HostDenseMatrix> {
    static void multiply_inplace(SubspaceMultiVector &V, HostDenseMatrix const &X)
    {
        V.view(0, X.N() - 1) = V * X;
        V.resize(X.N());
        V.discard_unused_columns();
    }
    static void on_restart(State &, HostDenseMatrix const &, SubspaceMultiVector &V, SubspaceMultiVector &)
    {
        if (V.basis()) V.basis()->compress();
    }
};

typedef Solver<SubspaceOperator, SubspaceMultiVector, HostDenseMatrix> SubspaceSolver;

} // namespace rails

#endif
