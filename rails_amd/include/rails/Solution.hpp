// rails::Solution<MultiVector, DenseMatrix> -- the low-rank solution X = U S U' as an object: trace, products, leading eigenpairs and the
// pointwise variance diag(X), written against the same MultiVector / DenseMatrix contract as the solver template (dot, operator*, view,
// orthogonalize; DenseMatrix: (m, n) constructor, operator(), M(), N(), eigs).  It is the second half of the reference's driver
// (src/main.cpp:140-170: the leading eigenpairs of the covariance, its trace, the share of each mode) in factored form: the reference
// iterates with Anasazi on an operator that applies X; with U and S in hand the eigenproblem is a small dense one and exact.
//
// U need not be orthonormal (a lifted Schur solution is not) and may be rank deficient.  The object holds a VIEW of U (no copy of the
// m x k data) and a deep copy of S.
#ifndef RAILS_SOLUTION_HPP
#define RAILS_SOLUTION_HPP

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <type_traits>
#include <utility>
#include <vector>

namespace rails
{

// Whether a MultiVector offers `rowquad(DenseMatrix const &S)`: the m x 1 multivector of sum_{j,l} U(i,j) S(j,l) U(i,l), a back end's own
// one-pass kernel (HipMultiVectorWrapper: rails_panel_rowquad).
template <class MultiVector, class DenseMatrix, class = void>
struct has_rowquad : std::false_type {
};
template <class MultiVector, class DenseMatrix>
struct has_rowquad<MultiVector, DenseMatrix, decltype(std::declval<MultiVector const &>().rowquad(std::declval<DenseMatrix const &>()), void())> : std::true_type {
};

// Whether a MultiVector offers `rowpair(S, ia, ib)` -- the n x 1 multivector of U(ia[i],:) S U(ib[i],:)', the same kernel on gathered rows
// (HipMultiVectorWrapper: rails_panel_rowpair) -- and with it `maps(S, rows, correlation)`, the one-point maps (rails_solution_maps).
template <class MultiVector, class DenseMatrix, class = void>
struct has_rowpair : std::false_type {
};
template <class MultiVector, class DenseMatrix>
struct has_rowpair<MultiVector, DenseMatrix,
                   decltype(std::declval<MultiVector const &>().rowpair(std::declval<DenseMatrix const &>(), std::declval<std::vector<int32_t> const &>(),
                                                                        std::declval<std::vector<int32_t> const &>()),
                            void())> : std::true_type {
};

template <class MultiVector, class DenseMatrix>
class Solution
{
    MultiVector U_;
    DenseMatrix S_;

    MultiVector covariance_(std::vector<int32_t> const &ia, std::vector<int32_t> const &ib, std::true_type) const { return U_.rowpair(S_, ia, ib); }
    // through element access (host back ends; MultiVector(rows, columns) makes the n x 1 result): t = S U(b,:)', then U(a,:) t
    MultiVector covariance_(std::vector<int32_t> const &ia, std::vector<int32_t> const &ib, std::false_type) const
    {
        const int k = U_.N(), n = (int)(ia.empty() ? ib.size() : ia.size());
        MultiVector out(n, 1);
        std::vector<double> t(k);
        for (int i = 0; i < n; ++i) {
            const int a = ia.empty() ? i : ia[i], b = ib.empty() ? i : ib[i];
            for (int j = 0; j < k; ++j) {
                t[j] = 0.0;
                for (int l = 0; l < k; ++l) t[j] += S_(j, l) * U_(b, l);
            }
            double x = 0.0;
            for (int j = 0; j < k; ++j) x += U_(a, j) * t[j];
            out(i, 0) = x;
        }
        return out;
    }

    MultiVector maps_(std::vector<int32_t> const &rows, bool correlation, std::true_type) const { return U_.maps(S_, rows, correlation); }
    // the composition of rails_solution_maps through the contract: G = S U(r,:)' by element access, the maps U G as one product, then the
    // scaling with the variances (one rank: every rows[j] is a row of U)
    MultiVector maps_(std::vector<int32_t> const &rows, bool correlation, std::false_type) const
    {
        const int k = U_.N(), m = U_.M(), q = (int)rows.size();
        DenseMatrix G(k, q);
        for (int j = 0; j < q; ++j)
            for (int l = 0; l < k; ++l) {
                double g = 0.0;
                for (int t = 0; t < k; ++t) g += S_(l, t) * U_(rows[j], t);
                G(l, j) = g;
            }
        MultiVector out = U_ * G;
        if (!correlation) return out;
        MultiVector var = variance();
        for (int j = 0; j < q; ++j) {
            const double vj = var(rows[j], 0);
            for (int i = 0; i < m; ++i) {
                const double vi = var(i, 0);
                if (!(vi > 0.0) || !(vj > 0.0))
                    out(i, j) = 0.0;
                else
                    out(i, j) = (i == rows[j]) ? 1.0 : out(i, j) / (std::sqrt(vi) * std::sqrt(vj));
            }
        }
        return out;
    }

    MultiVector variance_(std::true_type) const { return U_.rowquad(S_); }
    // through the contract: column l of P = U S is one product with a k x 1 matrix; it is multiplied into U's column l entry by entry, which
    // needs the element access of host back ends (operator()(i, j), as the reference's StlWrapper has it)
    MultiVector variance_(std::false_type) const
    {
        const int k = U_.N(), m = U_.M();
        MultiVector out(U_, 1);
        out = 0.0;
        for (int l = 0; l < k; ++l) {
            DenseMatrix s(k, 1);
            for (int j = 0; j < k; ++j) s(j, 0) = S_(j, l);
            MultiVector p = U_ * s;
            for (int i = 0; i < m; ++i) out(i, 0) += p(i, 0) * U_(i, l);
        }
        return out;
    }

public:
    struct Eigs {
        DenseMatrix values;  // found x 1, decreasing modulus
        MultiVector vectors; // m x found, orthonormal
        int found;
    };

    Solution(MultiVector const &U, DenseMatrix const &S) : U_(U.view()), S_(S)
    {
        const int k = S_.M();
        for (int j = 0; j < k; ++j) // S is symmetric by definition of the object
            for (int i = 0; i < j; ++i) S_(i, j) = S_(j, i) = 0.5 * (S_(i, j) + S_(j, i));
    }

    int rank() const { return U_.N(); }
    MultiVector const &U() const { return U_; }
    DenseMatrix const &S() const { return S_; }

    // tr(X) = tr(S U'U): one dot
    double trace() const
    {
        const int k = U_.N();
        DenseMatrix G = U_.dot(U_);
        double t = 0.0;
        for (int j = 0; j < k; ++j)
            for (int i = 0; i < k; ++i) t += S_(i, j) * G(j, i);
        return t;
    }

    // X W = U (S (U'W))
    MultiVector apply(MultiVector const &W) const
    {
        DenseMatrix C = U_.dot(W);
        return U_ * (S_ * C);
    }

    // diag(X) as an m x 1 multivector
    MultiVector variance() const { return variance_(has_rowquad<MultiVector, DenseMatrix>()); }

    // X(ia[i], ib[i]) for every pair as an n x 1 multivector (local row indices; an empty vector is the identity): the covariance of pairs
    // of unknowns -- two variables of one grid cell, a point and its neighbour along a section
    MultiVector covariance(std::vector<int32_t> const &ia, std::vector<int32_t> const &ib) const
    {
        return covariance_(ia, ib, has_rowpair<MultiVector, DenseMatrix>());
    }

    // One-point maps as an m x q multivector: column j is X(:, rows[j]), or with `correlation` X(i, r_j) / sqrt(X(i,i) X(r_j,r_j)) -- 0 where a
    // variance is not > 0, exactly 1 at the reference unknown itself
    MultiVector maps(std::vector<int32_t> const &rows, bool correlation = false) const
    {
        return maps_(rows, correlation, has_rowpair<MultiVector, DenseMatrix>());
    }

    // The `want` eigenpairs of largest modulus (want <= 0: all), those with |lambda| <= tol max|lambda| dropped: Q = orthonormal basis of U,
    // R = Q'U, the small symmetric eigenproblem of R S R', vectors = Q Z.  A dependent column of U leaves a column in Q that U has no part
    // along (a zero row of R), so a rank-deficient U costs nothing but zero eigenvalues.
    Eigs eigs(int want = 0, double tol = 0.0) const
    {
        const int k = U_.N();
        MultiVector Q(U_); // deep copy
        Q.orthogonalize();
        DenseMatrix R = Q.dot(U_);
        DenseMatrix M = (R * S_) * R.transpose();
        for (int j = 0; j < k; ++j)
            for (int i = 0; i < j; ++i) M(i, j) = M(j, i) = 0.5 * (M(i, j) + M(j, i));
        DenseMatrix Zall, d;
        M.eigs(Zall, d);
        std::vector<int> order(k);
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return std::abs(d(a, 0)) > std::abs(d(b, 0)); });
        const int cap = (want <= 0 || want > k) ? k : want;
        const double dmax = k > 0 ? std::abs(d(order[0], 0)) : 0.0;
        int found = 0;
        while (found < cap && std::abs(d(order[found], 0)) > tol * dmax) ++found;
        Eigs out{DenseMatrix(found, 1), MultiVector(), found};
        DenseMatrix Z(k, found);
        for (int q = 0; q < found; ++q) {
            out.values(q, 0) = d(order[q], 0);
            for (int i = 0; i < k; ++i) Z(i, q) = Zall(i, order[q]);
        }
        out.vectors = Q * Z;
        return out;
    }
};

} // namespace rails

#endif
