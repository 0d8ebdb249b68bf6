// Contract test of the classes that plug into Solver<Matrix, MultiVector, DenseMatrix> (the drop-in boundary):
// rails::HipOperatorWrapper, rails::HipMultiVectorWrapper, rails::HostDenseMatrix, and the coordinate-space back end
// rails::SubspaceOperator / rails::SubspaceMultiVector (same multivector cases, instantiated from one template).  The cases
// restate, for these classes, what the reference's typed tests demand of every back end:
//   test/GenericMultiVectorWrapper_test.cpp:63-507, test/GenericOperatorWrapper_test.cpp:74-114,187-229,
//   test/GenericDenseMatrixWrapper_test.cpp:61-209
// (the reference gets element access from a `Testable...` subclass, test/Epetra_TestableWrappers.hpp:14-95; here element
// access goes through host round trips of single columns).  Operator eigs() (GenericOperatorWrapper_test.cpp:116-185) is an
// optional member the solver never calls and is not provided.
//
//   wrapper_contract            all cases (needs a gfx950 GPU)
//   wrapper_contract --host     DenseMatrix cases only (no GPU needed)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <map>
#include <vector>

#include "rails/HipSolverOps.hpp"
#include "rails/SubspaceSolverOps.hpp"

using rails::HipMultiVectorWrapper;
using rails::HipOperatorWrapper;
using rails::HostDenseMatrix;
using rails::SubspaceBasis;
using rails::SubspaceMultiVector;
using rails::SubspaceOperator;

// the two device back ends behind one test body: how to make a 10 x n multivector, a small replicated one, and how exact the
// element-wise comparisons can be (coordinates in a basis reproduce entries to rounding, not bit for bit)
struct HipTraits {
    typedef HipMultiVectorWrapper MV;
    rails_ctx *ctx;
    double tol;
    const char *name;
    MV make(int n) const { return MV(10, n, ctx); }
    MV small(int rows, int n) const { return MV::Replicated(rows, n, ctx); }
};
struct SubspaceTraits {
    typedef SubspaceMultiVector MV;
    std::shared_ptr<SubspaceBasis> basis;
    double tol;
    const char *name;
    MV make(int n) const { return MV(basis, n); }
    MV small(int rows, int n) const { return MV::Plain(basis, rows, n); }
};

static int g_fail = 0, g_checks = 0;
static const char *g_case = "";

#define CHECK(cond)                                                                          \
    do {                                                                                     \
        ++g_checks;                                                                          \
        if (!(cond)) {                                                                       \
            ++g_fail;                                                                        \
            std::printf("FAIL [%s] %s:%d: %s\n", g_case, __FILE__, __LINE__, #cond);          \
        }                                                                                    \
    } while (0)
#define CHECK_NEAR(a, b, tol)                                                                                  \
    do {                                                                                                       \
        ++g_checks;                                                                                            \
        double xa_ = (a), xb_ = (b);                                                                           \
        if (!(std::abs(xa_ - xb_) <= (tol))) {                                                                 \
            ++g_fail;                                                                                          \
            std::printf("FAIL [%s] %s:%d: %s = %.17g vs %s = %.17g\n", g_case, __FILE__, __LINE__, #a, xa_, #b, xb_); \
        }                                                                                                      \
    } while (0)

// ---- element access for the device multivector --------------------------------------------------------------------------
template <class MV>
static std::vector<double> host_of(MV const &v) // column-major M x N
{
    int m = (int)v.local_rows(), n = v.N();
    std::vector<double> h((size_t)m * std::max(n, 0));
    if (n > 0) v.to_host(h.data(), m);
    return h;
}
template <class MV>
static double get(MV const &v, int i, int j)
{
    return host_of(v)[i + (size_t)j * v.local_rows()];
}
template <class MV>
static void set(MV &v, int i, int j, double x)
{
    int m = (int)v.local_rows();
    std::vector<double> col(m);
    MV c = v.view(j);
    c.to_host(col.data(), m);
    col[i] = x;
    int w = v.orthogonalized();
    c.from_host(col.data(), m);
    v.set_orthogonalized(std::min(w, j)); // writing into column j invalidates the watermark from there on
}
template <class MV>
static bool same(MV const &a, MV const &b, double tol = 0.0)
{
    if (a.M() != b.M() || a.N() != b.N()) return false;
    std::vector<double> ha = host_of(a), hb = host_of(b);
    for (size_t i = 0; i < ha.size(); ++i)
        if (!(std::abs(ha[i] - hb[i]) <= tol)) return false;
    return true;
}
template <class MV>
static bool orthonormal(MV const &a, double tol = 1e-14)
{
    HostDenseMatrix G = a.dot(a);
    double worst = 0.0;
    for (int i = 0; i < G.M(); ++i)
        for (int j = 0; j < G.N(); ++j) worst = std::max(worst, std::abs(G(i, j) - (i == j ? 1.0 : 0.0)));
    if (!(worst <= tol)) fprintf(stderr, "  orthonormal: %d columns, max |G - I| = %.3e\n", G.N(), worst);
    return worst <= tol;
}

template <class TR>
struct MVFixture { // four 10 x 10 multivectors, one column in use (GenericMultiVectorWrapper_test.cpp:14-48)
    typename TR::MV a, b, c, d;
    explicit MVFixture(TR const &tr) : a(tr.make(10)), b(tr.make(10)), c(tr.make(10)), d(tr.make(10)) { resize(1); }
    void resize(int n)
    {
        a.resize(n);
        b.resize(n);
        c.resize(n);
        d.resize(n);
    }
};

template <class TR>
static void multivector_cases(TR const &tr)
{
    typedef typename TR::MV MV;
    typedef MVFixture<TR> Fx;
    const double tol = tr.tol; // 0 for the direct back end
    auto run = [&](const char *name, std::function<void(Fx &)> body) {
        static std::string label;
        label = std::string(tr.name) + "." + name;
        g_case = label.c_str();
        if (getenv("RAILS_CONTRACT_VERBOSE")) std::printf("case %s\n", g_case);
        Fx f(tr);
        body(f);
    };
    run("MV.Resize", [&](Fx &f) {
        f.a.resize(0);
        CHECK(f.a.N() == 0);
        f.a.resize(0);
        CHECK(f.a.N() == 0);
        f.a.resize(2);
        CHECK(f.a.N() == 2);
        f.a.resize(1);
        CHECK(f.a.N() == 1);
    });
    run("MV.PutScalar", [&](Fx &f) {
        f.a = 2.0;
        for (int i = 0; i < 10; ++i) CHECK_NEAR(get(f.a, i, 0), 2.0, tol);
    });
    run("MV.Assignment shares storage", [&](Fx &f) {
        f.a.random();
        f.b = f.a;
        f.b = 2.0;
        CHECK(same(f.b, f.a, tol));
        CHECK_NEAR(get(f.a, 3, 0), 2.0, tol);
    });
    run("MV.ScaleAssign", [&](Fx &f) {
        f.a.random();
        f.b = f.a.copy();
        f.b *= 2.5;
        for (int i = 0; i < 10; ++i) CHECK_NEAR(get(f.b, i, 0), get(f.a, i, 0) * 2.5, tol);
    });
    run("MV.AddAssign", [&](Fx &f) {
        f.a.random();
        f.b = f.a.copy();
        f.b += f.a;
        f.a *= 2.0;
        CHECK(same(f.a, f.b, tol));
    });
    run("MV.SubAssign", [&](Fx &f) {
        f.a.random();
        f.b = f.a.copy();
        f.b -= f.a;
        f.a = 0.0;
        CHECK(same(f.a, f.b, tol));
    });
    run("MV.DivAssign", [&](Fx &f) {
        f.a.random();
        f.b = f.a.copy();
        f.b *= 1.0 / 13.0;
        f.a /= 13;
        CHECK(same(f.a, f.b, tol));
    });
    run("MV.Addition", [&](Fx &f) {
        f.a.random();
        f.b = f.a.copy();
        f.b *= 2.0;
        f.d = f.a + f.b;
        for (int i = 0; i < 10; ++i) CHECK_NEAR(get(f.d, i, 0), get(f.a, i, 0) + get(f.b, i, 0), tol);
        CHECK(!same(f.d, f.a)); // a + b is a new object
    });
    run("MV.ScalarTimes", [&](Fx &f) {
        f.a.random();
        f.b = f.a.copy();
        f.b *= 13.0;
        f.c = 13 * f.a;
        CHECK(same(f.b, f.c, tol));
    });
    run("MV.Norm", [&](Fx &f) {
        f.a.random();
        double s = 0.0;
        for (int i = 0; i < 10; ++i) s += get(f.a, i, 0) * get(f.a, i, 0);
        CHECK_NEAR(std::sqrt(s), f.a.norm(), 4e-16 * std::sqrt(s) + tol);
        f.a /= f.a.norm();
        CHECK_NEAR(1.0, f.a.norm(), 4e-16 + tol);
    });
    run("MV.NormView", [&](Fx &f) {
        f.resize(2);
        f.a.random();
        double n1 = 0.0, n2 = 0.0;
        for (int i = 0; i < 10; ++i) {
            n1 += get(f.a, i, 0) * get(f.a, i, 0);
            n2 += get(f.a, i, 1) * get(f.a, i, 1);
        }
        n1 = std::sqrt(n1);
        n2 = std::sqrt(n2);
        CHECK(n1 != 0.0 && n2 != 0.0 && n1 != n2);
        CHECK_NEAR(n1, f.a.view(0).norm(), 4e-16 * n1 + tol);
        CHECK_NEAR(n2, f.a.view(1).norm(), 4e-16 * n2 + tol);
        CHECK(f.a.N() == 2);
        CHECK(f.a.norm() != n1 && f.a.norm() != n2); // 2-norm of the pair, not of a column
    });
    run("MV.Dot", [&](Fx &f) {
        f.a.random();
        f.b.random();
        double s = 0.0;
        for (int i = 0; i < 10; ++i) s += get(f.a, i, 0) * get(f.b, i, 0);
        HostDenseMatrix c = f.a.dot(f.b);
        CHECK(c.M() == 1 && c.N() == 1);
        CHECK_NEAR(s, c(0, 0), 1e-15 + tol);
    });
    run("MV.Dot unequal widths", [&](Fx &f) {
        f.a.resize(2);
        f.a.random();
        f.b.resize(3);
        f.b.random();
        HostDenseMatrix c = f.a.dot(f.b);
        CHECK(c.M() == 2 && c.N() == 3);
        for (int k = 0; k < 3; ++k)
            for (int j = 0; j < 2; ++j) {
                double s = 0.0;
                for (int i = 0; i < 10; ++i) s += get(f.a, i, j) * get(f.b, i, k);
                CHECK_NEAR(s, c(j, k), 1e-15 + tol);
            }
    });
    run("MV.Orthogonalize known answer", [&](Fx &f) {
        f.resize(2);
        f.a = 0.0;
        set(f.a, 0, 0, 2.3);
        set(f.a, 0, 1, 5.3);
        set(f.a, 1, 1, 2.7);
        f.a.orthogonalize();
        f.b = 0.0;
        set(f.b, 0, 0, 1.0);
        set(f.b, 1, 1, 1.0);
        CHECK(same(f.b, f.a, 4e-16 + tol));
    });
    run("MV.Orthogonalize push_back watermark", [&](Fx &f) {
        f.a = 0.0;
        set(f.a, 0, 0, 2.3);
        f.b = 0.0;
        set(f.b, 0, 0, 1.0);
        f.a.orthogonalize();
        CHECK(same(f.b, f.a, 4e-16 + tol));
        f.b.resize(2);
        f.b = 0.0;
        set(f.b, 0, 0, 1.0);
        set(f.b, 1, 1, 1.0);
        f.c = 0.0;
        set(f.c, 0, 0, 5.3);
        set(f.c, 1, 0, 2.7);
        f.a.push_back(f.c);
        f.a.orthogonalize();
        CHECK(same(f.b, f.a, 4e-16 + tol));
    });
    run("MV.Orthogonalize random", [&](Fx &f) {
        f.a.resize(3);
        f.a.random();
        f.a.orthogonalize();
        CHECK(orthonormal(f.a));
        f.b.resize(3);
        f.b.random();
        f.a.push_back(f.b);
        f.a.orthogonalize();
        CHECK(orthonormal(f.a));
        CHECK(f.a.N() == 6);
    });
    run("MV.Orthogonalize after modification", [&](Fx &f) {
        f.a.resize(3);
        f.a.random();
        f.a.orthogonalize();
        CHECK(orthonormal(f.a));
        f.a.random();
        f.a.orthogonalize();
        CHECK(orthonormal(f.a));
        f.a *= 2.0;
        f.a.orthogonalize();
        CHECK(orthonormal(f.a));
        f.a *= 3.3;
        f.a.orthogonalize();
        CHECK(orthonormal(f.a));
        f.a /= 2.6;
        f.a.orthogonalize();
        CHECK(orthonormal(f.a));
        f.a.view(2).random();
        f.a.resize(2);
        f.a.resize(3);
        f.a.orthogonalize();
        CHECK(orthonormal(f.a));
    });
    run("MV.Resize after sharing", [&](Fx &f) {
        f.a.resize(20);
        CHECK(f.a.N() == 20);
        f.a.random();
        f.a.resize(0);
        CHECK(f.a.N() == 0);
        f.b.resize(10);
        f.b.random();
        f.a = f.b;
        CHECK(f.a.N() == 10);
        CHECK(same(f.b, f.a, tol));
        f.a.resize(10);
        CHECK(f.a.N() == 10);
        CHECK(same(f.b, f.a, tol));
    });
    run("MV.Resize keeps data inside the capacity", [&](Fx &f) {
        f.a.resize(1);
        f.a.random();
        f.b = f.a.copy();
        f.a.resize(10);
        f.c = f.a.view(0);
        CHECK(same(f.b, f.c, tol));
    });
    run("MV.View assigns through", [&](Fx &f) {
        f.a.random();
        f.b = f.a.copy();
        f.b.random();
        f.a.view(0) = f.b;
        CHECK(same(f.b, f.a, tol));
    });
    run("MV.View of a shared object", [&](Fx &f) {
        f.a.random();
        f.b = f.a;
        CHECK(same(f.b, f.a, tol));
        f.c.random();
        f.b = f.c;
        CHECK(same(f.b, f.c, tol));
        CHECK(get(f.a, 0, 0) != get(f.b, 0, 0));
        f.b = f.a;
        f.b.view() = f.c;
        CHECK(same(f.a, f.c, tol));
        CHECK(same(f.b, f.c, tol));
    });
    run("MV.Copy is deep", [&](Fx &f) {
        f.a.random();
        f.b = f.a;
        f.b.random();
        CHECK(same(f.b, f.a, tol));
        f.b = f.a.copy();
        CHECK(same(f.b, f.a, tol));
        f.b.random();
        CHECK(get(f.a, 0, 0) != get(f.b, 0, 0));
        MV other = f.a.copy();
        CHECK(same(f.a, other, tol));
        other.random();
        CHECK(get(f.a, 0, 0) != get(other, 0, 0));
    });
    run("MV.PushBack", [&](Fx &f) {
        f.a.resize(3);
        f.a.random();
        f.b = f.a.view(0).copy();
        f.b.push_back(f.a.view(1));
        f.b.push_back(f.a.view(2));
        CHECK(same(f.b, f.a, tol));
        f.a.random();
        f.b = f.a.view(0).copy();
        f.b.push_back(f.a.view(1, 2));
        CHECK(same(f.b, f.a, tol));
    });
    run("MV.Transpose products", [&](Fx &f) {
        // (10 x 10)' * (10 x 1) is the B'W shape of the solver: a small replicated result; (10 x 10) * y is the B*y shape
        // with y a replicated 10 x 1 object (src/MatrixOrMultiVectorWrapper.hpp:54,59)
        f.a.resize(10);
        f.a = 0.0;
        set(f.a, 0, 0, 1);
        set(f.a, 0, 1, 2);
        set(f.a, 1, 0, 3);
        set(f.a, 1, 1, 4);
        f.b.resize(1);
        f.b.random();
        double b0 = get(f.b, 0, 0), b1 = get(f.b, 1, 0);
        MV c = f.a.transpose() * f.b;
        CHECK(c.replicated() && c.M() == 10 && c.N() == 1);
        CHECK_NEAR(b0 + 3.0 * b1, c.host_data()[0], 1e-14 + tol);
        CHECK_NEAR(2.0 * b0 + 4.0 * b1, c.host_data()[1], 1e-14 + tol);
        MV y = tr.small(10, 1);
        std::vector<double> hb = host_of(f.b);
        y.from_host(hb.data(), 10);
        MV d = f.a * y;
        CHECK(!d.replicated() && d.M() == 10 && d.N() == 1);
        CHECK_NEAR(b0 + 2.0 * b1, get(d, 0, 0), 1e-14 + tol);
        CHECK_NEAR(3.0 * b0 + 4.0 * b1, get(d, 1, 0), 1e-14 + tol);
    });
    run("MV.Transpose shapes", [&](Fx &f) {
        f.a.resize(1);
        CHECK(f.a.M() == 10 && f.a.N() == 1);
        CHECK(f.a.transpose().M() == 1 && f.a.transpose().N() == 10);
    });
    run("MV.Construct like another", [&](Fx &f) { // (other, n): same rows, n columns (src/StlWrapper.cpp:46-51; uses :125,156,372)
        f.a.resize(3);
        MV q(f.a, 7);
        CHECK(q.M() == 10 && q.N() == 7 && q.capacity() >= 7);
        MV e;
        e.push_back(f.a.view(1)); // default-constructed target (src/LyapunovSolver.hpp:129)
        CHECK(e.N() == 1 && same(e, MV(f.a.view(1)), tol));
    });
}

// 10 x 10 operator from a dense array (explicit zeros dropped)
static HipOperatorWrapper op_from_dense(rails_ctx *ctx, std::vector<double> const &E, int n)
{
    std::vector<int64_t> rp(n + 1, 0);
    std::vector<int32_t> ci;
    std::vector<double> va;
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < n; ++j)
            if (E[i + (size_t)j * n] != 0.0) {
                ci.push_back(j);
                va.push_back(E[i + (size_t)j * n]);
            }
        rp[i + 1] = (int64_t)ci.size();
    }
    if (ci.empty()) {
        ci.push_back(0);
        va.push_back(0.0);
    }
    return HipOperatorWrapper(ctx, n, n, rp.data(), ci.data(), va.data());
}

// the coordinate-space operator: the same products through materialise / SpMM / absorb
static void subspace_operator_cases(rails_ctx *ctx)
{
    const int n = 10;
    g_case = "Subspace.Op";
    auto basis = std::make_shared<SubspaceBasis>(ctx, n, n, 32);
    std::vector<double> E((size_t)n * n, 0.0);
    E[0 + 0 * n] = 1;
    E[0 + 1 * n] = 2;
    E[1 + 0 * n] = 3;
    E[1 + 1 * n] = 4;
    SubspaceOperator A(op_from_dense(ctx, E, n), basis);
    SubspaceMultiVector a(basis, 1);
    a.random();
    double a0 = get(a, 0, 0), a1 = get(a, 1, 0);
    SubspaceMultiVector b = A * a, bt = A.transpose() * a;
    CHECK_NEAR(a0 + 2.0 * a1, get(b, 0, 0), 1e-13);
    CHECK_NEAR(3.0 * a0 + 4.0 * a1, get(b, 1, 0), 1e-13);
    CHECK_NEAR(0.0, get(b, 5, 0), 1e-13);
    CHECK_NEAR(a0 + 3.0 * a1, get(bt, 0, 0), 1e-13);
    CHECK_NEAR(2.0 * a0 + 4.0 * a1, get(bt, 1, 0), 1e-13);
    CHECK(A.M() == n && A.N() == n);
    // a wider block, then the basis cannot exceed the dimension of the space
    SubspaceMultiVector w(basis, 6);
    w.random();
    SubspaceMultiVector aw = A * w;
    std::vector<double> hw = host_of(w), haw = host_of(aw);
    for (int j = 0; j < 6; ++j) {
        CHECK_NEAR(hw[0 + (size_t)j * n] + 2.0 * hw[1 + (size_t)j * n], haw[0 + (size_t)j * n], 1e-12);
        CHECK_NEAR(3.0 * hw[0 + (size_t)j * n] + 4.0 * hw[1 + (size_t)j * n], haw[1 + (size_t)j * n], 1e-12);
    }
    SubspaceMultiVector more(basis, 8);
    more.random();
    CHECK(basis->dim <= n);
    HostDenseMatrix G = more.dot(more);
    std::vector<double> hm = host_of(more);
    double s01 = 0.0;
    for (int i = 0; i < n; ++i) s01 += hm[i] * hm[i + n];
    CHECK_NEAR(s01, G(0, 1), 1e-12);
}

// the basis machinery itself: degenerate blocks, growth past the initial capacities, compress()
static void subspace_basis_cases(rails_ctx *ctx)
{
    const int m = 300;
    g_case = "Subspace.Basis degenerate block";
    {
        auto basis = std::make_shared<SubspaceBasis>(ctx, m, m, 16); // small on purpose: rows and panel columns must grow
        HipMultiVectorWrapper X(m, 6, ctx);
        X.random();
        std::vector<double> h = host_of(X);
        // columns 0,1 random; 2 = 0 + 1; 3 = copy of 0; 4 random; 5 = 1e-9 * random + column 4 (nearly dependent)
        for (int i = 0; i < m; ++i) {
            h[i + 2 * (size_t)m] = h[i] + h[i + (size_t)m];
            h[i + 3 * (size_t)m] = h[i];
            h[i + 5 * (size_t)m] = h[i + 4 * (size_t)m] + 1e-9 * h[i + 5 * (size_t)m];
        }
        X.from_host(h.data(), m);
        SubspaceMultiVector c = SubspaceMultiVector::Absorb(basis, X);
        CHECK(basis->dim == 4 && basis->n_single == 1); // 3 independent directions + the 1e-9 one; taken column by column
        CHECK(same(c.materialise(), X, 1e-13));
        CHECK(orthonormal(basis->P));
        // the same vectors again: nothing new
        SubspaceMultiVector c2 = SubspaceMultiVector::Absorb(basis, X);
        CHECK(basis->dim == 4);
        CHECK(same(c2.materialise(), X, 1e-13));
    }
    g_case = "Subspace.Basis full space and rounding-level directions";
    {
        // (a) the basis spans the whole space: whatever is absorbed next has only rounding error left after the projections, and
        // none of it may enter the basis (a normalised rounding error is not orthogonal to P)
        const int ms = 40;
        auto basis = std::make_shared<SubspaceBasis>(ctx, ms, ms, 16);
        SubspaceMultiVector a(basis, 20), b(basis, 20);
        a.random();
        b.random();
        CHECK(basis->dim == ms);
        CHECK(orthonormal(basis->P, 1e-12)); // 20 random vectors in the 20 dimensions left: an ill-conditioned block, rounding x 1 / min diag(R)
        for (int rep = 0; rep < 3; ++rep) {
            HipMultiVectorWrapper X(ms, 5, ctx);
            X.random();
            SubspaceMultiVector c = SubspaceMultiVector::Absorb(basis, X);
            CHECK(basis->dim == ms);
            CHECK(orthonormal(basis->P, 1e-12)); // 20 random vectors in the 20 dimensions left: an ill-conditioned block, rounding x 1 / min diag(R)
            CHECK(same(c.materialise(), X, 1e-13));
        }
        // (b) a genuine direction 1e-11 below the part inside span(P) is kept, and kept orthogonal
        auto basis2 = std::make_shared<SubspaceBasis>(ctx, m, m, 16);
        SubspaceMultiVector p(basis2, 10);
        p.random();
        HipMultiVectorWrapper inside = p.materialise().copy(), D(m, 1, ctx);
        D.random();
        std::vector<double> hi = host_of(inside), hd = host_of(D), hx((size_t)m * 2);
        for (int i = 0; i < m; ++i) {
            hx[i] = hi[i + 2 * (size_t)m] - 0.5 * hi[i + 7 * (size_t)m] + 1e-11 * hd[i];
            hx[i + (size_t)m] = hi[i + 4 * (size_t)m]; // and a column wholly inside
        }
        HipMultiVectorWrapper X2(m, 2, ctx);
        X2.from_host(hx.data(), m);
        const long delicate_before = basis2->n_delicate;
        SubspaceMultiVector c = SubspaceMultiVector::Absorb(basis2, X2);
        CHECK(basis2->dim == 11 && basis2->n_delicate == delicate_before + 1);
        CHECK(orthonormal(basis2->P));
        CHECK(same(c.materialise(), X2, 1e-13));
    }
    g_case = "Subspace.Basis second round, synchronous and overlapped";
    {
        // a block whose leading two columns keep 30 % of their squared length outside span(P) (the DGKS rule sends them through a
        // second round) and whose other three are random (one round): once waiting for its orthogonalisation, once in the overlapped
        // form, on the same basis and the same block
        uint64_t seed = 0, stream = 0;
        CHECK(rails_ctx_rng_state(ctx, &seed, &stream) == 0);
        std::vector<double> coef[2];
        for (int run = 0; run < 2; ++run) {
            CHECK(rails_ctx_set_seed(ctx, seed, stream) == 0);
            auto basis = std::make_shared<SubspaceBasis>(ctx, m, m, 16);
            basis->overlap = run == 1;
            SubspaceMultiVector p(basis, 10);
            p.random();
            HipMultiVectorWrapper inside = p.materialise().copy(), X(m, 5, ctx);
            X.random();
            std::vector<double> hi = host_of(inside), hx = host_of(X);
            for (int j = 0; j < 2; ++j) {
                double ni = 0.0, no = 0.0;
                std::vector<double> in(m);
                for (int i = 0; i < m; ++i) {
                    in[i] = j == 0 ? hi[i + 2 * (size_t)m] - 0.5 * hi[i + 7 * (size_t)m] : hi[i + 4 * (size_t)m] + 0.25 * hi[i + (size_t)m];
                    ni += in[i] * in[i];
                    no += hx[i + j * (size_t)m] * hx[i + j * (size_t)m];
                }
                for (int i = 0; i < m; ++i) hx[i + j * (size_t)m] = std::sqrt(0.7 / ni) * in[i] + std::sqrt(0.3 / no) * hx[i + j * (size_t)m];
            }
            X.from_host(hx.data(), m);
            const long second_before = basis->n_second_round, overlapped_before = basis->n_overlapped;
            SubspaceMultiVector c = SubspaceMultiVector::Absorb(basis, X);
            CHECK(basis->n_second_round == second_before + 1 && basis->dim == 15);
            CHECK(basis->n_overlapped == overlapped_before + run);
            HipMultiVectorWrapper image = c.materialise().copy(); // (in the overlapped form this is where the block is read back)
            CHECK(!basis->failed);
            CHECK(orthonormal(basis->P));
            CHECK(same(image, X, 1e-13));
            for (int j = 0; j < 5; ++j)
                for (int i = 0; i < c.coefficient_rows(); ++i) coef[run].push_back(c.coefficients()[i + (size_t)j * c.coefficient_ld()]);
        }
        CHECK(coef[0].size() == 75 && coef[1].size() == 75);
        for (size_t k = 0; k < std::min(coef[0].size(), coef[1].size()); ++k) CHECK_NEAR(coef[0][k], coef[1][k], 1e-11);
    }
    g_case = "Subspace.Basis growth and compress";
    {
        auto basis = std::make_shared<SubspaceBasis>(ctx, m, m, 16);
        SubspaceMultiVector a(basis, 20), b(basis, 30);
        a.random(); // 20 new directions: past the 16 rows / 16 panel columns the basis started with
        b.random();
        CHECK(basis->dim == 50 && basis->row_cap >= 50);
        HipMultiVectorWrapper A0 = a.materialise().copy(), B0 = b.materialise().copy();
        CHECK(orthonormal(basis->P));
        HostDenseMatrix G = a.dot(b);
        std::vector<double> ha = host_of(A0), hb = host_of(B0);
        double s = 0.0;
        for (int i = 0; i < m; ++i) s += ha[i + 3 * (size_t)m] * hb[i + 7 * (size_t)m];
        CHECK_NEAR(s, G(3, 7), 1e-12);
        // drop most of b, compress: the basis shrinks to what is alive, the survivors are unchanged
        b.resize(5);
        b.discard_unused_columns();
        SubspaceMultiVector keep = a.view(0, 9).copy();
        a = SubspaceMultiVector(basis, 1); // the 20-column store dies
        basis->compress();
        CHECK(basis->n_compress == 1 && basis->dim == 15);
        CHECK(orthonormal(basis->P));
        CHECK(same(keep.materialise(), HipMultiVectorWrapper(A0.view(0, 9)), 1e-13));
        CHECK(same(b.materialise(), HipMultiVectorWrapper(B0.view(0, 4)), 1e-13));
        // and the basis keeps working afterwards
        SubspaceMultiVector more(basis, 3);
        more.random();
        CHECK(basis->dim == 18 && orthonormal(basis->P));
    }
}

static void operator_cases(rails_ctx *ctx)
{
    const int n = 10;
    std::vector<double> E((size_t)n * n, 0.0);
    E[0 + 0 * n] = 1;
    E[0 + 1 * n] = 2;
    E[1 + 0 * n] = 3;
    E[1 + 1 * n] = 4;
    HipOperatorWrapper A = op_from_dense(ctx, E, n);
    HipMultiVectorWrapper a(n, 1, ctx);
    g_case = "Op.Apply";
    a.random();
    double a0 = get(a, 0, 0), a1 = get(a, 1, 0);
    HipMultiVectorWrapper b = A * a;
    CHECK_NEAR(a0 + 2.0 * a1, get(b, 0, 0), 1e-14);
    CHECK_NEAR(3.0 * a0 + 4.0 * a1, get(b, 1, 0), 1e-14);
    CHECK_NEAR(0.0, get(b, 5, 0), 0.0);
    g_case = "Op.Transpose";
    HipMultiVectorWrapper bt = A.transpose() * a;
    HipMultiVectorWrapper c = A * a;
    CHECK_NEAR(a0 + 3.0 * a1, get(bt, 0, 0), 1e-14);
    CHECK_NEAR(2.0 * a0 + 4.0 * a1, get(bt, 1, 0), 1e-14);
    CHECK_NEAR(a0 + 2.0 * a1, get(c, 0, 0), 1e-14);
    CHECK_NEAR(3.0 * a0 + 4.0 * a1, get(c, 1, 0), 1e-14);
    CHECK(A.M() == n && A.N() == n && A.transpose().M() == n);
    HipOperatorWrapper copyA(A); // cheap handle copies share the device matrix (src/LyapunovSolverDecl.hpp:37-39)
    CHECK(copyA.csr() == A.csr());
    HipOperatorWrapper empty;
    CHECK(empty.csr() == nullptr);
    g_case = "Op.Norm rank one";
    HipMultiVectorWrapper V(n, n, ctx);
    V.view(0).random();
    std::vector<double> hv = host_of(V.view(0));
    std::fill(E.begin(), E.end(), 0.0);
    for (int i = 0; i < n; ++i) E[i] = hv[i];
    HipOperatorWrapper E1 = op_from_dense(ctx, E, n);
    CHECK(E1.norm() != 0.0);
    CHECK_NEAR(V.view(0).norm(), E1.norm(), 1e-13 * V.view(0).norm());
    g_case = "Op.Norm symmetric";
    V.random();
    std::vector<double> H = host_of(V);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j) H[i + (size_t)j * n] = H[j + (size_t)i * n];
    V.from_host(H.data(), n);
    HipOperatorWrapper E2 = op_from_dense(ctx, H, n);
    HostDenseMatrix DV, D;
    V.dot(V).eigs(DV, D);
    double mx = 0.0;
    for (int i = 0; i < n; ++i) mx = std::max(mx, std::sqrt(std::abs(D(i, 0))));
    CHECK(mx != 0.0);
    CHECK_NEAR(mx, E2.norm(), 1e-7 * mx); // power iteration on A'A: converged to the iteration's own stopping rule, not to the last bit
    g_case = "Op.Callback";
    {
        // an operator given by its action (what wrapping any Epetra_Operator is in the reference, src/Epetra_OperatorWrapper.cpp:75-91):
        // S = E2 - 0.5 I, computed from two library calls inside the callback
        int calls = 0;
        HipOperatorWrapper S = HipOperatorWrapper::FromCallback(ctx, n, [&](bool trans, HipMultiVectorWrapper const &X, HipMultiVectorWrapper &Y) {
            ++calls;
            Y = (trans ? E2.transpose() : E2) * X; // assignment to a view copies in
            Y -= 0.5 * X;
            return true;
        });
        CHECK(S.M() == n && S.csr() != nullptr);
        HipMultiVectorWrapper x(n, 3, ctx);
        x.random();
        HipMultiVectorWrapper y = S * x, ref = E2 * x;
        ref -= 0.5 * x;
        CHECK(calls == 1 && same(y, ref, 1e-14));
        HipMultiVectorWrapper yt = S.transpose() * x, reft = E2.transpose() * x;
        reft -= 0.5 * x;
        CHECK(calls == 2 && same(yt, reft, 1e-14));
        // the same handle under the coordinate-space operator
        auto basis = std::make_shared<SubspaceBasis>(ctx, n, n, 16);
        SubspaceOperator Ss(S, basis);
        SubspaceMultiVector xs = SubspaceMultiVector::Absorb(basis, x);
        SubspaceMultiVector ys = Ss * xs;
        CHECK(calls == 3 && same(ys.materialise(), ref, 1e-13));
        // a failing callback is an error of the product, not a crash
        HipOperatorWrapper bad = HipOperatorWrapper::FromCallback(ctx, n, [](bool, HipMultiVectorWrapper const &, HipMultiVectorWrapper &) { return false; });
        HipMultiVectorWrapper out(n, 3, ctx);
        CHECK(!bad.apply_into(x, out, 0));
    }
}

static void dense_cases()
{
    const double r45 = std::sqrt(45.0);
    {
        g_case = "Dense.Eigs 2x2";
        HostDenseMatrix A(2, 2), B(2, 2), C(2, 1);
        A(0, 0) = 1;
        A(0, 1) = 3;
        A(1, 0) = 3;
        A(1, 1) = 4;
        A.eigs(B, C);
        CHECK_NEAR((5.0 - r45) / 2.0, C(0, 0), 1e-12);
        CHECK_NEAR((5.0 + r45) / 2.0, C(1, 0), 1e-12);
        // eigenvectors: A v = lambda v
        for (int k = 0; k < 2; ++k)
            for (int i = 0; i < 2; ++i) CHECK_NEAR(A(i, 0) * B(0, k) + A(i, 1) * B(1, k), C(k, 0) * B(i, k), 1e-12);
    }
    {
        g_case = "Dense.Eigs after shrinking";
        HostDenseMatrix D(10, 10), B, C(4, 1);
        D = 0.0;
        D(0, 5) = 10.0;
        D(5, 0) = 10.0;
        D.resize(4, 4); // the entries outside the 4 x 4 window must not leak into the eigenproblem
        D(0, 0) = 1;
        D(0, 1) = 3;
        D(1, 0) = 3;
        D(1, 1) = 4;
        D.eigs(B, C);
        std::vector<int> idx;
        rails::find_largest_eigenvalues(C, idx, 4);
        CHECK_NEAR((5.0 + r45) / 2.0, C(idx[0], 0), 1e-12);
        CHECK_NEAR((5.0 - r45) / 2.0, C(idx[1], 0), 1e-12);
    }
    {
        g_case = "Dense.PutScalar/Scale";
        HostDenseMatrix A(2, 2), D(10, 10);
        A = 2.0;
        for (int i = 0; i < 2; ++i)
            for (int j = 0; j < 2; ++j) CHECK(A(i, j) == 2.0);
        A *= 1.5;
        CHECK(A(1, 1) == 3.0);
        D = 0.0;
        D(1, 1) = 1.0;
        D.resize(2, 2);
        D = 0.0;
        CHECK(D(1, 1) == 0.0 && D.M() == 2 && D.N() == 2);
    }
    {
        g_case = "Dense.Resize";
        HostDenseMatrix A(2, 2);
        A = 0.0;
        A(0, 0) = 10.0;
        A.resize(80, 100);
        CHECK(A.M() == 80 && A.LDA() == 80 && A.N() == 100);
        CHECK(A(0, 0) == 10.0);
        HostDenseMatrix E;
        E.resize(10, 10);
        CHECK(E.M() == 10 && E.N() == 10);
        // shrinking and growing inside the capacity keeps contents AND leading dimension (src/LyapunovSolver.hpp:165,323)
        HostDenseMatrix G(6, 6);
        for (int j = 0; j < 6; ++j)
            for (int i = 0; i < 6; ++i) G(i, j) = i + 10.0 * j;
        G.resize(3, 3);
        CHECK(G.LDA() == 6 && G(2, 2) == 22.0);
        G.resize(5, 5);
        CHECK(G.LDA() == 6 && G(4, 3) == 34.0);
        double *raw = G;
        CHECK(raw[4 + 3 * 6] == 34.0); // operator double* + LDA is what sb03md receives (:357)
    }
    {
        g_case = "Dense.View";
        HostDenseMatrix A(2, 2), D(10, 10);
        A = 2.0;
        D = 1.0;
        D.resize(2, 2);
        D.view() = A;
        for (int i = 0; i < 2; ++i)
            for (int j = 0; j < 2; ++j) CHECK(D(i, j) == 2.0);
        D.resize(10, 10);
        for (int i = 0; i < 2; ++i)
            for (int j = 0; j < 2; ++j) CHECK(D(i, j) == 2.0);
        CHECK(D(5, 5) == 1.0);
        HostDenseMatrix S;
        S = A; // assignment to a non-view shares
        S(0, 0) = 7.0;
        CHECK(A(0, 0) == 7.0);
        HostDenseMatrix Cp = A.copy();
        Cp(0, 0) = 8.0;
        CHECK(A(0, 0) == 7.0);
    }
    {
        g_case = "Dense.NormInf";
        HostDenseMatrix A(2, 2);
        A(0, 0) = 1;
        A(0, 1) = 3;
        A(1, 0) = -3;
        A(1, 1) = 4;
        CHECK(A.norm_inf() == 7.0);
    }
    {
        g_case = "Dense.Transpose";
        HostDenseMatrix A(2, 2), a(2, 1);
        A(0, 0) = 1;
        A(0, 1) = 2;
        A(1, 0) = 3;
        A(1, 1) = 4;
        a(0, 0) = 1.2423;
        a(1, 0) = -4.9693;
        HostDenseMatrix b = A.transpose() * a, c = A * a;
        CHECK_NEAR(a(0, 0) + 3.0 * a(1, 0), b(0, 0), 1e-14);
        CHECK_NEAR(2.0 * a(0, 0) + 4.0 * a(1, 0), b(1, 0), 1e-14);
        CHECK_NEAR(a(0, 0) + 2.0 * a(1, 0), c(0, 0), 1e-14);
        CHECK_NEAR(3.0 * a(0, 0) + 4.0 * a(1, 0), c(1, 0), 1e-14);
        CHECK(a.M() == 2 && a.N() == 1 && a.transpose().M() == 1 && a.transpose().N() == 2);
    }
}

// The solver template on the HIP classes against the reference's 2 x 2 known answers, with B given as an operator and as a panel
// (test/LyapunovSolverEpetra_test.cpp:109-177 and :179-239: A = [0 1; -5 -5]; B = -I gives X = [0.62 -0.5; -0.5 0.6], B = [-1; -1]
// gives X = [0.82 -0.5; -0.5 0.6], both to 1e-14 there), and what happens to a failed library call inside the wrappers.
struct KatParameters {
    std::map<std::string, double> p;
    template <typename T>
    T get(std::string const &name, T def)
    {
        auto it = p.find(name);
        return it == p.end() ? def : (T)it->second;
    }
};

template <class SolverT, class MV>
static void check_kat(SolverT &solver, MV &V, double x00, double x01, double x11)
{
    KatParameters params;
    params.p = {{"Minimize solution space", 0.0}, {"Lanczos iterations", 10.0}, {"Expand size", 3.0}};
    CHECK(solver.set_parameters(params) == 0);
    solver.set_verbose(false);
    HostDenseMatrix T;
    const int code = solver.solve(V, T);
    CHECK(code == 0);
    std::vector<double> h = host_of(V);
    const int n = 2, k = V.N();
    double X[2][2] = {{0, 0}, {0, 0}};
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j)
            for (int a = 0; a < k; ++a)
                for (int b = 0; b < k; ++b) X[i][j] += h[i + (size_t)a * n] * T(a, b) * h[j + (size_t)b * n];
    CHECK_NEAR(x00, X[0][0], 1e-12);
    CHECK_NEAR(x01, X[0][1], 1e-12);
    CHECK_NEAR(x01, X[1][0], 1e-12);
    CHECK_NEAR(x11, X[1][1], 1e-12);
}

static void solver_cases(rails_ctx *ctx)
{
    const int n = 2;
    std::vector<double> Ad = {0.0, -5.0, 1.0, -5.0}; // column-major [0 1; -5 -5]
    std::vector<double> minus_identity = {-1.0, 0.0, 0.0, -1.0};
    HipOperatorWrapper A = op_from_dense(ctx, Ad, n);
    {
        g_case = "Solver.B as an operator (direct panels)";
        rails::clear_sticky_error();
        HipOperatorWrapper Bop = op_from_dense(ctx, minus_identity, n);
        rails::HipSolver solver(A, Bop, A);
        CHECK(solver.B().given_as_operator());
        HipMultiVectorWrapper V(n, 1, ctx);
        check_kat(solver, V, 0.62, -0.5, 0.6);
        CHECK(rails::sticky_error() == RAILS_OK);
    }
    {
        g_case = "Solver.B as a panel (direct panels)";
        HipMultiVectorWrapper B(n, 1, ctx);
        B = -1.0;
        rails::HipSolver solver(A, B, A);
        CHECK(!solver.B().given_as_operator());
        HipMultiVectorWrapper V(n, 1, ctx);
        check_kat(solver, V, 0.82, -0.5, 0.6);
    }
    {
        g_case = "Solver.B as a panel (coordinates in a basis)";
        auto basis = std::make_shared<SubspaceBasis>(ctx, n, n, 16);
        HipMultiVectorWrapper B(n, 1, ctx);
        B = -1.0;
        SubspaceMultiVector Bc = SubspaceMultiVector::Absorb(basis, B);
        SubspaceOperator Ac(A, basis);
        rails::SubspaceSolver solver(Ac, Bc, Ac);
        SubspaceMultiVector V(basis, 1);
        check_kat(solver, V, 0.82, -0.5, 0.6);
    }
    {
        // a library call that fails inside a wrapper prints (like the reference) AND latches its code: a caller of solve() can tell
        g_case = "Wrappers.failed call is latched";
        rails::clear_sticky_error();
        HipMultiVectorWrapper huge(4000000, 1, ctx);
        std::fprintf(stderr, "(the next message is expected: a 128 TB panel is requested on purpose)\n");
        huge.resize(1 << 22);
        CHECK(rails::sticky_error() == RAILS_ENOMEM);
        CHECK(huge.N() <= huge.capacity()); // the column count stays inside what exists
        rails::clear_sticky_error();
        CHECK(rails::sticky_error() == RAILS_OK);
    }
}

int main(int argc, char **argv)
{
    bool host_only = argc > 1 && std::strcmp(argv[1], "--host") == 0;
    setvbuf(stdout, nullptr, _IONBF, 0);
    if (rails_host_lapack_init(nullptr) != RAILS_OK) {
        std::printf("no host LAPACK: %s\n", rails_last_error());
        return 2;
    }
    dense_cases();
    if (!host_only) {
        rails_ctx *ctx = nullptr;
        if (rails_ctx_create(0, nullptr, &ctx) != RAILS_OK) {
            std::printf("rails_ctx_create failed: %s\n", rails_last_error());
            return 2;
        }
        rails_ctx_set_seed(ctx, 11, 0);
        rails::set_default_context(ctx);
        HipTraits ht{ctx, 0.0, "MV"};
        multivector_cases(ht);
        operator_cases(ctx);
        { // the basis panel must be gone before the context
            SubspaceTraits st{std::make_shared<SubspaceBasis>(ctx, 10, 10, 32), 2e-14, "SubspaceMV"};
            multivector_cases(st);
        }
        subspace_operator_cases(ctx);
        subspace_basis_cases(ctx);
        solver_cases(ctx);
        rails_ctx_destroy(ctx);
    }
    std::printf("%s: %d checks, %d failures\n", host_only ? "host cases" : "all cases", g_checks, g_fail);
    if (g_fail == 0) std::printf("ALL PASSED\n");
    return g_fail == 0 ? 0 : 1;
}
