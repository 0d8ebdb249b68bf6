// solver_capi.cpp -- C ABI (include/rails_solver.h) over rails::Solver instantiated on the HIP backend.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include <exception>
#include <new>

#include "rails/HipSolverOps.hpp"
#include "rails/SubspaceSolverOps.hpp"
#include "rails_solution.h"
#include "rails_solver.h"
#include "solve_choice.h"

void rails_set_error(const char *fmt, ...);

namespace
{

// the duck-typed ParameterList of the reference's tests (test/LyapunovSolver_test.cpp:160-179)
class ParameterList
{
    std::map<std::string, double> params_;

public:
    template <typename T>
    T get(std::string const &name, T def)
    {
        auto it = params_.find(name);
        if (it == params_.end()) return def;
        return (T)it->second;
    }
    void set(std::string const &name, double val) { params_[name] = val; }
};

// What a solve leaves behind for the accessors, whichever back end ran it.
struct Outcome {
    int code = 0, trips = 0;
    std::vector<double> history;
    std::map<std::string, double> profile;
    double scale = 0.0; // ||B||_2^2
    int null_rank = 0, start_rank = 0;
    std::string stats = "{}"; // counters of the coordinate-space back end
    rails::SolveBackend backend = rails::DirectBackend;
};

template <class SolverT>
Outcome outcome_of(SolverT const &solver, int code, rails::SolveBackend backend, std::string const &stats = "{}")
{
    return {code, solver.trips(), solver.residual_history(), solver.profile(), solver.scale(), solver.nullspace_rank(), solver.start_rank(), stats, backend};
}

} // namespace

struct rails_solver {
    rails_ctx *ctx = nullptr;
    rails::HipOperatorWrapper A, M;
    rails::HipMultiVectorWrapper B;
    rails::HipOperatorWrapper Bop; // rails_solver_create_sparse: B as an operator over the caller's rails_sprhs
    rails_sprhs *sprhs = nullptr;
    rails::HipSolver *solver = nullptr;
    ParameterList params;
    rails::HipMultiVectorWrapper V;
    rails::HostDenseMatrix T;
    int64_t m_local = 0, m_global = 0;
    bool has_M = false;
    rails::HipOperatorWrapper Ainv; // rails_solver_set_inverse (the caller owns the handle)
    bool has_inv = false;
    rails::HipMultiVectorWrapper N; // rails_solver_set_nullspace (null_q columns; 0: none)
    int null_q = 0;
    bool mass = false;
    bool ortho_m = false; // V kept M-orthonormal (matlab/RAILSsolver.m opts.ortho = 'M'); needs mass
    rails_trip_fn trip_fn = nullptr;
    void *trip_user = nullptr;
    // the option "subspace": the coordinate-space back end (rails/SubspaceWrappers.hpp) where solve_choice.h lets it run
    bool subspace = true, verbose = true, projected = false;
    int max_trips = 0;
    bool have_V0 = false;
    rails::HipMultiVectorWrapper start; // rails_solver_set_start_space: the raw start space of the next solve (a device copy)
    bool have_start = false;
    Outcome last; // of the last solve that ran, on either back end

    // the options and the trip callback, applied to a solver of either back end
    template <class SolverT>
    void configure(SolverT &to)
    {
        to.use_mass_matrix(mass);
        to.use_mass_orthogonalisation(ortho_m);
        to.set_verbose(verbose);
        to.set_max_trips(max_trips);
        to.set_projected_lanczos(projected);
        to.set_trip_callback(trip_fn ? std::function<void(int)>([this](int trip) { trip_fn(trip_user, trip); }) : std::function<void(int)>());
    }
};

extern "C" int rails_solver_create(rails_ctx *ctx, rails_csr *A, rails_csr *M, const double *B_host, int64_t ldb, int p, int64_t m_global,
                                   rails_solver **out)
try {
    if (!ctx || !A || !out || (p > 0 && !B_host) || p < 0) {
        rails_set_error("rails_solver_create: bad argument");
        return RAILS_EINVAL;
    }
    int64_t m = rails_csr_rows(A);
    if (ldb < m) {
        rails_set_error("rails_solver_create: ldb %lld < local rows %lld", (long long)ldb, (long long)m);
        return RAILS_EINVAL;
    }
    if (M && rails_csr_rows(M) != m) {
        rails_set_error("rails_solver_create: M has %lld rows, A %lld", (long long)rails_csr_rows(M), (long long)m);
        return RAILS_EINVAL;
    }
    rails_solver *s = new rails_solver();
    s->ctx = ctx;
    s->m_local = m;
    s->m_global = m_global > 0 ? m_global : m;
    s->A = rails::HipOperatorWrapper(ctx, A, s->m_global);
    s->has_M = (M != nullptr);
    s->M = M ? rails::HipOperatorWrapper(ctx, M, s->m_global) : s->A;
    s->B = rails::HipMultiVectorWrapper(m, p, ctx);
    s->B.set_global_rows(s->m_global);
    s->B.from_host(B_host, ldb);
    s->solver = new rails::HipSolver(s->A, s->B, s->M);
    s->V = rails::HipMultiVectorWrapper(m, 1, ctx);
    s->V.set_global_rows(s->m_global);
    *out = s;
    return RAILS_OK;
} catch (std::bad_alloc const &) {
    rails_set_error("rails_solver_create: out of host memory");
    return RAILS_ENOMEM;
} catch (std::exception const &e) {
    rails_set_error("rails_solver_create: %s", e.what());
    return RAILS_EINVAL;
}

extern "C" int rails_solver_create_sparse(rails_ctx *ctx, rails_csr *A, rails_csr *M, rails_sprhs *S, int64_t m_global, rails_solver **out)
try {
    if (!ctx || !A || !S || !out) {
        rails_set_error("rails_solver_create_sparse: null argument");
        return RAILS_EINVAL;
    }
    const int64_t m = rails_csr_rows(A);
    if (rails_sprhs_rows(S) != m || (M && rails_csr_rows(M) != m)) {
        rails_set_error("rails_solver_create_sparse: A has %lld rows, B %lld, M %lld", (long long)m, (long long)rails_sprhs_rows(S),
                        (long long)(M ? rails_csr_rows(M) : m));
        return RAILS_EINVAL;
    }
    if (m_global > 0 && m_global != m) {
        rails_set_error("rails_solver_create_sparse: single GPU only (%lld global rows, %lld local)", (long long)m_global, (long long)m);
        return RAILS_EINVAL;
    }
    rails_solver *s = new rails_solver();
    s->ctx = ctx;
    s->m_local = s->m_global = m;
    s->A = rails::HipOperatorWrapper(ctx, A, m);
    s->has_M = (M != nullptr);
    s->M = M ? rails::HipOperatorWrapper(ctx, M, m) : s->A;
    s->sprhs = S;
    s->Bop = rails::HipOperatorWrapper(ctx, S);
    if (!s->Bop.csr()) {
        delete s;
        return RAILS_EINVAL; // rails_csr_create_sprhs has set the message
    }
    s->solver = new rails::HipSolver(s->A, s->Bop, s->M);
    s->V = rails::HipMultiVectorWrapper(m, 1, ctx);
    *out = s;
    return RAILS_OK;
} catch (std::bad_alloc const &) {
    rails_set_error("rails_solver_create_sparse: out of host memory");
    return RAILS_ENOMEM;
} catch (std::exception const &e) {
    rails_set_error("rails_solver_create_sparse: %s", e.what());
    return RAILS_EINVAL;
}

extern "C" int rails_solver_destroy(rails_solver *s)
{
    if (!s) return RAILS_OK;
    delete s->solver;
    delete s;
    return RAILS_OK;
}

extern "C" int rails_solver_set_parameter(rails_solver *s, const char *name, double value)
{
    if (!s || !name) return RAILS_EINVAL;
    s->params.set(name, value);
    return RAILS_OK;
}

extern "C" int rails_solver_apply_parameters(rails_solver *s, int *code)
{
    if (!s) return RAILS_EINVAL;
    int rc = s->solver->set_parameters(s->params);
    if (code) *code = rc;
    return RAILS_OK;
}

extern "C" int rails_solver_set_option(rails_solver *s, const char *name, double value)
{
    if (!s || !name) return RAILS_EINVAL;
    std::string n(name);
    if (n == "mass") {
        if (value != 0.0 && !s->has_M) {
            rails_set_error("rails_solver_set_option: mass requested but the solver was created without M");
            return RAILS_EINVAL;
        }
        s->mass = value != 0.0;
    } else if (n == "mass_orthogonalisation" || n == "ortho_m") {
        if (value != 0.0 && !s->mass) {
            rails_set_error("rails_solver_set_option: mass_orthogonalisation needs the option mass (set it first)");
            return RAILS_EINVAL;
        }
        s->ortho_m = value != 0.0;
    } else if (n == "verbose")
        s->verbose = value != 0.0;
    else if (n == "max_trips")
        s->max_trips = (int)value;
    else if (n == "projected_lanczos")
        s->projected = value != 0;
    else if (n == "subspace")
        s->subspace = value != 0;
    else {
        rails_set_error("rails_solver_set_option: unknown option '%s'", name);
        return RAILS_EINVAL;
    }
    s->configure(*s->solver);
    return RAILS_OK;
}

extern "C" int rails_solver_set_inverse(rails_solver *s, rails_csr *Ainv)
{
    if (!s || !Ainv) {
        rails_set_error("rails_solver_set_inverse: null argument");
        return RAILS_EINVAL;
    }
    if (rails_csr_rows(Ainv) != s->m_local) {
        rails_set_error("rails_solver_set_inverse: the inverse has %lld rows, A %lld", (long long)rails_csr_rows(Ainv), (long long)s->m_local);
        return RAILS_EINVAL;
    }
    s->Ainv = rails::HipOperatorWrapper(s->ctx, Ainv, s->m_global);
    s->has_inv = true;
    s->solver->set_inverse(s->Ainv);
    return RAILS_OK;
}

extern "C" int rails_solver_set_nullspace(rails_solver *s, const double *N_host, int64_t ldn, int q)
{
    if (!s || q < 0 || (q > 0 && (!N_host || ldn < s->m_local))) {
        rails_set_error("rails_solver_set_nullspace: bad argument");
        return RAILS_EINVAL;
    }
    s->null_q = q;
    s->last.null_rank = 0;
    if (q == 0) {
        s->N = rails::HipMultiVectorWrapper();
        s->solver->clear_nullspace();
        return RAILS_OK;
    }
    s->N = rails::HipMultiVectorWrapper(s->m_local, q, s->ctx);
    s->N.set_global_rows(s->m_global);
    s->N.from_host(N_host, ldn);
    s->solver->set_nullspace(s->N);
    return RAILS_OK;
}

extern "C" int rails_solver_nullspace_rank(rails_solver *s) { return s ? s->last.null_rank : -1; }

extern "C" int rails_solver_set_trip_callback(rails_solver *s, rails_trip_fn fn, void *user)
{
    if (!s) return RAILS_EINVAL;
    s->trip_fn = fn;
    s->trip_user = user;
    s->configure(*s->solver);
    return RAILS_OK;
}

extern "C" int rails_solver_set_V(rails_solver *s, const double *V_host, int64_t ldv, int k)
{
    if (!s || !V_host || k < 1 || ldv < s->m_local) {
        rails_set_error("rails_solver_set_V: bad argument");
        return RAILS_EINVAL;
    }
    s->V = rails::HipMultiVectorWrapper(s->m_local, k, s->ctx);
    s->V.set_global_rows(s->m_global);
    s->V.from_host(V_host, ldv);
    s->V.set_orthogonalized(k); // the caller's V is assumed orthonormal
    s->have_V0 = true;
    s->have_start = false;
    s->start = rails::HipMultiVectorWrapper();
    return RAILS_OK;
}

extern "C" int rails_solver_set_start_space(rails_solver *s, const rails_panel *P, int c0, int k)
{
    if (!s || !P) {
        rails_set_error("rails_solver_set_start_space: null argument");
        return RAILS_EINVAL;
    }
    if (k < 1 || c0 < 0 || c0 + k > rails_panel_capacity(P)) {
        rails_set_error("rails_solver_set_start_space: columns [%d,%d) of a panel of capacity %d", c0, c0 + k, rails_panel_capacity(P));
        return RAILS_EINVAL;
    }
    if (rails_panel_rows(P) != s->m_local) {
        rails_set_error("rails_solver_set_start_space: the panel has %lld rows, the solver %lld local rows", (long long)rails_panel_rows(P),
                        (long long)s->m_local);
        return RAILS_EINVAL;
    }
    rails::HipMultiVectorWrapper W(s->m_local, k, s->ctx);
    W.set_global_rows(s->m_global);
    const int rc = rails_panel_copy(s->ctx, P, c0, k, W.panel(), 0); // device to device
    if (rc != RAILS_OK) return rc;
    s->start = W;
    s->have_start = true;
    s->have_V0 = false;
    return RAILS_OK;
}

extern "C" int rails_solver_start_rank(rails_solver *s) { return s ? s->last.start_rank : -1; }

// the same solve on the coordinate-space back end: B and every later vector are expressed in one orthonormal device basis
static int solve_in_coordinates(rails_solver *s)
{
    rails::HipSolver::Projection proj;
    const bool pair = rails::HipSolver::parse_projection(s->params.get("Projection method", 1.0), proj) && proj.pair; // 2.x: twice per trip
    const int restart = s->params.get("Restart size", -1);
    const int rows = rails::trip::coordinate_basis_rows(restart, s->params.get("Expand size", 3), pair, s->have_start ? s->start.N() : 0, s->B.N());
    auto basis = std::make_shared<rails::SubspaceBasis>(s->ctx, s->m_local, s->m_global, rows);
    if (restart > 0 || s->params.get("Restart iterations", 20) > 0) basis->preallocate_compress_panel(); // restarts will re-base the basis
    rails::SubspaceMultiVector Bc = rails::SubspaceMultiVector::Absorb(basis, s->B);
    rails::SubspaceOperator Ac(s->A, basis);
    rails::SubspaceOperator Mc(s->mass ? s->M : s->A, basis);
    rails::SubspaceSolver solver(Ac, Bc, Mc);
    if (s->has_inv) solver.set_inverse(rails::SubspaceOperator(s->Ainv, basis));
    if (s->null_q > 0) solver.set_nullspace(rails::SubspaceMultiVector::Absorb(basis, s->N)); // the one absorb of N: a live store from then on
    ParameterList params = s->params;
    if (s->have_start) params.set("Restart from solution", 1.0); // a start space makes a warm start whatever the parameter says
    int prc = solver.set_parameters(params);
    if (prc != 0) return prc + 100;
    s->configure(solver);
    solver.set_failure_check([basis]() { return basis->failed; }); // a latched failure of the basis ends the run at the next trip
    rails::SubspaceMultiVector Vc(basis, 1);
    if (s->have_V0) { // warm start: the caller's (orthonormal) V expressed in the basis (src/LyapunovSolver.hpp:116-123)
        Vc = rails::SubspaceMultiVector::Absorb(basis, s->V);
        Vc.set_orthogonalized(Vc.N());
    }
    if (s->have_start) { // opts.space: orthonormalised on the device with dependent columns dropped, then absorbed like the warm start's V
        if (s->start.orthogonalize_range(nullptr, 0.0) < 1) {
            if (rails::sticky_error() == RAILS_OK) std::cerr << "rails::Solver: no column of the start space is left after orthonormalisation" << std::endl;
            return -2;
        }
        // A start space that is a converged solution holds B to within the tolerance: projected against B's basis columns the block keeps
        // every column's length but loses rank, which is not what the overlapped orthogonalisation predicts from -- absorbed the
        // waiting way, where every block is decided before the next step
        const bool overlap = basis->overlap;
        basis->overlap = false;
        Vc = rails::SubspaceMultiVector::Absorb(basis, s->start);
        basis->overlap = overlap;
        Vc.set_orthogonalized(Vc.N());
    }
    int rc = solver.solve(Vc, s->T);
    if (rc != -2) { // (refused before the first trip: V and T stay as they were)
        s->V = Vc.materialise();
        s->V.set_orthogonalized(s->V.N());
    }
    rails::SubspaceBasis const &b = *basis;
    char buf[1536];
    snprintf(buf, sizeof(buf), "{\"dim\": %d, \"absorb\": %ld, \"absorb_columns\": %ld, \"one_by_one\": %ld, \"dropped\": %ld, \"compress\": %ld, \"materialise\": %ld, \"prefetched_random\": %ld, \"second_rounds\": %ld, \"delicate_blocks\": %ld, \"reprojected_blocks\": %ld, \"overlapped_blocks\": %ld, \"scratch_blocks\": %ld, \"replaced_columns\": %ld, \"verified\": %d, \"verify_representation\": %.3e, \"verify_orthonormality\": %.3e, \"seconds\": {\"materialise\": %.4f, \"absorb\": %.4f, \"compress_qr\": %.4f, \"compress_rotate\": %.4f, "
             "\"compress_coefficients\": %.4f}}",
             b.dim, b.n_absorb, b.n_absorb_cols, b.n_single, b.n_dropped, b.n_compress, b.n_materialise, b.n_prefetched, b.n_second_round, b.n_delicate, b.n_reprojected, b.n_overlapped, b.n_scratch_blocks, b.n_replaced, b.verify ? 1 : 0, b.verify_repr, b.verify_orth,
             b.t_materialise, b.t_absorb, b.t_qr, b.t_rotate, b.t_recoef);
    s->last = outcome_of(solver, rc, rails::CoordinateBackend, buf);
    if (rc != -2 && basis->failed) {
        rails_set_error("coordinate-space back end: a device operation failed (%s)", rails_last_error());
        return -1000;
    }
    return rc;
}

extern "C" int rails_solver_solve(rails_solver *s, int *code, int *k)
{
    if (!s) return RAILS_EINVAL;
    const bool restart_from_solution = s->params.get("Restart from solution", 0.0) != 0.0;
    const rails::SolveBackend backend = rails::choose_backend(s->subspace, s->sprhs != nullptr, s->have_V0, s->have_start, s->null_q, restart_from_solution);
    { // the projection method: a valid value (rails_solver_apply_parameters reports it) with the inverse it needs
        rails::HipSolver::Projection proj;
        const double method = s->params.get("Projection method", 1.0);
        if (!rails::HipSolver::parse_projection(method, proj)) {
            rails_set_error("rails_solver_solve: 'Projection method' %g is none of 1, 1.1, 1.2, 1.3, 2.1, 2.2, 2.3", method);
            return RAILS_EINVAL;
        }
        if (proj.uses_inverse() && !s->has_inv) {
            rails_set_error("rails_solver_solve: 'Projection method' %g needs an inverse (rails_solver_set_inverse)", method);
            return RAILS_EINVAL;
        }
    }
    rails::clear_sticky_error();
    int rc;
    try { // the solver templates allocate (std::vector, make_shared): nothing may unwind through the C boundary
        if (backend == rails::CoordinateBackend) {
            rc = solve_in_coordinates(s);
            if (rc == -1000) return RAILS_EHIP;
        } else if (s->have_start) { // on the start space's own copy: a refused solve leaves V and T as they were
            const bool was_warm = s->solver->settings().warm_start;
            struct Restore { // also when the parameters are refused or the solve throws
                rails_solver *s;
                bool warm; // (a parameter that is not in the list keeps its current value: put the former one back by name)
                ~Restore()
                {
                    ParameterList back = s->params;
                    back.set("Restart from solution", warm ? 1.0 : 0.0);
                    s->solver->set_raw_start_space(false);
                    s->solver->set_parameters(back);
                }
            } restore{s, was_warm};
            ParameterList params = s->params;
            params.set("Restart from solution", 1.0);
            const int prc = s->solver->set_parameters(params);
            if (prc != 0) {
                rails_set_error("rails_solver_solve: the parameters are not valid (code %d, rails_solver_apply_parameters)", prc);
                return RAILS_EINVAL;
            }
            s->solver->set_raw_start_space(true);
            rails::HipMultiVectorWrapper Vs = s->start;
            rc = s->solver->solve(Vs, s->T);
            if (rc != -2) s->V = Vs;
        } else
            rc = s->solver->solve(s->V, s->T);
        if (backend == rails::DirectBackend) s->last = outcome_of(*s->solver, rc, backend);
    } catch (std::bad_alloc const &) {
        rails_set_error("rails_solver_solve: out of host memory");
        return RAILS_ENOMEM;
    } catch (std::exception const &e) {
        rails_set_error("rails_solver_solve: %s", e.what());
        return RAILS_EINVAL;
    }
    s->have_start = false; // one solve consumes the start space
    s->start = rails::HipMultiVectorWrapper();
    s->have_V0 = false; // V now holds the result; a later warm start passes its V again (or runs on the direct back end)
    if (code) *code = rc;
    if (k) *k = s->V.N();
    if (rails_ctx_sync(s->ctx) != RAILS_OK) return RAILS_EHIP;
    // a library call that failed somewhere inside the wrappers (they only print, like the reference's): V and T are not to be trusted
    if (rails::sticky_error() != RAILS_OK) {
        const int err = rails::sticky_error();
        rails_set_error("rails_solver_solve: a device operation failed during the solve (code %d, first failure; see stderr): %s", err, rails_last_error());
        return err;
    }
    return RAILS_OK;
}

extern "C" int rails_solver_get_V(rails_solver *s, double *V_host, int64_t ldv)
{
    if (!s || !V_host || ldv < s->m_local) return RAILS_EINVAL;
    s->V.to_host(V_host, ldv);
    return RAILS_OK;
}

extern "C" int rails_solver_get_T(rails_solver *s, double *T_host, int ldt)
{
    if (!s || !T_host) return RAILS_EINVAL;
    int k = s->T.M();
    if (ldt < k) return RAILS_EINVAL;
    for (int j = 0; j < k; ++j)
        for (int i = 0; i < k; ++i) T_host[i + (size_t)j * ldt] = s->T(i, j);
    return RAILS_OK;
}

extern "C" int rails_solver_trips(rails_solver *s) { return s ? s->last.trips : -1; }

extern "C" int rails_solver_scale(rails_solver *s, double *scale)
{
    if (!s || !scale) return RAILS_EINVAL;
    *scale = s->last.scale;
    return RAILS_OK;
}

extern "C" const char *rails_solver_backend_stats(rails_solver *s) { return s ? s->last.stats.c_str() : "{}"; }

extern "C" int rails_solver_history(rails_solver *s, double *res, int cap)
{
    if (!s) return -1;
    auto const &h = s->last.history;
    int n = (int)h.size();
    for (int i = 0; i < n && i < cap; ++i) res[i] = h[i];
    return n;
}

extern "C" int rails_solver_profile(rails_solver *s, char *buf, int cap)
{
    if (!s || !buf || cap < 2) return RAILS_EINVAL;
    std::string out = "{";
    bool first = true;
    for (auto const &kv : s->last.profile) {
        char tmp[256];
        snprintf(tmp, sizeof(tmp), "%s\"%s\": %.6f", first ? "" : ", ", kv.first.c_str(), kv.second);
        out += tmp;
        first = false;
    }
    out += "}";
    if ((int)out.size() + 1 > cap) return RAILS_EINVAL;
    memcpy(buf, out.c_str(), out.size() + 1);
    return RAILS_OK;
}

// S (order n, symmetric) <- P'P for P = [blk[0] ... blk[nb - 1]], block a at row and column off[a]
static std::vector<double> gram_of_blocks(rails::HipMultiVectorWrapper const *const *blk, const int *off, int nb, int n)
{
    std::vector<double> S((size_t)n * n, 0.0);
    for (int a = 0; a < nb; ++a)
        for (int b = a; b < nb; ++b) {
            rails::HostDenseMatrix C = blk[a]->dot(*blk[b]);
            for (int j = 0; j < C.N(); ++j)
                for (int i = 0; i < C.M(); ++i) S[(off[a] + i) + (size_t)(off[b] + j) * n] = S[(off[b] + j) + (size_t)(off[a] + i) * n] = C(i, j);
        }
    return S;
}

// The same with a sparse B: P = [AV MV], K = [[0 T],[T 0]], Z = B'P;  ||R||_F^2 = tr((P'P K)^2) + 2 tr(K Z'Z) + ||B'B||_F^2
static int sparse_relative_residual(rails_solver *s, rails::HipMultiVectorWrapper const &AV, rails::HipMultiVectorWrapper const &MV, double *rel)
{
    const int k = AV.N(), n = 2 * k;
    const rails::HipOperatorWrapper Bt = s->Bop.transpose();
    rails::HipMultiVectorWrapper ZA = Bt * AV, ZM = Bt * MV; // p x k each
    rails::HipMultiVectorWrapper const *blk[2] = {&AV, &MV}, *zbl[2] = {&ZA, &ZM};
    const int off[2] = {0, k};
    const std::vector<double> S = gram_of_blocks(blk, off, 2, n), W = gram_of_blocks(zbl, off, 2, n);
    // SK = S K: column block 0 of S K is S[:, MV] T, column block 1 is S[:, AV] T
    std::vector<double> SK((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < k; ++j) {
            double s1 = 0.0, s2 = 0.0;
            for (int l = 0; l < k; ++l) {
                s1 += S[i + (size_t)(k + l) * n] * s->T(l, j);
                s2 += S[i + (size_t)l * n] * s->T(l, j);
            }
            SK[i + (size_t)j * n] = s1;
            SK[i + (size_t)(k + j) * n] = s2;
        }
    double tr = 0.0; // tr(SK SK)
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) tr += SK[i + (size_t)j * n] * SK[j + (size_t)i * n];
    double cross = 0.0; // tr(K W) = 2 sum_ij T_ij W[MV_j, AV_i]
    for (int j = 0; j < k; ++j)
        for (int i = 0; i < k; ++i) cross += s->T(i, j) * (W[(k + j) + (size_t)i * n] + W[j + (size_t)(k + i) * n]);
    const double bb = rails_sprhs_gram_norm2(s->sprhs);
    *rel = std::sqrt(std::fabs(tr + 2.0 * cross + bb)) / std::sqrt(bb);
    return RAILS_OK;
}

// ||R||_F with R = P G P^T, P = [AV MV B], G = [[0 T 0],[T 0 0],[0 0 I]]:  ||R||_F^2 = tr(G S G S), S = P^T P
extern "C" int rails_solver_relative_residual(rails_solver *s, double *rel)
{
    if (!s || !rel) return RAILS_EINVAL;
    int k = s->V.N(), p = s->sprhs ? 0 : s->B.N();
    if (k != s->T.M()) {
        rails_set_error("rails_solver_relative_residual: V has %d columns but T is %d x %d", k, s->T.M(), s->T.N());
        return RAILS_EINVAL;
    }
    rails::HipMultiVectorWrapper AV = s->A * s->V;
    rails::HipMultiVectorWrapper MV = s->mass ? (s->M * s->V) : s->V.view();
    if (s->sprhs) return sparse_relative_residual(s, AV, MV, rel);
    int n = 2 * k + p;
    rails::HipMultiVectorWrapper const *blk[3] = {&AV, &MV, &s->B};
    const int off[3] = {0, k, 2 * k};
    const std::vector<double> S = gram_of_blocks(blk, off, 3, n);
    // GS = G * S
    std::vector<double> GS((size_t)n * n, 0.0);
    for (int j = 0; j < n; ++j) {
        for (int i = 0; i < k; ++i) {
            double s1 = 0.0, s2 = 0.0;
            for (int l = 0; l < k; ++l) {
                s1 += s->T(i, l) * S[(k + l) + (size_t)j * n]; // row block 0: T * S[MV rows]
                s2 += s->T(i, l) * S[l + (size_t)j * n];       // row block 1: T * S[AV rows]
            }
            GS[i + (size_t)j * n] = s1;
            GS[(k + i) + (size_t)j * n] = s2;
        }
        for (int i = 0; i < p; ++i) GS[(2 * k + i) + (size_t)j * n] = S[(2 * k + i) + (size_t)j * n];
    }
    double tr = 0.0; // tr(GS * GS)
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) tr += GS[i + (size_t)j * n] * GS[j + (size_t)i * n];
    double bb = 0.0; // ||B B^T||_F^2 = ||B^T B||_F^2
    for (int i = 0; i < p; ++i)
        for (int j = 0; j < p; ++j) {
            double v = S[(2 * k + i) + (size_t)(2 * k + j) * n];
            bb += v * v;
        }
    *rel = std::sqrt(std::fabs(tr)) / std::sqrt(bb);
    return RAILS_OK;
}

// the solution object (include/rails_solution.h) of the last solve: a device copy of V and the host T
extern "C" int rails_solution_from_solver(rails_solver *s, rails_solution **out)
{
    if (!s || !out) {
        rails_set_error("rails_solution_from_solver: null argument");
        return RAILS_EINVAL;
    }
    const int k = s->V.N();
    if (k < 1 || !s->V.panel() || s->T.M() != k || s->T.N() != k) {
        rails_set_error("rails_solution_from_solver: no solution yet (V has %d columns, T is %d x %d)", k, s->T.M(), s->T.N());
        return RAILS_EINVAL;
    }
    return rails_solution_create(s->ctx, s->V.panel(), s->V.offset(), k, (double *)s->T, s->T.LDA(), 1, out);
}
