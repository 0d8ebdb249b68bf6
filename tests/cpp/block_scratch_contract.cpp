// The overlapped block orthogonalisation of rails::SubspaceBasis with the block in its compact scratch panel against the same chain
// with the block in the basis panel's tail (SubspaceBasis::block_scratch, RAILS_SUBSPACE_BLOCK_SCRATCH): only addresses differ, so the
// basis panel and the coordinates have to agree bit for bit.  The block shapes are forced here, on the basis object itself -- through
// the solver nobody chooses whether a block needs a second round:
//   * no second round (w2 == 0: random columns keep nearly all their length outside a small basis): no fused pass, the first scaling
//     moves the block into the scratch panel;
//   * a second round on the leading two columns, behind a basis of 10 columns (the two separate kernels: the block is copied to the
//     scratch panel) and of 42 columns (k_update_gram writes it there; 42 is no multiple of 4: the kernel's loads run on into the block);
//   * a block wider than the one before (the scratch panel grows) and a narrower one after it (it is kept).
// Run by tests/test_gpu_block_scratch.py; needs a gfx950 GPU.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rails/HipSolverOps.hpp"
#include "rails/SubspaceSolverOps.hpp"

using rails::HipMultiVectorWrapper;
using rails::SubspaceBasis;
using rails::SubspaceMultiVector;

static int g_fail = 0, g_checks = 0;
static const char *g_case = "";

#define CHECK(cond)                                                                 \
    do {                                                                            \
        ++g_checks;                                                                 \
        if (!(cond)) {                                                              \
            ++g_fail;                                                               \
            std::printf("FAIL [%s] %s:%d: %s\n", g_case, __FILE__, __LINE__, #cond); \
        }                                                                           \
    } while (0)

static std::vector<double> host_of(HipMultiVectorWrapper const &v)
{
    const int m = (int)v.local_rows(), n = v.N();
    std::vector<double> h((size_t)m * std::max(n, 0));
    if (n > 0) v.to_host(h.data(), m);
    return h;
}

static bool same_bits(std::vector<double> const &a, std::vector<double> const &b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0);
}

struct Outcome {
    std::vector<double> panel, coef;
    long overlapped = 0, second = 0, scratch = 0;
    int dim = 0;
};

// a basis of nb random columns, then blocks of the widths in `widths` absorbed in the overlapped form; the leading `mixed` columns of
// every block keep 30 % of their squared length outside the basis (they take the second round), the others are random
static Outcome run(rails_ctx *ctx, uint64_t seed, uint64_t stream, bool scratch, int m, int nb, std::vector<int> const &widths, int mixed)
{
    Outcome out;
    CHECK(rails_ctx_set_seed(ctx, seed, stream) == 0);
    auto basis = std::make_shared<SubspaceBasis>(ctx, m, m, 16);
    basis->block_scratch = scratch;
    basis->overlap = true;
    SubspaceMultiVector p(basis, nb);
    p.random();
    HipMultiVectorWrapper inside = p.materialise().copy();
    const std::vector<double> hi = host_of(inside);
    const long scratch_start = basis->n_scratch_blocks, overlapped_start = basis->n_overlapped;
    for (int w : widths) {
        HipMultiVectorWrapper X(m, w, ctx);
        X.random();
        std::vector<double> hx = host_of(X);
        for (int j = 0; j < mixed; ++j) {
            double ni = 0.0, no = 0.0;
            std::vector<double> in(m);
            for (int i = 0; i < m; ++i) {
                in[i] = hi[i + (size_t)(2 + j) * m] - 0.5 * hi[i + (size_t)(7 - j) * m];
                ni += in[i] * in[i];
                no += hx[i + j * (size_t)m] * hx[i + j * (size_t)m];
            }
            for (int i = 0; i < m; ++i) hx[i + j * (size_t)m] = std::sqrt(0.7 / ni) * in[i] + std::sqrt(0.3 / no) * hx[i + j * (size_t)m];
        }
        X.from_host(hx.data(), m);
        const long second_before = basis->n_second_round, overlapped_before = basis->n_overlapped, scratch_before = basis->n_scratch_blocks;
        const int dim_before = basis->dim;
        SubspaceMultiVector c = SubspaceMultiVector::Absorb(basis, X);
        CHECK(basis->n_overlapped == overlapped_before + 1);                // the chain under test was queued
        CHECK(basis->n_second_round == second_before + (mixed > 0 ? 1 : 0)); // ... in the branch this case is about
        CHECK(basis->n_scratch_blocks == scratch_before + (scratch ? 1 : 0));
        CHECK(basis->dim == dim_before + w);
        HipMultiVectorWrapper image = c.materialise().copy(); // (the block is read back here)
        CHECK(!basis->failed);
        for (int j = 0; j < w; ++j)
            for (int i = 0; i < c.coefficient_rows(); ++i) out.coef.push_back(c.coefficients()[i + (size_t)j * c.coefficient_ld()]);
    }
    out.panel = host_of(basis->P);
    out.dim = basis->dim;
    out.overlapped = basis->n_overlapped - overlapped_start;
    out.second = basis->n_second_round;
    out.scratch = basis->n_scratch_blocks - scratch_start;
    // the result is a basis: orthonormal to rounding (the chain really ran to its end in P's tail)
    rails::HostDenseMatrix G = basis->P.dot(basis->P);
    double worst = 0.0;
    for (int j = 0; j < out.dim; ++j)
        for (int i = 0; i < out.dim; ++i) worst = std::max(worst, std::abs(G(i, j) - (i == j ? 1.0 : 0.0)));
    CHECK(worst < 1e-13);
    return out;
}

static void compare(rails_ctx *ctx, const char *name, int m, int nb, std::vector<int> const &widths, int mixed)
{
    g_case = name;
    uint64_t seed = 0, stream = 0;
    CHECK(rails_ctx_rng_state(ctx, &seed, &stream) == 0);
    const Outcome off = run(ctx, seed, stream, false, m, nb, widths, mixed), on = run(ctx, seed, stream, true, m, nb, widths, mixed);
    CHECK(off.scratch == 0 && on.scratch == (long)widths.size() && on.overlapped == off.overlapped);
    CHECK(on.dim == off.dim && on.second == off.second);
    CHECK(!on.panel.empty() && same_bits(on.panel, off.panel));
    CHECK(!on.coef.empty() && same_bits(on.coef, off.coef));
    std::printf("%s: dim %d, %ld blocks through the scratch panel, panel and coordinates %s\n", name, on.dim, on.scratch,
                same_bits(on.panel, off.panel) && same_bits(on.coef, off.coef) ? "bit for bit" : "DIFFER");
}

int main()
{
    setvbuf(stdout, nullptr, _IONBF, 0);
    if (rails_host_lapack_init(nullptr) != RAILS_OK) {
        std::printf("no host LAPACK: %s\n", rails_last_error());
        return 2;
    }
    rails_ctx *ctx = nullptr;
    if (rails_ctx_create(0, nullptr, &ctx) != RAILS_OK) {
        std::printf("rails_ctx_create failed: %s\n", rails_last_error());
        return 2;
    }
    rails_ctx_set_seed(ctx, 23, 0);
    rails::set_default_context(ctx);
    const int m = 4133; // the fused kernel runs from 4096 rows on; no multiple of 16
    compare(ctx, "no second round: the first scaling moves the block", m, 12, {5}, 0);
    compare(ctx, "no second round, 17 columns, 300 rows", 300, 12, {17}, 0);
    compare(ctx, "second round behind 10 columns: the two separate kernels", m, 10, {5}, 2);
    compare(ctx, "second round behind 42 columns: the fused pass", m, 42, {17}, 2);
    compare(ctx, "the scratch panel grows and is kept", m, 12, {5, 9, 4}, 0);
    rails_ctx_destroy(ctx);
    std::printf("%d checks, %d failures\n", g_checks, g_fail);
    if (g_fail == 0) std::printf("ALL PASSED\n");
    return g_fail == 0 ? 0 : 1;
}
