// The block-Jacobi preconditioner of the iterative A^-1 object through the C ABI alone (include/rails_hip.h, nothing else): a chain of 50
// cells of 3 unknowns whose coupling inside a cell is stiff (the cell's block is -(C_i + 2 I) with C_i symmetric, eigenvalues 1, 30 and
// 1000 in a basis that turns from cell to cell; the neighbours couple through I) as a CSR handle, a rails_iter (conjugate gradients),
// the point-Jacobi solve as the count to beat, the blocks taken from the CSR arrays, rails_iter_block_jacobi_info, the solve checked by its
// true residual on the host, the same bits from blocks passed explicitly, the toggle, the clearing call and the refusals a C caller meets.
// Built by rails_amd/csrc/Makefile into rails_amd/lib/iter_block_jacobi_capi, run by tests/test_gpu_block_jacobi_cpp.py.  Prints OK at the
// end.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rails_hip.h"

static int failures = 0;
#define CHECK(cond, ...)                   \
    do {                                   \
        if (!(cond)) {                     \
            std::printf("FAILED: " __VA_ARGS__); \
            std::printf("\n");             \
            failures++;                    \
        }                                  \
    } while (0)
#define MUST(call)                                                           \
    do {                                                                     \
        if ((call) != RAILS_OK) {                                            \
            std::printf("%s: %s\nFAILED\n", #call, rails_last_error());      \
            return 1;                                                        \
        }                                                                    \
    } while (0)

int main()
{
    const int nb = 50, b = 3, m = nb * b, nc = 3;
    const double tol = 1e-10;
    std::vector<double> blocks((size_t)nb * b * b);
    for (int i = 0; i < nb; ++i) {
        const double v[3] = {1.0, std::sin(i + 1.0), std::cos(2.0 * i + 1.0)}, lam[3] = {1.0, 30.0, 1000.0};
        const double vv = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
        double Q[3][3];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) Q[r][c] = (r == c ? 1.0 : 0.0) - 2.0 * v[r] * v[c] / vv;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c <= r; ++c) {
                double s = 0.0;
                for (int l = 0; l < 3; ++l) s += Q[r][l] * lam[l] * Q[c][l];
                blocks[(size_t)i * 9 + r * 3 + c] = blocks[(size_t)i * 9 + c * 3 + r] = -(s + (r == c ? 2.0 : 0.0));
            }
    }
    std::vector<int64_t> rp(1, 0);
    std::vector<int32_t> ci;
    std::vector<double> va;
    for (int i = 0; i < nb; ++i)
        for (int r = 0; r < b; ++r) {
            if (i > 0) ci.push_back((i - 1) * b + r), va.push_back(1.0);
            for (int c = 0; c < b; ++c) ci.push_back(i * b + c), va.push_back(blocks[(size_t)i * 9 + r * 3 + c]);
            if (i < nb - 1) ci.push_back((i + 1) * b + r), va.push_back(1.0);
            rp.push_back((int64_t)ci.size());
        }
    rails_ctx *ctx = nullptr;
    if (rails_ctx_create(0, nullptr, &ctx) != RAILS_OK) {
        std::printf("no gfx950 device: %s\n", rails_last_error());
        return 2;
    }
    rails_csr *A = nullptr;
    rails_iter *it = nullptr;
    rails_panel *X = nullptr, *Y = nullptr;
    MUST(rails_csr_create(ctx, m, m, rp.data(), ci.data(), va.data(), &A));
    MUST(rails_iter_create(ctx, A, RAILS_ITER_CG, nullptr, &it));
    MUST(rails_iter_set(it, "tolerance", tol));
    MUST(rails_panel_create(ctx, m, nc, &X));
    MUST(rails_panel_create(ctx, m, nc, &Y));
    std::vector<double> xh((size_t)m * nc), yh((size_t)m * nc), y1, y2;
    for (int j = 0; j < nc; ++j)
        for (int i = 0; i < m; ++i) xh[i + (size_t)j * m] = std::sin(0.37 * (i + 1) * (j + 1)) + 0.25 * ((i * 7 + j) % 5);
    MUST(rails_panel_upload(ctx, X, 0, nc, xh.data(), m));

    auto residual = [&]() {
        double worst = 0.0;
        for (int j = 0; j < nc; ++j) {
            double rr = 0.0, bb = 0.0;
            for (int i = 0; i < m; ++i) {
                double s = 0.0;
                for (int64_t q = rp[i]; q < rp[i + 1]; ++q) s += va[q] * yh[ci[q] + (size_t)j * m];
                rr += (s - xh[i + (size_t)j * m]) * (s - xh[i + (size_t)j * m]);
                bb += xh[i + (size_t)j * m] * xh[i + (size_t)j * m];
            }
            worst = std::fmax(worst, std::sqrt(rr / bb));
        }
        return worst;
    };
    auto solve = [&](std::vector<double> *keep, double *most) {
        double st[19] = {};
        if (rails_panel_fill(ctx, Y, 0, nc, 0.0) != RAILS_OK || rails_iter_solve(ctx, it, 0, X, 0, nc, Y, 0) != RAILS_OK ||
            rails_panel_download(ctx, Y, 0, nc, yh.data(), m) != RAILS_OK)
            return false;
        rails_iter_stats(it, st, 19);
        *most = st[0];
        if (keep) *keep = yh;
        return st[3] == 0.0;
    };

    // point Jacobi first: the count to beat
    double point = 0, block = 0, again = 0;
    std::vector<double> y_point;
    CHECK(solve(&y_point, &point) && residual() <= 10 * tol, "the point-Jacobi solve: %s", rails_last_error());
    std::printf("point Jacobi: most iterations %g, true residual %.2e\n", point, residual());
    int bb = -1;
    CHECK(rails_iter_block_jacobi_info(it, &bb, nullptr, 0) == 0 && bb == 0, "no blocks before any are installed");
    CHECK(rails_iter_set(it, "block_jacobi", 1) == RAILS_EINVAL && std::strstr(rails_last_error(), "without blocks"), "\"block_jacobi\" 1 without blocks");

    // the blocks from the CSR arrays, the info
    MUST(rails_iter_block_jacobi(ctx, it, b, nullptr));
    std::vector<double> inv((size_t)nb * 9, 0.0), inv2((size_t)nb * 9, -1.0);
    CHECK(rails_iter_block_jacobi_info(it, &bb, inv.data(), nb) == nb && bb == b, "the info");
    double worst = 0.0;
    for (int i = 0; i < nb; ++i)
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                double s = 0.0;
                for (int l = 0; l < 3; ++l) s += inv[(size_t)i * 9 + r * 3 + l] * blocks[(size_t)i * 9 + l * 3 + c];
                worst = std::fmax(worst, std::fabs(s - (r == c ? 1.0 : 0.0)));
            }
    std::printf("block Jacobi: %d blocks of %d x %d, |G D - I| at most %.2e\n", nb, bb, bb, worst);
    CHECK(worst <= 1e-12, "the inverses");
    CHECK(rails_iter_block_jacobi_info(it, nullptr, inv2.data(), 2) == nb && inv2[17] == inv[17] && inv2[18] == -1.0, "cap_blocks limits what is written");

    // the solve
    CHECK(solve(&y1, &block) && residual() <= 10 * tol, "the block-Jacobi solve: %s", rails_last_error());
    std::printf("block Jacobi: most iterations %g, unconverged columns 0, true residual %.2e\n", block, residual());
    CHECK(block >= 1 && 2 * block < point, "%g iterations against point Jacobi's %g", block, point);
    // the same blocks passed explicitly: the same inverses and the same bits
    MUST(rails_iter_block_jacobi(ctx, it, b, blocks.data()));
    CHECK(rails_iter_block_jacobi_info(it, &bb, inv2.data(), nb) == nb && std::memcmp(inv.data(), inv2.data(), inv.size() * sizeof(double)) == 0, "explicit blocks: the inverses");
    CHECK(solve(&y2, &again) && again == block && std::memcmp(y1.data(), y2.data(), y1.size() * sizeof(double)) == 0, "explicit blocks: the solve");
    // the toggle: point Jacobi again, bit for bit; and back
    MUST(rails_iter_set(it, "block_jacobi", 0));
    CHECK(solve(&y2, &again) && again == point && std::memcmp(y_point.data(), y2.data(), y2.size() * sizeof(double)) == 0, "\"block_jacobi\" 0 is the point-Jacobi solve");
    MUST(rails_iter_set(it, "block_jacobi", 1));
    CHECK(solve(&y2, &again) && again == block && std::memcmp(y1.data(), y2.data(), y1.size() * sizeof(double)) == 0, "\"block_jacobi\" 1 again");

    // refusals; the object stays usable
    CHECK(rails_iter_block_jacobi(ctx, it, 4, nullptr) == RAILS_EINVAL && std::strstr(rails_last_error(), "does not divide"), "b = 4 on 150 rows");
    CHECK(rails_iter_block_jacobi(ctx, it, 9, blocks.data()) == RAILS_EINVAL && std::strstr(rails_last_error(), "2 .. 8"), "b = 9");
    CHECK(rails_iter_set(it, "poly_degree", 2) == RAILS_EINVAL && std::strstr(rails_last_error(), "block_jacobi"), "poly_degree with block_jacobi on");
    CHECK(rails_iter_set(it, "amg", 1) == RAILS_EINVAL && std::strstr(rails_last_error(), "block_jacobi"), "amg with block_jacobi on");
    std::vector<double> singular(blocks);
    for (int c = 0; c < 9; ++c) singular[(size_t)7 * 9 + c] = 0.0;
    CHECK(rails_iter_block_jacobi(ctx, it, b, singular.data()) == RAILS_EINVAL && std::strstr(rails_last_error(), "block 7 "), "a singular block is named");
    CHECK(solve(&y2, &again) && again == block && std::memcmp(y1.data(), y2.data(), y1.size() * sizeof(double)) == 0, "the refusals left the blocks alone");
    // clearing
    MUST(rails_iter_block_jacobi(ctx, it, 0, nullptr));
    CHECK(rails_iter_block_jacobi_info(it, &bb, nullptr, 0) == 0 && bb == 0, "cleared");
    CHECK(rails_iter_set(it, "block_jacobi", 1) == RAILS_EINVAL, "\"block_jacobi\" 1 after clearing");
    CHECK(solve(&y2, &again) && again == point && std::memcmp(y_point.data(), y2.data(), y2.size() * sizeof(double)) == 0, "cleared: the point-Jacobi solve");

    rails_panel_destroy(X);
    rails_panel_destroy(Y);
    rails_iter_destroy(it);
    rails_csr_destroy(A);
    rails_ctx_destroy(ctx);
    if (failures) {
        std::printf("%d FAILED\n", failures);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
