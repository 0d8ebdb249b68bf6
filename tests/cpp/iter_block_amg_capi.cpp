// The block multigrid preconditioner of the iterative A^-1 object through the C ABI alone (include/rails_hip.h, nothing else): a 7-point
// grid of 8 x 8 x 8 cells with 3 unknowns each, the matrix -(L (x) K + 0.01 blockdiag(C_i)) as a block-CSR handle, a rails_iter (conjugate
// gradients) with "block_amg" and the four "amg_..." settings through rails_iter_set, rails_iter_block_amg_setup,
// rails_iter_block_amg_info, a solve of three columns checked by its true residual on the host, fewer than half of the iterations of the
// block-Jacobi solve of the same object, and the refusals a C caller meets.  Built by rails_amd/csrc/Makefile into
// rails_amd/lib/iter_block_amg_capi, run by tests/test_gpu_block_amg_cpp.py.  Prints OK at the end.
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
    const int k = 8, b = 3, mb = k * k * k, m = mb * b, nc = 3;
    const double tol = 1e-8;
    // K: symmetric positive definite with eigenvalues spread over two decades; C_i: diagonally dominant, different in every cell
    const double K[3][3] = {{40.0, 9.0, 2.0}, {9.0, 6.0, 1.0}, {2.0, 1.0, 1.5}};
    std::vector<int64_t> brp(1, 0);
    std::vector<int32_t> bci;
    std::vector<double> bva;
    auto block = [&](int c, double scale, int cell) {
        bci.push_back(c);
        for (int r = 0; r < b; ++r)
            for (int s = 0; s < b; ++s) {
                double v = scale * K[r][s];
                if (cell >= 0) v -= 0.01 * (r == s ? 5.0 + (cell * 7 + r) % 11 : 0.5 * ((cell + r + s) % 3));
                bva.push_back(v);
            }
    };
    for (int z = 0; z < k; ++z)
        for (int y = 0; y < k; ++y)
            for (int x = 0; x < k; ++x) {
                const int r = x + k * (y + k * z);
                if (z > 0) block(r - k * k, 1.0, -1);
                if (y > 0) block(r - k, 1.0, -1);
                if (x > 0) block(r - 1, 1.0, -1);
                block(r, -6.0, r);
                if (x < k - 1) block(r + 1, 1.0, -1);
                if (y < k - 1) block(r + k, 1.0, -1);
                if (z < k - 1) block(r + k * k, 1.0, -1);
                brp.push_back((int64_t)bci.size());
            }
    rails_ctx *ctx = nullptr;
    if (rails_ctx_create(0, nullptr, &ctx) != RAILS_OK) {
        std::printf("no gfx950 device: %s\n", rails_last_error());
        return 2;
    }
    rails_csr *A = nullptr;
    rails_iter *it = nullptr, *bi = nullptr;
    rails_panel *X = nullptr, *Y = nullptr;
    MUST(rails_csr_create_bsr(ctx, mb, mb, b, brp.data(), bci.data(), bva.data(), &A));
    MUST(rails_iter_create(ctx, A, RAILS_ITER_CG, nullptr, &it));
    MUST(rails_iter_set(it, "tolerance", tol));
    MUST(rails_panel_create(ctx, m, nc, &X));
    MUST(rails_panel_create(ctx, m, nc, &Y));
    std::vector<double> xh((size_t)m * nc), yh((size_t)m * nc);
    for (int j = 0; j < nc; ++j)
        for (int i = 0; i < m; ++i) xh[i + (size_t)j * m] = std::sin(0.37 * (i + 1) * (j + 1)) + 0.25 * ((i * 7 + j) % 5);
    MUST(rails_panel_upload(ctx, X, 0, nc, xh.data(), m));

    auto residual = [&]() {
        double worst = 0.0;
        for (int j = 0; j < nc; ++j) {
            double rr = 0.0, bb = 0.0;
            for (int I = 0; I < mb; ++I)
                for (int r = 0; r < b; ++r) {
                    double s = 0.0;
                    for (int64_t q = brp[I]; q < brp[I + 1]; ++q)
                        for (int c = 0; c < b; ++c) s += bva[(size_t)q * b * b + r * b + c] * yh[(size_t)bci[q] * b + c + (size_t)j * m];
                    const double x = xh[(size_t)I * b + r + (size_t)j * m];
                    rr += (s - x) * (s - x);
                    bb += x * x;
                }
            worst = std::fmax(worst, std::sqrt(rr / bb));
        }
        return worst;
    };

    // block Jacobi first: the count to beat
    double st[19] = {};
    MUST(rails_iter_block_jacobi(ctx, it, 0, nullptr));
    MUST(rails_iter_solve(ctx, it, 0, X, 0, nc, Y, 0));
    MUST(rails_panel_download(ctx, Y, 0, nc, yh.data(), m));
    rails_iter_stats(it, st, 19);
    const double jacobi_iterations = st[0];
    std::printf("block Jacobi: most iterations %g, true residual %.2e\n", st[0], residual());
    CHECK(residual() <= 10 * tol && st[3] == 0.0, "the block-Jacobi solve");
    int64_t rows[20], nnz[20];
    double hi[20];
    CHECK(rails_iter_block_amg_info(it, rows, nnz, hi, 20) == 0, "no hierarchy before \"block_amg\" is used");
    CHECK(rails_iter_set(it, "block_amg", 1) == RAILS_EINVAL && std::strstr(rails_last_error(), "one preconditioner at a time"), "block_amg with block_jacobi on");
    MUST(rails_iter_set(it, "block_jacobi", 0));

    // the settings, the set-up, the info
    MUST(rails_iter_set(it, "amg_degree", 1));
    MUST(rails_iter_set(it, "amg_ratio", 4));
    MUST(rails_iter_set(it, "amg_theta", 0.08));
    MUST(rails_iter_set(it, "amg_coarse", 256));
    MUST(rails_iter_set(it, "block_amg", 1));
    MUST(rails_iter_block_amg_setup(ctx, it));
    const int levels = rails_iter_block_amg_info(it, rows, nnz, hi, 20);
    std::printf("levels %d:", levels);
    for (int l = 0; l < levels; ++l) std::printf(" %lld rows %lld entries hi %.3f;", (long long)rows[l], (long long)nnz[l], hi[l]);
    std::printf(" operator complexity %.2f\n", levels > 0 ? hi[levels + 1] : 0.0);
    CHECK(levels >= 2 && levels <= 16 && rows[0] == m && nnz[0] == (int64_t)bva.size() && rows[levels - 1] <= 256 && hi[levels - 1] == 0.0, "the hierarchy");
    for (int l = 0; l < levels; ++l) CHECK(rows[l] % b == 0, "level %d: %lld rows are no multiple of b", l, (long long)rows[l]);
    for (int l = 0; l + 1 < levels; ++l) CHECK(rows[l + 1] * 5 <= rows[l] * 4 && hi[l] > 0.0, "level %d", l);
    CHECK(levels > 0 && hi[levels + 1] > 1.0 && hi[levels + 1] < 2.5, "operator complexity");
    CHECK(rails_iter_amg_info(it, rows, nnz, hi, 20) == 0, "rails_iter_amg_info does not speak for the block hierarchy");
    int64_t two[2] = {-1, -1};
    CHECK(rails_iter_block_amg_info(it, two, nullptr, nullptr, 1) == levels && two[0] == m && two[1] == -1, "cap limits what is written");

    // the solve
    MUST(rails_panel_fill(ctx, Y, 0, nc, 0.0));
    MUST(rails_iter_solve(ctx, it, 0, X, 0, nc, Y, 0));
    MUST(rails_panel_download(ctx, Y, 0, nc, yh.data(), m));
    rails_iter_stats(it, st, 19);
    rails_iter_block_amg_info(it, rows, nnz, hi, 20);
    std::printf("block multigrid: most iterations %g, unconverged columns %g, cycles %lld, products in them %lld, launches in them %g, true residual %.2e\n", st[0], st[3],
                (long long)rows[levels], (long long)nnz[levels], hi[levels], residual());
    CHECK(residual() <= 10 * tol && st[3] == 0.0, "the multigrid solve");
    CHECK(st[0] >= 1 && 2 * st[0] <= jacobi_iterations, "%g iterations against block Jacobi's %g", st[0], jacobi_iterations);
    CHECK(rows[levels] >= st[0] + 1 && nnz[levels] == rows[levels] * (levels - 1) * 6 && hi[levels] == (double)(rows[levels] * ((levels - 1) * 6 + 1)), "the counts per cycle");
    int32_t iters[3], flags[3];
    CHECK(rails_iter_columns(it, iters, nullptr, flags, 3) == 3 && flags[0] == 2 && flags[1] == 2 && flags[2] == 2, "every column converged");

    // one cycle on its own is a preconditioner: finite, of the operator's sign
    MUST(rails_iter_precondition(ctx, it, X, 0, nc, Y, 0));
    MUST(rails_panel_download(ctx, Y, 0, nc, yh.data(), m));
    for (int j = 0; j < nc; ++j) {
        double xz = 0.0;
        for (int i = 0; i < m; ++i) xz += xh[i + (size_t)j * m] * yh[i + (size_t)j * m];
        CHECK(std::isfinite(xz) && xz < 0.0, "x' M x = %g in column %d", xz, j);
    }

    // refusals
    CHECK(rails_iter_set(it, "poly_degree", 2) == RAILS_EINVAL && std::strstr(rails_last_error(), "block_amg"), "poly_degree with block_amg on");
    CHECK(rails_iter_set(it, "amg", 1) == RAILS_EINVAL, "amg with block_amg on");
    CHECK(rails_iter_block_jacobi(ctx, it, 0, nullptr) == RAILS_EINVAL && std::strstr(rails_last_error(), "one preconditioner at a time"), "block Jacobi with block_amg on");
    CHECK(rails_iter_set(it, "amg_coarse", 2000) == RAILS_EINVAL, "amg_coarse 2000");
    CHECK(rails_iter_set(it, "no_such_setting", 1) == RAILS_EINVAL && std::strstr(rails_last_error(), "block_amg"), "the list of settings names block_amg");
    MUST(rails_iter_create(ctx, A, RAILS_ITER_BICGSTAB, nullptr, &bi));
    CHECK(rails_iter_set(bi, "block_amg", 1) == RAILS_EINVAL && std::strstr(rails_last_error(), "BiCGStab"), "block_amg on a BiCGStab object");
    CHECK(rails_iter_block_amg_setup(ctx, bi) == RAILS_EINVAL, "the set-up on a BiCGStab object");
    rails_iter_destroy(bi);
    // the object still solves
    MUST(rails_iter_solve(ctx, it, 0, X, 0, nc, Y, 0));
    MUST(rails_panel_download(ctx, Y, 0, nc, yh.data(), m));
    CHECK(residual() <= 10 * tol, "a solve after the refusals");

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
