// tile_plan_host.cpp -- the tile plan of the LDS-staged SpMM (rails_amd/csrc/tile_plan.cpp) checked on the host: no HIP, no library.
//
// usage: tile_plan_host <max_row_nnz> <max_fp> <reuse>   (of the banded pattern, computed by tests/test_tile_plan_host.py in numpy)
//
// Every pattern is generated in here.  For each one the program checks what the kernels of spmm_tiled.hip rely on: every row in exactly
// one tile of at most 256 rows, per-tile row offsets, sorted footprints, every nonzero mapped back to its column and value through its
// LDS row, distinct LDS rows below max_pos, the halo-box layout of box tiles (and the fall-back of tiles that do not fit it), the
// padding element, and that "entry 0 of a row" and "footprint row 0 of a tile" -- which the register kernel loads unconditionally --
// index inside the arrays.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "../../rails_amd/csrc/tile_plan.h"

namespace {

struct Csr {
    std::vector<int64_t> rowptr{0};
    std::vector<int32_t> col;
    std::vector<double> val;
    int64_t m() const { return (int64_t)rowptr.size() - 1; }
    int max_row_nnz() const
    {
        int64_t mx = 0;
        for (int64_t i = 0; i < m(); ++i) mx = std::max(mx, rowptr[i + 1] - rowptr[i]);
        return (int)mx;
    }
    void add_row(std::vector<int32_t> c)
    {
        std::sort(c.begin(), c.end());
        for (int32_t x : c) {
            col.push_back(x);
            val.push_back(1.0 + 0.25 * (double)(col.size() % 61)); // distinct enough to catch a value that moved
        }
        rowptr.push_back((int64_t)col.size());
    }
};

uint32_t mix(uint64_t a, uint64_t b) { return (uint32_t)((a * 2654435761ull + b * 40503ull + 12345ull) & 0xffffffffull); }

// n - 1 off-diagonal entries at i +- (1 .. bw), reflected at the ends, and the diagonal; columns may repeat inside a row.
// tests/test_tile_plan_host.py generates the same pattern in numpy.
Csr banded(int64_t m, int n, int bw)
{
    Csr A;
    for (int64_t i = 0; i < m; ++i) {
        std::vector<int32_t> c;
        for (int k = 0; k < n - 1; ++k) {
            const uint32_t h = mix((uint64_t)i, (uint64_t)k);
            const int64_t off = 1 + (h >> 8) % (uint32_t)bw;
            int64_t j = ((h >> 4) & 1u) ? i + off : i - off;
            if (j < 0 || j >= m) j = 2 * i - j;
            c.push_back((int32_t)j);
        }
        c.push_back((int32_t)i);
        A.add_row(c);
    }
    return A;
}

// 7-point (full = false) or 27-point stencil on gx x gy x gz in natural ordering
Csr stencil(int gx, int gy, int gz, bool full)
{
    Csr A;
    for (int z = 0; z < gz; ++z)
        for (int y = 0; y < gy; ++y)
            for (int x = 0; x < gx; ++x) {
                std::vector<int32_t> c;
                for (int dz = -1; dz <= 1; ++dz)
                    for (int dy = -1; dy <= 1; ++dy)
                        for (int dx = -1; dx <= 1; ++dx) {
                            if (!full && std::abs(dx) + std::abs(dy) + std::abs(dz) > 1) continue;
                            const int xx = x + dx, yy = y + dy, zz = z + dz;
                            if (xx < 0 || xx >= gx || yy < 0 || yy >= gy || zz < 0 || zz >= gz) continue;
                            c.push_back((int32_t)((zz * gy + yy) * gx + xx));
                        }
                A.add_row(c);
            }
    return A;
}

// rows of 0 to about 30 distinct entries within |j - i| <= 60; every 37th row and the last `empty_tail` rows are empty
Csr ragged(int64_t m, int64_t empty_tail)
{
    Csr A;
    for (int64_t i = 0; i < m; ++i) {
        std::vector<int32_t> c;
        if (i % 37 != 0 && i < m - empty_tail) {
            const uint32_t density = mix((uint64_t)i, 7) % 31;
            for (int64_t j = std::max<int64_t>(0, i - 60); j <= std::min(m - 1, i + 60); ++j)
                if (mix((uint64_t)i, (uint64_t)(1000 + j)) % 121 < density) c.push_back((int32_t)j);
        }
        A.add_row(c);
    }
    return A;
}

// 7-point pattern of a 16 x 24 x 24 grid (m = 9216: the grid detection samples every second row, the even ones).  On the odd rows with
// x = 1 mod 4, y even, z mod 8 < 4 the x+1 neighbour is replaced by the column 4003 rows on (3 further in x, 10 in y, 10 in z): the
// sampled rows still say `grid`, but the tiles of every other layer of 4 x 4 x 4 boxes have columns outside their halo box
Csr box_fail()
{
    const Csr L = stencil(16, 24, 24, false);
    const int64_t m = L.m();
    Csr A;
    for (int64_t i = 0; i < m; ++i) {
        std::vector<int32_t> c(L.col.begin() + L.rowptr[i], L.col.begin() + L.rowptr[i + 1]);
        const int64_t x = i % 16, y = (i / 16) % 24, z = i / (16 * 24);
        if (x % 4 == 1 && y % 2 == 0 && z % 8 < 4)
            for (int32_t &j : c)
                if (j == i + 1) j = (int32_t)((i + 4003) % m);
        A.add_row(c);
    }
    return A;
}

int failures = 0;
#define CHECK(cond, ...)                                    \
    do {                                                    \
        if (!(cond)) {                                      \
            if (failures++ < 20) {                          \
                std::printf("FAIL %s: %s: ", name, #cond);  \
                std::printf(__VA_ARGS__);                   \
                std::printf("\n");                          \
            }                                               \
            return;                                         \
        }                                                   \
    } while (0)

struct Expect {
    bool grid;
    int64_t gx, gy, gz;
    int bx, by, bz;          // boxes, when grid
    int64_t failing_tiles;   // box tiles expected to fall back to consecutive LDS rows
};

void check(const char *name, const Csr &A, const Expect &E, rails_tile_plan &P)
{
    const int64_t m = A.m(), nnz = A.rowptr[m];
    int64_t nx = 0, ny = 0, nz = 0;
    const bool grid = rails_detect_grid(m, A.rowptr.data(), A.col.data(), &nx, &ny, &nz);
    CHECK(grid == E.grid, "detected %d", (int)grid);
    if (grid) CHECK(nx == E.gx && ny == E.gy && nz == E.gz, "%lld x %lld x %lld", (long long)nx, (long long)ny, (long long)nz);

    const rails_tile_params prm; // 64 rows, boxes on, Morton on, 8-column chunks
    const bool ok = rails_tile_plan_build(prm, m, A.rowptr.data(), A.col.data(), A.val.data(), A.max_row_nnz(), P);
    CHECK(ok, "%s", P.why.c_str());
    CHECK(P.grid == E.grid, "plan.grid %d", (int)P.grid);
    if (P.grid) CHECK(P.gx == E.gx && P.gy == E.gy && P.gz == E.gz && P.bx == E.bx && P.by == E.by && P.bz == E.bz, "boxes %d x %d x %d", P.bx, P.by, P.bz);
    const int64_t nt = P.n_tiles;
    CHECK(nt > 0 && (int64_t)P.t_rowptr.size() == nt + 1 && (int64_t)P.t_nzptr.size() == nt + 1 && (int64_t)P.fp_ptr.size() == nt + 1, "n_tiles %lld", (long long)nt);
    CHECK((int64_t)P.t_rows.size() == m && (int64_t)P.t_rp.size() == m + nt, "t_rows %zu t_rp %zu", P.t_rows.size(), P.t_rp.size());
    // the padding element
    CHECK((int64_t)P.t_val.size() == nnz + 1 && (int64_t)P.t_lcol.size() == nnz + 1, "t_val %zu t_lcol %zu nnz %lld", P.t_val.size(), P.t_lcol.size(), (long long)nnz);
    CHECK((int64_t)P.fp.size() == (int64_t)P.fp_ptr[nt] + 1 && P.fp_pos.size() == P.fp.size(), "fp %zu fp_pos %zu", P.fp.size(), P.fp_pos.size());
    CHECK(P.t_rowptr[0] == 0 && P.t_rowptr[nt] == m && P.t_nzptr[0] == 0 && P.t_nzptr[nt] == nnz && P.fp_ptr[0] == 0, "ends");

    std::vector<int> seen(m, 0);
    int max_fp = 0, max_nz = 0, max_rows = 0;
    int64_t failing = 0;
    for (int64_t t = 0; t < nt; ++t) {
        const int tr0 = P.t_rowptr[t], nrows = P.t_rowptr[t + 1] - tr0;
        const int64_t z0 = P.t_nzptr[t];
        const int tnz = (int)(P.t_nzptr[t + 1] - z0);
        const int f0 = P.fp_ptr[t], nf = P.fp_ptr[t + 1] - f0;
        CHECK(nrows >= 1 && nrows <= 256 && tnz >= 0 && nf >= 0, "tile %lld: %d rows", (long long)t, nrows);
        max_fp = std::max(max_fp, nf);
        max_nz = std::max(max_nz, tnz);
        max_rows = std::max(max_rows, nrows);
        // what the register kernel loads whatever the tile holds: footprint row 0, and per row slot the offsets and entry 0
        CHECK(f0 < (int)P.fp.size() && f0 < (int)P.fp_pos.size(), "tile %lld: footprint row 0 outside", (long long)t);
        // footprint: sorted, no duplicates, distinct LDS rows below max_pos
        std::map<int, int32_t> col_of_pos;
        for (int f = 0; f < nf; ++f) {
            if (f) CHECK(P.fp[f0 + f] > P.fp[f0 + f - 1], "tile %lld: footprint not sorted / duplicate at %d", (long long)t, f);
            const int pos = P.fp_pos[f0 + f];
            CHECK(pos < P.max_pos, "tile %lld: LDS row %d >= max_pos %d", (long long)t, pos, P.max_pos);
            CHECK(col_of_pos.emplace(pos, P.fp[f0 + f]).second, "tile %lld: LDS row %d twice", (long long)t, pos);
        }
        // rows: each once; offsets monotone from 0 to the tile's nonzeros; every nonzero back to its column and value
        const int32_t *rp = &P.t_rp[(size_t)tr0 + t];
        CHECK(rp[0] == 0 && rp[nrows] == tnz, "tile %lld: offsets run %d .. %d of %d", (long long)t, rp[0], rp[nrows], tnz);
        for (int i = 0; i < nrows; ++i) {
            const int64_t r = P.t_rows[tr0 + i];
            CHECK(r >= 0 && r < m && !seen[r]++, "tile %lld: row %lld", (long long)t, (long long)r);
            CHECK(rp[i + 1] - rp[i] == A.rowptr[r + 1] - A.rowptr[r], "tile %lld row %lld: %d entries", (long long)t, (long long)r, rp[i + 1] - rp[i]);
            CHECK(z0 + rp[i] < (int64_t)P.t_val.size() && z0 + rp[i] < (int64_t)P.t_lcol.size(), "tile %lld row %lld: entry 0 outside", (long long)t, (long long)r);
            for (int64_t p = A.rowptr[r]; p < A.rowptr[r + 1]; ++p) {
                const int64_t q = z0 + rp[i] + (p - A.rowptr[r]);
                const auto it = col_of_pos.find(P.t_lcol[q]);
                CHECK(it != col_of_pos.end() && it->second == A.col[p] && P.t_val[q] == A.val[p], "tile %lld row %lld entry %lld", (long long)t, (long long)r, (long long)(p - A.rowptr[r]));
            }
        }
        // LDS rows: box tiles inside the halo box (x extent padded to a multiple of 4), ghost columns behind it; tiles of runs, and
        // box tiles with a column outside the box, in footprint order
        bool boxed = P.grid;
        const int W = P.grid ? (P.bx + 2 + 3) / 4 * 4 : 0, H = P.by + 2, D = P.bz + 2;
        int64_t ox = 0, oy = 0, oz = 0;
        if (P.grid) {
            const int64_t r = P.t_rows[tr0];
            ox = (r % P.gx) / P.bx * P.bx, oy = ((r / P.gx) % P.gy) / P.by * P.by, oz = (r / (P.gx * P.gy)) / P.bz * P.bz;
            for (int i = 0; i < nrows; ++i) { // the tile is that box
                const int64_t q = P.t_rows[tr0 + i], x = q % P.gx - ox, y = (q / P.gx) % P.gy - oy, z = q / (P.gx * P.gy) - oz;
                CHECK(x >= 0 && x < P.bx && y >= 0 && y < P.by && z >= 0 && z < P.bz, "tile %lld: row %lld outside its box", (long long)t, (long long)q);
            }
            for (int f = 0; f < nf && boxed; ++f) {
                const int64_t c = P.fp[f0 + f];
                if (c >= m) continue;
                const int64_t fx = c % P.gx - ox + 1, fy = (c / P.gx) % P.gy - oy + 1, fz = c / (P.gx * P.gy) - oz + 1;
                boxed = fx >= 0 && fx < W && fy >= 0 && fy < H && fz >= 0 && fz < D;
            }
            if (!boxed) failing++;
        }
        int ghosts = 0;
        for (int f = 0; f < nf; ++f) {
            const int64_t c = P.fp[f0 + f];
            int want = f;
            if (boxed && c < m)
                want = (int)((c % P.gx - ox + 1) + W * (((c / P.gx) % P.gy - oy + 1) + H * (c / (P.gx * P.gy) - oz + 1)));
            else if (boxed)
                want = W * H * D + ghosts++;
            CHECK(P.fp_pos[f0 + f] == want, "tile %lld footprint %d: LDS row %d, expected %d", (long long)t, f, (int)P.fp_pos[f0 + f], want);
        }
    }
    for (int64_t r = 0; r < m; ++r) CHECK(seen[r] == 1, "row %lld in %d tiles", (long long)r, seen[r]);
    CHECK(failing == E.failing_tiles, "%lld tiles fell back", (long long)failing);
    CHECK(P.max_fp == max_fp && P.max_rows == max_rows, "max_fp %d (%d) max_rows %d (%d)", P.max_fp, max_fp, P.max_rows, max_rows);
    CHECK(P.max_nz % 4 == 0 && P.max_nz >= max_nz && P.max_nz < max_nz + 4, "max_nz %d for %d", P.max_nz, max_nz);
    CHECK(std::fabs(P.reuse - (double)nnz / (double)P.fp_ptr[nt]) < 1e-12, "reuse %g", P.reuse);
    std::printf("PASS %-10s m %lld nnz %lld tiles %lld rows/tile %d max_fp %d max_pos %d max_nz %d reuse %.4f grid %d\n", name, (long long)m, (long long)nnz,
                (long long)nt, P.max_rows, P.max_fp, P.max_pos, P.max_nz, P.reuse, (int)P.grid);
}

} // namespace

int main(int argc, char **argv)
{
    if (argc != 4) {
        std::printf("usage: %s <max_row_nnz> <max_fp> <reuse> of the banded pattern\n", argv[0]);
        return 2;
    }
    rails_tile_plan P;
    const Expect runs = {false, 0, 0, 0, 0, 0, 0, 0};
    {
        const char *name = "banded";
        const Csr A = banded(3000, 12, 40);
        check(name, A, runs, P);
        auto stats = [&]() { CHECK(A.max_row_nnz() == std::atoi(argv[1]) && P.max_fp == std::atoi(argv[2]) && std::fabs(P.reuse - std::atof(argv[3])) < 1e-12 && P.max_pos == P.max_fp && P.n_tiles == 47 && P.max_rows == 64,
                                   "max_row_nnz %d max_fp %d reuse %.15g tiles %lld", A.max_row_nnz(), P.max_fp, P.reuse, (long long)P.n_tiles); };
        if (!failures) stats();
    }
    check("grid7", stencil(23, 11, 9, false), Expect{true, 23, 11, 9, 4, 4, 4, 0}, P);
    check("grid27", stencil(9, 8, 7, true), Expect{true, 9, 8, 7, 4, 4, 4, 0}, P);
    check("grid9_2d", stencil(50, 61, 1, true), Expect{true, 50, 61, 1, 4, 16, 1, 0}, P);
    {
        const char *name = "ragged";
        const Csr A = ragged(2990, 46); // 2990 = 46 x 64 + 46: the last tile has only empty rows
        auto shape = [&]() { CHECK(A.rowptr[2990] == A.rowptr[2944] && A.rowptr[1] == 0 && A.rowptr[38] == A.rowptr[37], "empty rows"); };
        shape();
        check(name, A, runs, P);
        auto tail = [&]() { CHECK(P.n_tiles == 47 && P.t_nzptr[47] == P.t_nzptr[46] && P.fp_ptr[47] == P.fp_ptr[46], "the last tile is not empty"); };
        if (!failures) tail();
    }
    // every other layer of boxes: 4 x 6 x 3 tiles with the far columns
    check("box_fail", box_fail(), Expect{true, 16, 24, 24, 4, 4, 4, 72}, P);
    if (failures) {
        std::printf("%d FAILED\n", failures);
        return 1;
    }
    std::printf("ALL PASSED\n");
    return 0;
}
