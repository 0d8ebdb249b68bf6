// tile_plan.cpp -- builds the tile plan of the LDS-staged footprint SpMM on the host (see tile_plan.h).
#include "tile_plan.h"

#include <algorithm>
#include <cstdlib>
#include <utility>

bool rails_detect_grid(int64_t m, const int64_t *rowptr, const int32_t *col, int64_t *nx, int64_t *ny, int64_t *nz)
{
    if (m < 64) return false;
    std::vector<int64_t> offs;
    int64_t step = std::max<int64_t>(1, m / 4096);
    for (int64_t r = 0; r < m; r += step)
        for (int64_t p = rowptr[r]; p < rowptr[r + 1]; ++p) {
            int64_t c = col[p];
            if (c < m && c > r) offs.push_back(c - r);
        }
    std::sort(offs.begin(), offs.end());
    offs.erase(std::unique(offs.begin(), offs.end()), offs.end());
    if (offs.empty() || offs.size() > 13 || offs[0] != 1) return false;
    auto has = [&](int64_t v) { return std::binary_search(offs.begin(), offs.end(), v); };
    if (offs.size() < 2) return false;
    int64_t a = offs[1]; // smallest offset > 1: nx (5/7-point) or nx-1 (9/27-point)
    int64_t gx = (has(a + 1) && has(a + 2)) ? a + 1 : a;
    if (gx < 3 || m % gx != 0) return false;
    // offsets beyond the in-plane cluster {1, nx-1, nx, nx+1} form a symmetric cluster around nx*ny
    int64_t gxy = 0, lo = 0, hi = 0;
    for (int64_t v : offs)
        if (v > gx + 1) {
            if (!lo) lo = v;
            hi = v;
        }
    if (lo) gxy = (lo + hi) / 2;
    if (gxy && (gxy % gx != 0 || !has(gxy))) return false;
    if (gxy == 0) gxy = m; // 2D grid
    if (m % gxy != 0) return false;
    // validate on the sample
    for (int64_t r = 0; r < m; r += step)
        for (int64_t p = rowptr[r]; p < rowptr[r + 1]; ++p) {
            int64_t c = col[p];
            if (c >= m) continue;
            int64_t x = r % gx, y = (r % gxy) / gx, z = r / gxy;
            int64_t cx = c % gx, cy = (c % gxy) / gx, cz = c / gxy;
            if (std::llabs(cx - x) > 1 || std::llabs(cy - y) > 1 || std::llabs(cz - z) > 1) return false;
        }
    *nx = gx;
    *ny = gxy / gx;
    *nz = m / gxy;
    return true;
}

namespace {

// boxes of about tile_rows grid points (x longest: contiguous in memory, then y, then z), numbered along a Morton (Z-order) curve over
// their (x, y, z) box coordinates: tiles that share halo rows are processed close together in time (and, with the XCD-aware block
// map, on the same XCD), so the halo re-reads are served by L2 / Infinity Cache instead of HBM
void assign_boxes(const rails_tile_params &prm, int64_t m, rails_tile_plan &P, std::vector<int32_t> &tile_of_row)
{
    int bx = 8, by = 4, bz = 4;
    if (prm.tile_rows <= 64) { bx = 4; by = 4; bz = 4; }
    if (prm.tile_rows >= 256) { bx = 8; by = 8; bz = 4; }
    if (P.gz == 1) { bz = 1; by = std::max(1, prm.tile_rows / bx); }
    const int64_t gx = P.gx, gy = P.gy, gz = P.gz;
    const int64_t tx = (gx + bx - 1) / bx, ty = (gy + by - 1) / by, tz = (gz + bz - 1) / bz;
    P.n_tiles = tx * ty * tz;
    P.bx = bx, P.by = by, P.bz = bz;
    std::vector<int32_t> rank(P.n_tiles);
    std::vector<std::pair<uint64_t, int32_t>> keys(P.n_tiles);
    auto spread = [](uint64_t v) { // 21 bits -> every third bit
        v &= 0x1fffff;
        v = (v | v << 32) & 0x1f00000000ffffull;
        v = (v | v << 16) & 0x1f0000ff0000ffull;
        v = (v | v << 8) & 0x100f00f00f00f00full;
        v = (v | v << 4) & 0x10c30c30c30c30c3ull;
        v = (v | v << 2) & 0x1249249249249249ull;
        return v;
    };
    for (int64_t z = 0; z < tz; ++z)
        for (int64_t y = 0; y < ty; ++y)
            for (int64_t x = 0; x < tx; ++x) {
                int64_t id = z * ty * tx + y * tx + x;
                uint64_t key = prm.morton ? (spread(x) | spread(y) << 1 | spread(z) << 2) : (uint64_t)id;
                keys[id] = std::make_pair(key, (int32_t)id);
            }
    std::sort(keys.begin(), keys.end());
    for (int64_t i = 0; i < P.n_tiles; ++i) rank[keys[i].second] = (int32_t)i;
    for (int64_t r = 0; r < m; ++r) {
        int64_t x = r % gx, y = (r / gx) % gy, z = r / (gx * gy);
        tile_of_row[r] = rank[(z / bz) * ty * tx + (y / by) * tx + (x / bx)];
    }
}

// runs of consecutive rows; false when a sample of tiles says that a staged row is used less than about twice (cheap, before the
// full analysis)
bool assign_runs(const rails_tile_params &prm, int64_t m, const int64_t *rowptr, const int32_t *col, rails_tile_plan &P,
                 std::vector<int32_t> &tile_of_row)
{
    const int rows = std::min(prm.tile_rows, 256);
    P.n_tiles = (m + rows - 1) / rows;
    std::vector<int32_t> tmp;
    double snz = 0, sfp = 0;
    const int64_t step = std::max<int64_t>(1, P.n_tiles / 64);
    for (int64_t tt = 0; tt < P.n_tiles; tt += step) {
        int64_t r0 = tt * rows, r1 = std::min<int64_t>(m, r0 + rows);
        tmp.assign(col + rowptr[r0], col + rowptr[r1]);
        snz += (double)tmp.size();
        std::sort(tmp.begin(), tmp.end());
        tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
        sfp += (double)tmp.size();
    }
    if (sfp <= 0 || snz / sfp < RAILS_TILE_MIN_REUSE) return false;
    for (int64_t r = 0; r < m; ++r) tile_of_row[r] = (int32_t)(r / rows);
    return true;
}

// tile_of_row -> the arrays of the plan; returns false when a tile exceeds the caps
bool make_plan(int64_t m, const int64_t *rowptr, const int32_t *col, const double *val, const std::vector<int32_t> &tile_of_row, int fp_cap,
               int nz_cap, rails_tile_plan &P)
{
    const int64_t ntiles = P.n_tiles, nnz = rowptr[m];
    P.t_rowptr.assign(ntiles + 1, 0);
    for (int64_t r = 0; r < m; ++r) P.t_rowptr[tile_of_row[r] + 1]++;
    for (int64_t t = 0; t < ntiles; ++t) P.t_rowptr[t + 1] += P.t_rowptr[t];
    P.t_rows.resize(m);
    {
        std::vector<int32_t> next(P.t_rowptr.begin(), P.t_rowptr.end() - 1);
        for (int64_t r = 0; r < m; ++r) P.t_rows[next[tile_of_row[r]]++] = (int32_t)r;
    }
    P.t_nzptr.assign(ntiles + 1, 0);
    P.fp_ptr.assign(ntiles + 1, 0);
    P.t_rp.resize((size_t)m + ntiles);
    P.t_val.resize((size_t)nnz);
    P.t_lcol.resize((size_t)nnz);
    P.fp.reserve((size_t)nnz / 4 + 16);
    std::vector<int32_t> tmp;
    int64_t z = 0;
    int max_nz = 0;
    for (int64_t t = 0; t < ntiles; ++t) {
        int r0 = P.t_rowptr[t], r1 = P.t_rowptr[t + 1];
        if (r1 - r0 > 256) return false;
        tmp.clear();
        for (int i = r0; i < r1; ++i) {
            int64_t r = P.t_rows[i];
            tmp.insert(tmp.end(), col + rowptr[r], col + rowptr[r + 1]);
        }
        int nzt = (int)tmp.size();
        std::sort(tmp.begin(), tmp.end());
        tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
        if ((int)tmp.size() > fp_cap || nzt > nz_cap) return false;
        // LDS row of every footprint entry.  Box tiles: position inside the halo box with the x extent padded to a
        // multiple of 4 rows, so the four row slots a ds_read_b128 lane group serves (x-consecutive rows) hit four
        // different bank quarters; ghost columns and non-grid tiles: consecutive positions.
        std::vector<uint16_t> pos(tmp.size());
        int npos = (int)tmp.size();
        if (P.grid && r1 > r0) {
            const int64_t rr = P.t_rows[r0];
            const int64_t ox = (rr % P.gx) / P.bx * P.bx, oy = ((rr / P.gx) % P.gy) / P.by * P.by, oz = (rr / (P.gx * P.gy)) / P.bz * P.bz;
            const int W = (P.bx + 2 + 3) / 4 * 4, H = P.by + 2;
            const int box = W * H * (P.bz + 2);
            int extra = 0;
            bool ok = true;
            for (size_t f = 0; f < tmp.size(); ++f) {
                int64_t c = tmp[f];
                if (c < m) {
                    int64_t fx = c % P.gx - ox + 1, fy = (c / P.gx) % P.gy - oy + 1, fz = c / (P.gx * P.gy) - oz + 1;
                    if (fx < 0 || fx >= W || fy < 0 || fy >= H || fz < 0 || fz >= P.bz + 2) {
                        ok = false;
                        break;
                    }
                    pos[f] = (uint16_t)(fx + W * (fy + H * fz));
                } else
                    pos[f] = (uint16_t)(box + extra++);
            }
            if (ok)
                npos = box + extra;
            else
                for (size_t f = 0; f < tmp.size(); ++f) pos[f] = (uint16_t)f;
        } else
            for (size_t f = 0; f < tmp.size(); ++f) pos[f] = (uint16_t)f;
        if (npos > 65535) return false;
        int loc = 0;
        for (int i = r0; i < r1; ++i) {
            int64_t r = P.t_rows[i];
            P.t_rp[(size_t)r0 + t + (i - r0)] = loc;
            for (int64_t p = rowptr[r]; p < rowptr[r + 1]; ++p) {
                P.t_val[z + loc] = val[p];
                P.t_lcol[z + loc] = pos[std::lower_bound(tmp.begin(), tmp.end(), col[p]) - tmp.begin()];
                loc++;
            }
        }
        P.t_rp[(size_t)r0 + t + (r1 - r0)] = loc;
        z += nzt;
        P.t_nzptr[t + 1] = z;
        P.fp.insert(P.fp.end(), tmp.begin(), tmp.end());
        P.fp_pos.insert(P.fp_pos.end(), pos.begin(), pos.end());
        P.max_pos = std::max(P.max_pos, npos);
        P.fp_ptr[t + 1] = (int32_t)P.fp.size();
        P.max_fp = std::max(P.max_fp, (int)tmp.size());
        max_nz = std::max(max_nz, nzt);
        P.max_rows = std::max(P.max_rows, r1 - r0);
    }
    P.max_nz = (max_nz + 3) / 4 * 4;
    P.reuse = P.fp.empty() ? 0.0 : (double)nnz / (double)P.fp.size();
    P.t_val.push_back(0.0); // (the padding: see tile_plan.h)
    P.t_lcol.push_back(0);
    P.fp.push_back(0);
    P.fp_pos.push_back(0);
    return true;
}

} // namespace

bool rails_tile_plan_build(const rails_tile_params &prm, int64_t m, const int64_t *rowptr, const int32_t *col, const double *val,
                           int max_row_nnz, rails_tile_plan &P)
{
    P = rails_tile_plan();
    std::vector<int32_t> tile_of_row(m);
    P.grid = prm.box && rails_detect_grid(m, rowptr, col, &P.gx, &P.gy, &P.gz);
    if (P.grid)
        assign_boxes(prm, m, P, tile_of_row);
    else if (!assign_runs(prm, m, rowptr, col, P, tile_of_row)) {
        P.why = "a sample of tiles has too few nonzeros per staged row";
        return false;
    }
    // caps: 256 rows of max_row_nnz entries, 16-bit LDS rows
    if (!make_plan(m, rowptr, col, val, tile_of_row, 65535, 256 * std::max(1, max_row_nnz), P)) {
        P.why = "a tile has more than 256 rows, 65535 LDS rows or 256 rows' worth of nonzeros";
        return false;
    }
    if (P.reuse < RAILS_TILE_MIN_REUSE) {
        P.why = "too few nonzeros per staged row";
        return false;
    }
    if (rails_tile_lds_bytes(P.max_nz, P.max_pos, prm.kc, 1) > (size_t)RAILS_TILE_LDS_BUDGET) {
        P.why = "the largest tile does not fit the LDS budget";
        return false;
    }
    return true;
}
