// tile_plan.h -- host-side plan of the LDS-staged footprint SpMM, spmm_tiled.hip.
//
// Rows are grouped into tiles; the set of X rows a tile touches (its column footprint, sorted) is computed once per operator, every
// nonzero gets a 16-bit LDS row for its X row, and the tile's (val, LDS row) pairs are stored tile-major.  No HIP in tile_plan.cpp: it
// is built and checked on its own (tests/cpp/tile_plan_host.cpp); the device code only uploads the arrays.  Tiles: bx x by x bz boxes
// of grid points if the matrix is a structured-grid stencil in natural ordering (5/7/9/27-point; footprint (bx+2)(by+2)(bz+2), 9.6
// uses per staged row for an 8x4x4 box of a 27-point stencil), else runs of consecutive rows (~2.8 uses per staged row for a banded
// 27-entry pattern), accepted only when a staged row is used about twice or more.
#ifndef RAILS_TILE_PLAN_H
#define RAILS_TILE_PLAN_H

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

constexpr int RAILS_TILE_LDS_BUDGET = 150 * 1024; // bytes of LDS a workgroup of the tiled kernels may ask for
constexpr double RAILS_TILE_MIN_REUSE = 1.8;      // nonzeros per staged X row below which staging does not pay

struct rails_tile_params {
    int tile_rows = 64; // rows per tile (runs of consecutive rows: at most 256), grid points per box: 4x4x4 up to 64, 8x4x4, 8x8x4 from 256
    bool box = true;    // look for a structured grid and cut it into boxes
    bool morton = true; // number the boxes along a Z-order curve (else x fastest)
    int kc = 8;         // columns per staged chunk: decides whether the largest tile fits the LDS budget
};

struct rails_tile_plan {
    int64_t n_tiles = 0;
    std::vector<int32_t> t_rowptr; // [n_tiles + 1] offsets into t_rows
    std::vector<int32_t> t_rows;   // [m] rows of every tile
    std::vector<int32_t> t_rp;     // [m + n_tiles] per-tile local nonzero offsets (rows + 1 per tile; tile t's start at t_rowptr[t] + t)
    std::vector<int64_t> t_nzptr;  // [n_tiles + 1] offsets into t_val / t_lcol
    std::vector<double> t_val;     // [nnz + 1] values, tile-major
    std::vector<uint16_t> t_lcol;  // [nnz + 1] LDS row of every nonzero's X row
    std::vector<int32_t> fp_ptr;   // [n_tiles + 1] offsets into fp / fp_pos
    std::vector<int32_t> fp;       // footprints: sorted columns per tile
    std::vector<uint16_t> fp_pos;  // LDS row of every footprint entry
    // t_val, t_lcol, fp and fp_pos end with one element of padding: the register-resident kernel loads entry 0 of a row and footprint
    // row 0 of a tile unconditionally, and for an empty last row (a last tile of empty rows) those are one past the end
    int max_fp = 0, max_pos = 0, max_rows = 0;
    int max_nz = 0; // nonzeros of the largest tile, rounded up to a multiple of 4 (the LDS carve-up's alignment)
    double reuse = 0.0; // nonzeros per footprint entry
    // the grid, when tiles are boxes
    bool grid = false;
    int64_t gx = 0, gy = 0, gz = 0;
    int bx = 0, by = 0, bz = 0;
    std::string why; // reason when the build returns false
};

// LDS bytes of k_spmm_tiled (x_buffers = 1) and k_spmm_tiled_pipe (2): vals[max_nz] | x_buffers x Xs[max_pos x kc] | rp[264] (int32) |
// lcols[max_nz] (uint16)
inline size_t rails_tile_lds_bytes(int max_nz, int max_pos, int kc, int x_buffers)
{
    return (size_t)max_nz * 8 + (size_t)x_buffers * (size_t)max_pos * kc * 8 + 264 * 4 + (size_t)max_nz * 2 + 64;
}

// Structured-grid detection from the column offsets of local columns (< m): returns true and (nx, ny, nz) when every
// sampled offset decomposes as dx + nx*dy + nx*ny*dz with |dx|,|dy|,|dz| <= 1.
bool rails_detect_grid(int64_t m, const int64_t *rowptr, const int32_t *col, int64_t *nx, int64_t *ny, int64_t *nz);

// Builds the plan of an operator with m rows (columns >= m are ghost rows).  Returns false (plan.why says why) when staging is not
// worthwhile (fewer than RAILS_TILE_MIN_REUSE nonzeros per staged row) or a tile does not fit (rows, LDS rows, LDS bytes).
bool rails_tile_plan_build(const rails_tile_params &prm, int64_t m, const int64_t *rowptr, const int32_t *col, const double *val,
                           int max_row_nnz, rails_tile_plan &plan);

#endif
