// row_choice.h -- which row kernel of spmm.hip computes a product (or a span of its rows), from plain facts: no HIP in here.
//
// The serial tail of rails_spmm and the spans of the halo-overlapped product (spmm_span) both launch what rails_row_choice says, so a
// row's product is bitwise the same whichever launch it belongs to.  The rule as a table: DESIGN.md, "Which row kernel runs".
#ifndef RAILS_ROW_CHOICE_H
#define RAILS_ROW_CHOICE_H

#include <cstdint>

struct RowFacts {
    // the operator
    int variant = 0, max_row_nnz = 0;
    int64_t m = 0, ncols_ext = 0, n_ghost = 0;
    bool rect = false;
    // the product: nc columns; X rows 16-byte aligned (x_vec2), Y rows likewise (y_vec2), both windows on even columns and ghost rows
    // aligned (vec2); leading dimensions of X and of the ghost rows; the ghost rows are the rows of X behind the operator's own m
    int nc = 0;
    bool x_vec2 = false, y_vec2 = false, vec2 = false;
    int ldx = 0, ldg = 0;
    bool xg_is_tail = false;
    // the caller: -1 = the serial path (the operator's own ghost form); 0 / 1 = a span whose rows have no / may have ghost columns
    int span_ghost = -1;
    // RAILS_SPMM_NARROW_CC, RAILS_SPMM_NARROW_FAST, RAILS_SPMM_CHUNK
    bool narrow_cc = true, narrow_fast = true;
    int chunk_env = 0;
};

struct RowChoice {
    enum Kind { PLAIN, CC, NARROW } kind; // k_spmm_rowgather, k_spmm_rowgather_cc, k_spmm_narrow
    int lpr;                              // lanes per row
    bool ghost;                           // NARROW: the form that takes columns >= m from the ghost buffer
    int vec;                              // PLAIN: columns per lane
    bool y_vec;                           // CC, NARROW: 16-byte stores
};

inline RowChoice rails_row_choice(const RowFacts &f)
{
    const bool serial = f.span_ghost < 0;
    int lpr = 0; // of the chunked (1b) or lean (1c) kernel; 0 = neither
    bool y_vec = f.y_vec2, narrow_only = false;
    // column chunks of 32 / 64 for panels wider than that: variants 4 / 5 or RAILS_SPMM_CHUNK, serial path, aligned windows only
    if (serial && f.vec2) {
        int chunk = 0;
        if (f.variant == 4 || f.variant == 5)
            chunk = 32 * (f.variant - 3);
        else if (f.variant != 3 && (f.chunk_env == 32 || f.chunk_env == 64))
            chunk = f.chunk_env;
        if (chunk && f.nc > chunk) lpr = chunk / 2, y_vec = true;
    }
    // narrow panels (the in-loop A*W at Expand size <= 32): one chunk of 16 or 32 columns.  X rows that are only 8-byte aligned (a
    // window on an odd column): the lean kernel takes them up to 16 columns, the chunked one does not -- serial path only
    const bool narrow_width = f.narrow_cc && f.variant != 3 && f.nc > 8 && f.max_row_nnz <= 64;
    if (!lpr && narrow_width && f.x_vec2 && f.nc <= 32)
        lpr = f.nc <= 16 ? 8 : 16;
    else if (!lpr && narrow_width && serial && !f.x_vec2 && f.nc <= 16)
        lpr = 8, narrow_only = true;
    if (lpr) {
        if (lpr <= 16 && f.nc <= 2 * lpr && f.narrow_fast) {
            // the lean kernel: every X row within 32-bit byte offsets of its base -- all of them at X + c * ldx (no ghost rows; a
            // rectangular operator's extra rows follow X in the same panel), or local and ghost rows behind two bases
            const bool flat = f.span_ghost == 0 || (serial && ((f.n_ghost == 0 && !f.rect) || (f.xg_is_tail && f.ldg == f.ldx)));
            const bool small = f.ncols_ext < (1 << 24) && (int64_t)f.ldx * 8 < (1 << 24) && (int64_t)f.ldg * 8 < (1 << 24);
            if (small && flat && (uint64_t)f.ncols_ext * (uint64_t)f.ldx * 8u < 0xffffff00ull) return {RowChoice::NARROW, lpr, false, 2, y_vec};
            if (small && !flat && !f.rect && (uint64_t)f.m * (uint64_t)f.ldx * 8u < 0xffffff00ull &&
                (uint64_t)(f.ncols_ext - f.m) * (uint64_t)f.ldg * 8u < 0xffffff00ull)
                return {RowChoice::NARROW, lpr, true, 2, y_vec};
        }
        if (!narrow_only) return {RowChoice::CC, lpr, false, 2, y_vec};
    }
    // the plain kernel: two columns per lane whatever the alignment of the windows (Acc<2>), as many lanes per row as the width asks for
    const int vec = ((serial && f.vec2) || f.nc >= 2) ? 2 : 1;
    const int need = (f.nc + vec - 1) / vec;
    const int plain_lpr = need >= 64 ? 64 : need > 16 ? 32 : need > 8 ? 16 : need > 4 ? 8 : need > 2 ? 4 : need > 1 ? 2 : 1;
    return {RowChoice::PLAIN, plain_lpr, false, vec, false};
}

#endif
