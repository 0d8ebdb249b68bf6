// op_choice.h -- which whole-operator kernel takes a product of rails_spmm, from plain facts: no HIP in here (the sibling of row_choice.h,
// which decides among the row kernels once none of these has taken the product).
//
// rails_spmm, rails_csr_prepare and the interior sweep of spmm_sweep.hip all ask this header, so a schedule is built ahead exactly where
// a product would use it.  First row that applies, in this order ("Which kernel takes a product"):
//
//   serial product (rails_op_order)
//     SWEEP   forced     variant 7
//             automatic  variant 0, no ghost rows, rails_sweep_shape_worthwhile(m, window_rows, nc), not a grid stencil
//     PLANES  forced     variant 9
//             automatic  variant 0, nc >= 2, no ghost rows, not rectangular, RAILS_SPMM_PLANES, a grid stencil
//     TILED   forced     variants 2 and 6
//             automatic  variant 0, unless the lean row kernel is to have the product (RAILS_SPMM_NARROW_CC and _FAST, 8 < nc <= 16,
//                        longest row <= 64 entries, fewer than 2^24 columns)
//     then the row kernels (row_choice.h).  A forced kernel that does not take the product is an error, an automatic one declines.
//
//   row-partitioned product (rails_halo_order)
//     overlapped         RAILS_SPMM_HALO_OVERLAP, ghost rows, not rectangular, variant 0 / 1 / 3, interior rows >= max(m / 2, 1024)
//     interior PLANES    overlapped, variant 0, RAILS_SPMM_PLANES (the kernel's plan says whether the block is a slab of a grid stencil)
//     interior SWEEP     overlapped, variant 0, rails_sweep_interior_shape_ok
//     then the row kernels for the interior rows; the boundary rows are theirs always.  Not overlapped: the serial order above.
//
//   ahead of the products (rails_prepare_choice): the sweep schedule where SWEEP leads the serial order; the interior one where the
//   product overlaps and its interior rows would try the sweep, unless the block is a grid stencil (the planes take those).
#ifndef RAILS_OP_CHOICE_H
#define RAILS_OP_CHOICE_H

#include <cstdint>

// The sweep kernel's geometry (spmm_sweep.hip instantiates it, sweep_plan.h explains it): a workgroup owns one block of
// groups x waves x 16 slots rows at a time, one row per slot.
constexpr int RAILS_SWEEP_WAVES = 8, RAILS_SWEEP_GROUPS = 22, RAILS_SWEEP_SLOTS = 16;
constexpr int64_t RAILS_SWEEP_BLOCK_ROWS = (int64_t)RAILS_SWEEP_GROUPS * RAILS_SWEEP_WAVES * RAILS_SWEEP_SLOTS;
static_assert(RAILS_SWEEP_BLOCK_ROWS == 2816, "the sweep kernel's row block");

struct OpFacts {
    // the operator
    int variant = 0, max_row_nnz = 0;
    int64_t m = 0, ncols_ext = 0, n_ghost = 0;
    bool rect = false;
    int64_t window_rows = 0;                             // mean window of X rows a row gathers from
    int64_t window_rows_int = 0, int_lo = 0, int_hi = 0; // row-partitioned: the interior rows [int_lo, int_hi) and their window
    // the product: nc columns; X rows 16-byte aligned with an even width (x_vec2), Y rows 16-byte aligned (y_vec2)
    int nc = 0;
    bool x_vec2 = false, y_vec2 = false;
    // the device
    int num_cu = 0;
    // RAILS_SPMM_PLANES, RAILS_SPMM_NARROW_CC, RAILS_SPMM_NARROW_FAST, RAILS_SPMM_HALO_OVERLAP
    bool planes = true, narrow_cc = true, narrow_fast = true, halo_overlap = true;
};

// The sweep kernel as an automatic choice for `rows` rows whose rows gather from a window of `window_rows` X rows, from what is known
// without building its schedule: 64 to 256 columns in chunks of 16 that divide the 32 workgroups of an XCD; the window fits
// (phases - 1) row blocks (the planner decides exactly); every XCD's part holds a few blocks per phase; an X row is staged by at most 8
// workgroups per row of the part (phases x (1 + window / rows of a part): the launcher's own bound).
inline bool rails_sweep_shape_worthwhile(int64_t rows, int64_t window_rows, int nc)
{
    if (!(nc >= 64 && nc <= 256 && nc % 16 == 0 && 32 % (nc / 16) == 0 && window_rows > 0)) return false;
    const int64_t phases = 32 / (nc / 16), part_rows = rows / 8;
    return window_rows + 256 <= (phases - 1) * RAILS_SWEEP_BLOCK_ROWS && rows >= 8 * phases * RAILS_SWEEP_BLOCK_ROWS &&
           (double)phases * (double)(part_rows + window_rows + 1024) <= 8.0 * (double)part_rows;
}

// A built schedule is worth launching only where the lock-step trips are reasonably full (the units run early to level the waves count
// as trips: 0.52 on the banded-random pattern) and a row block re-uses what it stages.
inline bool rails_sweep_plan_fits(bool ok, double efficiency, double staged_rows_per_row)
{
    return ok && efficiency >= 0.4 && staged_rows_per_row <= 8.0;
}

// The interior rows of a row-partitioned operator (no ghost columns: a rectangular operator over the local X rows) as a sweep of their own.
inline bool rails_sweep_interior_shape_ok(const OpFacts &f)
{
    return f.x_vec2 && f.y_vec2 && f.num_cu >= 256 && f.n_ghost > 0 && !f.rect && f.m < 0x7fffffffLL &&
           rails_sweep_shape_worthwhile(f.int_hi - f.int_lo, f.window_rows_int, f.nc);
}

struct OpStep {
    enum Kernel { SWEEP, PLANES, TILED } kernel;
    bool forced; // the variant asks for this kernel: fail instead of declining
};
struct OpOrder {
    OpStep step[3];
    int n = 0;
    void add(OpStep::Kernel k, bool forced) { step[n++] = {k, forced}; }
    bool has(OpStep::Kernel k) const
    {
        for (int i = 0; i < n; ++i)
            if (step[i].kernel == k) return true;
        return false;
    }
};

// The whole-operator kernels a serial product tries, in order, before the row kernels.  is_grid() -- is the pattern a structured-grid
// stencil? -- is a scan of the matrix: asked at most once, and only after the cheap conditions have passed.  Few nonzeros per row leave
// the sweep at its floor of one LDS-DMA latency per step, so grid stencils go to the plane-sweep and LDS-staged box kernels (7-point
// Laplacian 50 x 50 x 400 at 128 columns: 0.65 ms against 0.82).  At Expand size <= 16 the lean row kernel beats the box kernel on the
// stencils too (27-point: 0.206 against 0.256 ms, 7-point: 0.097 against 0.130): in automatic mode the box kernel is for wider panels.
template <class IsGrid>
bool rails_sweep_leads(const OpFacts &f, IsGrid &&is_grid) // the sweep is the first kernel a serial product tries
{
    return f.variant == 7 || (f.variant == 0 && f.n_ghost == 0 && rails_sweep_shape_worthwhile(f.m, f.window_rows, f.nc) && !is_grid());
}

template <class IsGrid>
OpOrder rails_op_order(const OpFacts &f, IsGrid &&is_grid)
{
    int grid_known = -1;
    auto grid = [&]() {
        if (grid_known < 0) grid_known = is_grid() ? 1 : 0;
        return grid_known == 1;
    };
    OpOrder o;
    const bool automatic = f.variant == 0;
    if (rails_sweep_leads(f, grid)) o.add(OpStep::SWEEP, !automatic);
    if (f.variant == 9 || (automatic && f.nc >= 2 && f.n_ghost == 0 && !f.rect && f.planes && grid())) o.add(OpStep::PLANES, f.variant == 9);
    const bool leave_to_narrow = f.narrow_cc && f.narrow_fast && f.nc > 8 && f.nc <= 16 && f.max_row_nnz <= 64 && f.ncols_ext < (1 << 24);
    if (f.variant == 2 || f.variant == 6 || (automatic && !leave_to_narrow)) o.add(OpStep::TILED, !automatic);
    return o;
}

// A row-partitioned product: whether the interior rows' product runs beside the halo exchange, and what those rows try before the row
// kernels.  (No grid scan here: the plane kernel's own plan, one pass on the device, says whether the block is a slab of a stencil.)
struct HaloOrder {
    bool overlap = false;
    OpOrder interior;
};
inline HaloOrder rails_halo_order(const OpFacts &f)
{
    HaloOrder h;
    const int64_t interior_rows = f.int_hi - f.int_lo;
    h.overlap = f.halo_overlap && f.n_ghost > 0 && !f.rect && (f.variant == 0 || f.variant == 1 || f.variant == 3) && interior_rows >= f.m / 2 &&
                interior_rows >= 1024;
    if (h.overlap && f.variant == 0) {
        if (f.planes) h.interior.add(OpStep::PLANES, false);
        if (rails_sweep_interior_shape_ok(f)) h.interior.add(OpStep::SWEEP, false);
    }
    return h;
}

// What rails_csr_prepare builds ahead of the products of f.nc columns (facts with aligned windows): what their own order would take.
enum class PrepareChoice { NONE, SWEEP, SWEEP_INTERIOR };
template <class IsGrid>
PrepareChoice rails_prepare_choice(const OpFacts &f, IsGrid &&is_grid)
{
    if (rails_sweep_leads(f, is_grid)) return PrepareChoice::SWEEP;
    if (rails_halo_order(f).interior.has(OpStep::SWEEP) && !is_grid()) return PrepareChoice::SWEEP_INTERIOR;
    return PrepareChoice::NONE;
}

#endif
