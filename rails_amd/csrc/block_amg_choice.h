// block_amg_choice.h -- what the block multigrid cycle of the iterative A^-1 operator (itsolve.hip, "block_amg")
// decides about a level without computing: how many rows the cycle's kernels address, and which Chebyshev step a level takes -- the fused
// kernel k_cheb_step_bsr<B, LPR> on k_spmm_bsr's block-row body, or rails_spmm and the pass k_cheb_pass_bj<B> -- with the fused kernel's
// instantiation, grid and LDS.  Plain arithmetic on integers, no HIP, no I/O, no environment: checked on the host alone by
// tests/cpp/block_amg_host.cpp against the restatement in tests/block_amg_reference.py.
#ifndef RAILS_BLOCK_AMG_CHOICE_H
#define RAILS_BLOCK_AMG_CHOICE_H

#include "bsr_choice.h"

// Rows of the finest matrix.  The level matrices are block-CSR handles (rails_csr_create_bsr: mb b below 2^31, 64-bit offsets in
// k_spmm_bsr's body); P and R are rectangular CSR handles and the work panels those of the scalar cycle, whose kernels the scalar
// multigrid holds to fewer than 2^24 rows: the same bound here.
constexpr int64_t RAILS_BAMG_MAX_ROWS = (int64_t)1 << 24;
inline bool rails_bamg_rows_ok(int64_t m, int b) { return b >= 2 && b <= 8 && m >= b && m % b == 0 && m < RAILS_BAMG_MAX_ROWS; }

// Whether k_cheb_step_bsr<b, lpr> and k_amg_residual_bsr<b, lpr> are free of spills and scratch in the gfx950 cross-compile
// (profiles/block_amg_kernel_resources.txt): a fact of the build, not a guess.  An instantiation that is not takes the unfused step.
constexpr bool rails_bamg_fused_compiled(int b, int lpr) { return b >= 2 && b <= 8 && (lpr == 8 || lpr == 16 || lpr == 32); }

struct BamgStep {
    bool ok;        // false: no kernels for these facts
    bool fused;     // the step and the residual run on the fused kernels
    BsrChoice k;    // their launch: k_spmm_bsr's own rule for the level matrix at the group's width
    int lds_bytes;  // of a workgroup of the fused kernels
};

// f: the level matrix (b, mb, max_brow), the group's width nc, the work panels' row stride in ldx and ldy; want_fused: "poly_fused"
inline BamgStep rails_bamg_step(const BsrFacts &f, bool want_fused)
{
    BamgStep s{};
    s.k = rails_bsr_choice(f);
    if (!s.k.ok || f.nc > 32 || f.ldx < f.nc || f.ldx != f.ldy) return s;
    s.ok = true;
    s.fused = want_fused && rails_bamg_fused_compiled(s.k.b, s.k.lpr);
    const int cap = rails_bsr_lds_blocks(f.b);
    s.lds_bytes = cap * f.b * f.b * 8 + cap * 4;
    return s;
}

#endif
