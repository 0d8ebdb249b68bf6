// iter_geom.h -- the geometry of a pass of the iterative A^-1 operator (itsolve.hip, iter_kernels.inc): how the 256 threads of a block
// share the columns of a group and how the rows are cut into slabs, one block each.  The one statement of the rule in C++: the group's
// passes and those of every multigrid level take it from here.  No HIP in here: tests/cpp/iter_geom_host.cpp stands alone on it, and
// tests/iter_steps_reference.py restates it in Python.  The geometry of a solve with block Jacobi on (slabs of whole block rows) is the second
// function: tests/cpp/block_jacobi_host.cpp and tests/block_jacobi_reference.py.
#ifndef RAILS_ITER_GEOM_H
#define RAILS_ITER_GEOM_H

#include <algorithm>
#include <cstdint>

struct rails_pass_geom {
    int ncw;     // columns of the group
    int ld;      // row stride of every work panel
    int tx_bits; // TX = 1 << tx_bits threads along the column pairs, TY = 256 / TX along the rows
    int64_t m, rows_per_slab;
};

// the passes' geometry for w <= 32 columns of n rows at row stride ld, and the number of slabs (blocks) in *slabs: a thread owns a pair of
// columns, slabs of at least 8 rows per thread, at most 1024 of them (k_colnorms2's rule), none of them empty
inline rails_pass_geom rails_iter_pass_geom(int64_t n, int w, int ld, int64_t *slabs)
{
    const int pairs = (w + 1) / 2;
    int tx_bits = 0;
    while ((1 << tx_bits) < pairs) ++tx_bits; // <= 4
    const int TY = 256 >> tx_bits;
    const int64_t ns = std::max<int64_t>(1, std::min<int64_t>(1024, n / ((int64_t)TY * 8)));
    const int64_t rps = (n + ns - 1) / ns;
    *slabs = (n + rps - 1) / rps;
    return rails_pass_geom{w, ld, tx_bits, n, rps};
}

// The geometry of a solve with block Jacobi on (iter_kernels.inc: iter_pass_block; tests/block_jacobi_reference.py restates it): n = nb * b
// rows in nb block rows.  Along the rows a thread walks block rows, so the slabs are whole block rows: at least 8 block rows per thread
// where there are that many, at most 1024 slabs, none of them empty.  rows_per_slab is a multiple of b; the point passes of such a solve
// (the inner products, k_cg_dir, k_bi_update) run on the same slabs.
inline rails_pass_geom rails_iter_pass_geom_block(int64_t n, int w, int ld, int b, int64_t *slabs)
{
    const int pairs = (w + 1) / 2;
    int tx_bits = 0;
    while ((1 << tx_bits) < pairs) ++tx_bits; // <= 4
    const int TY = 256 >> tx_bits;
    const int64_t nb = n / b;
    const int64_t ns = std::max<int64_t>(1, std::min<int64_t>(1024, nb / ((int64_t)TY * 8)));
    const int64_t bps = (nb + ns - 1) / ns;
    *slabs = (nb + bps - 1) / bps;
    return rails_pass_geom{w, ld, tx_bits, n, bps * b};
}

#endif
