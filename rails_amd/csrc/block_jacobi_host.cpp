// block_jacobi_host.cpp -- see block_jacobi_host.h.  Host code only.
#include "block_jacobi_host.h"

#include <cmath>
#include <cstdio>

int rails_bj_plan(int op, int handle_b, bool reduces, int64_t m, int b, bool blocks_given, int *source, int *b_eff, char *err, size_t cap)
{
    const char *who = "rails_iter_block_jacobi";
    *source = RAILS_BJ_CLEAR;
    *b_eff = 0;
    if (!blocks_given && b == 0 && op != RAILS_BJ_OP_BSR) return 0; // clears the blocks: always allowed
    if (reduces) {
        snprintf(err, cap, "%s: a context that reduces (more than one rank, an all-reduce hook or a communicator): block Jacobi is single GPU", who);
        return 1;
    }
    if (!blocks_given && op == RAILS_BJ_OP_BSR && b == 0) b = handle_b;
    if (b < RAILS_BJ_MIN_B || b > RAILS_BJ_MAX_B) {
        snprintf(err, cap, "%s: block size %d is not in %d .. %d", who, b, RAILS_BJ_MIN_B, RAILS_BJ_MAX_B);
        return 1;
    }
    if (m % b != 0) {
        snprintf(err, cap, "%s: block size %d does not divide the operator's %lld rows", who, b, (long long)m);
        return 1;
    }
    if (op == RAILS_BJ_OP_BSR && b != handle_b) {
        snprintf(err, cap, "%s: block size %d on a block-CSR operator of block size %d", who, b, handle_b);
        return 1;
    }
    if (!blocks_given) {
        switch (op) {
        case RAILS_BJ_OP_BSR: *source = RAILS_BJ_FROM_BSR; break;
        case RAILS_BJ_OP_CSR: *source = RAILS_BJ_FROM_CSR; break;
        case RAILS_BJ_OP_CSR_NO_HOST: snprintf(err, cap, "%s: no blocks given and the operator keeps no CSR arrays on the host to take them from", who); return 1;
        case RAILS_BJ_OP_CALLBACK: snprintf(err, cap, "%s: no blocks given and the operator is a callback: pass the diagonal blocks", who); return 1;
        case RAILS_BJ_OP_LU: snprintf(err, cap, "%s: no blocks given and the operator is an LU handle: pass the diagonal blocks", who); return 1;
        default: snprintf(err, cap, "%s: no blocks given and the operator is an iterative solve: pass the diagonal blocks", who); return 1;
        }
    } else
        *source = RAILS_BJ_FROM_ARGUMENT;
    *b_eff = b;
    return 0;
}

void rails_bj_from_bsr(int64_t mb, int b, const int64_t *browptr, const int32_t *bcol, const double *bval, double *blocks)
{
    const int bb = b * b;
    for (int64_t k = 0; k < mb * bb; ++k) blocks[k] = 0.0;
    for (int64_t I = 0; I < mb; ++I)
        for (int64_t q = browptr[I]; q < browptr[I + 1]; ++q)
            if (bcol[q] == I)
                for (int e = 0; e < bb; ++e) blocks[I * bb + e] += bval[q * bb + e];
}

void rails_bj_from_csr(int64_t mb, int b, const int64_t *rowptr, const int32_t *col, const double *val, double *blocks)
{
    const int bb = b * b;
    for (int64_t k = 0; k < mb * bb; ++k) blocks[k] = 0.0;
    for (int64_t I = 0; I < mb; ++I)
        for (int r = 0; r < b; ++r) {
            const int64_t i = I * b + r;
            for (int64_t q = rowptr[i]; q < rowptr[i + 1]; ++q) {
                const int64_t c = (int64_t)col[q] - I * b;
                if (c >= 0 && c < b) blocks[I * bb + r * b + c] += val[q];
            }
        }
}

int rails_bj_invert(int64_t nblocks, int b, const double *blocks, double *inv, char *err, size_t cap)
{
    long double a[RAILS_BJ_MAX_B][2 * RAILS_BJ_MAX_B];
    for (int64_t k = 0; k < nblocks; ++k) {
        const double *blk = blocks + k * b * b;
        for (int i = 0; i < b; ++i)
            for (int j = 0; j < b; ++j) {
                a[i][j] = blk[i * b + j];
                a[i][b + j] = i == j ? 1.0L : 0.0L;
            }
        for (int p = 0; p < b; ++p) {
            int best = p; // the largest entry of column p at or below the diagonal; a NaN there stays and is refused as the pivot
            for (int i = p + 1; i < b; ++i)
                if (fabsl(a[i][p]) > fabsl(a[best][p]) || std::isnan(a[i][p])) best = i;
            if (best != p)
                for (int j = 0; j < 2 * b; ++j) {
                    const long double t = a[p][j];
                    a[p][j] = a[best][j];
                    a[best][j] = t;
                }
            const long double piv = a[p][p];
            if (!(piv != 0.0L) || !std::isfinite(piv)) {
                snprintf(err, cap, "rails_iter_block_jacobi: diagonal block %lld (rows %lld .. %lld) has the pivot %Lg at elimination step %d: it is singular or not finite",
                         (long long)k, (long long)(k * b), (long long)(k * b + b - 1), piv, p);
                return 1;
            }
            for (int j = 0; j < 2 * b; ++j) a[p][j] /= piv;
            for (int i = 0; i < b; ++i) {
                if (i == p) continue;
                const long double f = a[i][p];
                if (f == 0.0L) continue;
                for (int j = 0; j < 2 * b; ++j) a[i][j] -= f * a[p][j];
            }
        }
        for (int i = 0; i < b; ++i)
            for (int j = 0; j < b; ++j) {
                const double v = (double)a[i][b + j];
                if (!std::isfinite(v)) {
                    snprintf(err, cap, "rails_iter_block_jacobi: the inverse of diagonal block %lld (rows %lld .. %lld) is not finite", (long long)k, (long long)(k * b),
                             (long long)(k * b + b - 1));
                    return 1;
                }
                inv[k * b * b + i * b + j] = v;
            }
    }
    return 0;
}
