// dense_gram_cols.inc -- the body of the wide-X Gram kernels k_gram_cols and k_gram_cols2 (dense_gram.hip), included once in each.  The kernel
// supplies its parameters (a, Y, ldy, b, m, rows_per_slab, partial) and the left operand Xo, a OneSeg or a TwoSeg.
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int li = lane & 15, kk = lane >> 4;
    const int xcol0 = ((int)blockIdx.y * 4 + wave) * TI * 16;
    if (xcol0 >= a) return; // wave-uniform; no barrier below
    const int64_t r_begin = (int64_t)blockIdx.x * rows_per_slab;
    int64_t r_end = r_begin + rows_per_slab;
    if (r_end > m) r_end = m;

    v4f64 acc[TI][TJ];
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j) acc[i][j] = (v4f64){0.0, 0.0, 0.0, 0.0};
    double acce[TI][NE > 0 ? NE : 1];
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int q = 0; q < (NE > 0 ? NE : 1); ++q) acce[i][q] = 0.0;
    // Loads without branches and without selects on X: with `cond ? load : 0` every load sat in an exec-masked block of its own and the
    // compiler waited for everything in flight (`s_waitcnt vmcnt(0)`: the next step's operands too) before the first MFMA of a step.
    // Columns outside the operands are clamped to column 0 (their results are never written), rows past the slab to its last row
    // with the Y operand zeroed: what comes back from there is multiplied by zero.
    decltype(Xo.col(0)) xcol[TI];
    int yoff[TJ], eoff[NE > 0 ? NE : 1];
#pragma unroll
    for (int i = 0; i < TI; ++i) xcol[i] = Xo.col((xcol0 + 16 * i + li) < a ? xcol0 + 16 * i + li : 0);
#pragma unroll
    for (int j = 0; j < TJ; ++j) yoff[j] = (16 * j + li) < b ? 16 * j + li : 0;
#pragma unroll
    for (int q = 0; q < NE; ++q) eoff[q] = 16 * TJ + q < b ? 16 * TJ + q : 0;

    auto fetch = [&](int64_t r, double *xa, double *yb, double *ye) {
        const int64_t row = r + kk;
        const bool rok = row < r_end;
        const int64_t rc = rok ? row : (r_end > 0 ? r_end - 1 : 0);
        const auto xr = Xo.row(rc);
        const double *yr = Y + rc * ldy;
#pragma unroll
        for (int i = 0; i < TI; ++i) xa[i] = *Xo.at(xr, xcol[i]);
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
            const double t = yr[yoff[j]];
            yb[j] = rok ? t : 0.0;
        }
#pragma unroll
        for (int q = 0; q < NE; ++q) {
            const double t = yr[eoff[q]]; // (one address per row: a broadcast; a column past b is clamped and its result dropped)
            ye[q] = rok ? t : 0.0;
        }
    };
    auto work = [&](const double *xa, const double *yb, const double *ye) {
#pragma unroll
        for (int i = 0; i < TI; ++i) {
#pragma unroll
            for (int j = 0; j < TJ; ++j) acc[i][j] = mfma_f64(xa[i], yb[j], acc[i][j]);
#pragma unroll
            for (int q = 0; q < NE; ++q) acce[i][q] += xa[i] * ye[q];
        }
    };
    double xa[TI], ya[TJ], xb[TI], yb[TJ], ea[NE > 0 ? NE : 1], eb[NE > 0 ? NE : 1];
    fetch(r_begin, xa, ya, ea);
    fetch(r_begin + 4, xb, yb, eb);
    for (int64_t r = r_begin; r < r_end; r += 8) {
        work(xa, ya, ea);
        fetch(r + 8, xa, ya, ea); // rows past the slab come back as zeros
        work(xb, yb, eb);
        fetch(r + 12, xb, yb, eb);
    }
    double *P = partial + (int64_t)blockIdx.x * a * b;
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                int ci = xcol0 + 16 * i + kk + 4 * v; // D row  -> X column
                int cj = 16 * j + li;                 // D col  -> Y column
                if (ci < a && cj < b) P[ci + (int64_t)cj * a] = acc[i][j][v];
            }
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int q = 0; q < NE; ++q) {
            const double t0 = acce[i][q];
            const double t1 = __shfl(t0, li + 16, 64), t2 = __shfl(t0, li + 32, 64), t3 = __shfl(t0, li + 48, 64);
            const int ci = xcol0 + 16 * i + li;
            if (kk == 0 && ci < a && 16 * TJ + q < b) P[ci + (int64_t)(16 * TJ + q) * a] = ((t0 + t1) + t2) + t3;
        }
