// dense_gram.inc -- the body of the row-split Gram kernels k_gram and k_gram2 (dense_gram.hip), included once in each.  The kernel supplies its
// parameters (a, Y, ldy, b, m, rows_per_slab, ngj, partial) and the left operand Xo, a OneSeg or a TwoSeg.
    __shared__ double red[TI * TJ * 256];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int li = lane & 15, kk = lane >> 4;
    const int gi = blockIdx.y / ngj, gj = blockIdx.y % ngj;
    const int xcol0 = gi * TI * 16, ycol0 = gj * TJ * 16;
    const int64_t r_begin = (int64_t)blockIdx.x * rows_per_slab;
    int64_t r_end = r_begin + rows_per_slab;
    if (r_end > m) r_end = m;

    v4f64 acc[TI][TJ];
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j) acc[i][j] = (v4f64){0.0, 0.0, 0.0, 0.0};

    // Loads without branches (a load inside a conditional gets its own exec-masked block, and the compiler then waits for ALL loads in
    // flight -- the next step's too -- before the first MFMA: see k_gram_cols): columns outside the operands are clamped to the tile's
    // first column (their results are never written), rows past the slab to its last row with the Y operand zeroed.
    decltype(Xo.col(0)) xcol[TI];
    int yoff[TJ];
#pragma unroll
    for (int i = 0; i < TI; ++i) xcol[i] = Xo.col((xcol0 + 16 * i + li) < a ? xcol0 + 16 * i + li : 0);
#pragma unroll
    for (int j = 0; j < TJ; ++j) yoff[j] = (ycol0 + 16 * j + li) < b ? ycol0 + 16 * j + li : 0;

    // software pipeline: the operands of the next 4-row step are in flight while the MFMAs of this one run (one step's loads per
    // wave do not cover the HBM latency at 3 waves per SIMD: the Gram at 17 columns ran at 37 % of the HBM rate without it)
    auto fetch = [&](int64_t r, double *xa, double *yb) {
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
    };
    double xa[TI], yb[TJ], xn[TI], yn[TJ];
    int64_t r = r_begin + 4 * wave;
    if (r < r_end) fetch(r, xa, yb);
    for (; r < r_end; r += 16) {
        const bool more = r + 16 < r_end;
        if (more) fetch(r + 16, xn, yn);
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int j = 0; j < TJ; ++j) acc[i][j] = mfma_f64(xa[i], yb[j], acc[i][j]);
        if (more) {
#pragma unroll
            for (int i = 0; i < TI; ++i) xa[i] = xn[i];
#pragma unroll
            for (int j = 0; j < TJ; ++j) yb[j] = yn[j];
        }
    }

    // cross-wave reduction in a fixed order (wave 0 += wave 1, 2, 3)
    for (int w = 1; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int i = 0; i < TI; ++i)
#pragma unroll
                for (int j = 0; j < TJ; ++j)
#pragma unroll
                    for (int v = 0; v < 4; ++v) red[((i * TJ + j) * 4 + v) * 64 + lane] = acc[i][j][v];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int i = 0; i < TI; ++i)
#pragma unroll
                for (int j = 0; j < TJ; ++j)
#pragma unroll
                    for (int v = 0; v < 4; ++v) acc[i][j][v] += red[((i * TJ + j) * 4 + v) * 64 + lane];
        }
        __syncthreads();
    }
    if (wave == 0) {
        double *P = partial + (int64_t)blockIdx.x * a * b;
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int j = 0; j < TJ; ++j)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    int ci = xcol0 + 16 * i + kk + 4 * v; // D row  -> X column
                    int cj = ycol0 + 16 * j + li;         // D col  -> Y column
                    if (ci < a && cj < b) P[ci + (int64_t)cj * a] = acc[i][j][v];
                }
    }
