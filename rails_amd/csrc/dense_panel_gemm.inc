// dense_panel_gemm.inc -- the body of the panel GEMM kernels k_panel_gemm and k_panel_gemm2 (dense_gemm.hip), included once in each.  The kernel
// supplies its parameters (alpha, k = the columns of X, C, r, beta, Yp, ldy, m), the left operand Xo (a OneSeg or a TwoSeg) and
// RAILS_PG_VEC4(c): may columns c .. c + 3 of a row be fetched as two 16-byte loads (aligned rows, one segment, inside the operand).
    constexpr int RL = 16 * TR + 4; // LDS row length (doubles): +4 keeps the 4 k-groups on disjoint banks
    __shared__ double Cs[KC * RL];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int li = lane & 15, kk = lane >> 4;
    const int64_t r0 = ((int64_t)blockIdx.x * 4 + wave) * 16;
    const int64_t myrow = r0 + li;
    const bool rowok = myrow < m;

    v4f64 acc[TR];
#pragma unroll
    for (int t = 0; t < TR; ++t) acc[t] = (v4f64){0.0, 0.0, 0.0, 0.0};

    const auto xrow = Xo.row(myrow); // (not read when the row is past m)
    for (int kc = 0; kc < k; kc += KC) {
        __syncthreads();
        // stage C[kc:kc+KC, 0:r) (col-major, ld = k) into LDS row-major, zero padded
        for (int idx = threadIdx.x; idx < KC * 16 * TR; idx += 256) {
            int kl = idx % KC, j = idx / KC;
            double v = 0.0;
            if (kc + kl < k && j < r) v = C[(kc + kl) + (int64_t)j * k];
            Cs[kl * RL + j] = v;
        }
        __syncthreads();
#pragma unroll
        for (int kb = 0; kb < KC; kb += 16) {
            const int kcol = kc + kb + 4 * kk;
            double xs[4];
            if (rowok && RAILS_PG_VEC4(kcol)) {
                const double *src = Xo.at(xrow, Xo.col(kcol));
                v2f64 t0 = *reinterpret_cast<const v2f64 *>(src);
                v2f64 t1 = *reinterpret_cast<const v2f64 *>(src + 2);
                xs[0] = t0.x;
                xs[1] = t0.y;
                xs[2] = t1.x;
                xs[3] = t1.y;
            } else {
#pragma unroll
                for (int s = 0; s < 4; ++s) xs[s] = (rowok && kcol + s < k) ? *Xo.at(xrow, Xo.col(kcol + s)) : 0.0;
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const double *crow = &Cs[(kb + 4 * kk + s) * RL + li];
#pragma unroll
                for (int t = 0; t < TR; ++t) acc[t] = mfma_f64(xs[s], crow[16 * t], acc[t]);
            }
        }
    }
    // D[row = kk + 4v][col = li]
#pragma unroll
    for (int t = 0; t < TR; ++t) {
        const int j = 16 * t + li;
        if (j >= r) continue;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int64_t row = r0 + kk + 4 * v;
            if (row >= m) continue;
            double *dst = Yp + row * ldy + j;
            double val = alpha * acc[t][v];
            if (beta != 0.0) val += beta * (*dst);
            *dst = val;
        }
    }
#undef RAILS_PG_VEC4
