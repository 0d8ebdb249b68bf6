// solution_rowform.inc -- the one body of k_panel_rowquad<TR> and k_panel_rowpair<TR> (solution.hip), included once in each:
//   out[i] (+)= sum_{j < r} (sum_{l < k} U[a(i), l] St[l, j]) U[b(i), j0 + j],   i < Rw.n
// The kernel supplies `Rw`: Rw.n results, Rw.a(i) / Rw.b(i) the rows of U that result i takes its left and right factor from (i < Rw.n; the
// identity for the row form, two index arrays for the pair form), and the arguments U, ldu, k, St, j0, r, out, ldo, vec_ok, accumulate.  A
// wave's 16 A-operand rows are rows a(.), the epilogue multiplies the accumulator tile with rows b(.); results past Rw.n in a wave's tile
// read the rows of result Rw.n - 1 and write nothing.
    constexpr int KC = 32, RL = 16 * TR + 4, CHUNK_B = KC * RL * 8, PIECES = CHUNK_B / 1024;
    static_assert(CHUNK_B % 1024 == 0, "whole LDS-DMA pieces per chunk");
    extern __shared__ double Cs[]; // 2 x KC x RL
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int li = lane & 15, kk = lane >> 4;
    const int64_t r0 = ((int64_t)blockIdx.x * 8 + wave) * 16;
    const int64_t myrow = r0 + li;
    const bool rowok = myrow < Rw.n;
    const int nchunks = (k + KC - 1) / KC;
    const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)Cs;
    const uint32_t lane16 = (uint32_t)lane * 16u;
    auto stage = [&](int chunk) { // this wave's pieces of a chunk: piece p goes to wave p % 8
        const char *src = reinterpret_cast<const char *>(St) + (size_t)chunk * CHUNK_B;
        const uint32_t dst = lds_base + (uint32_t)((chunk & 1) * CHUNK_B);
        for (int p = wave; p < PIECES; p += 8) {
            uint32_t keep;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(lane16), "s"(src + (size_t)p * 1024), "s"(dst + (uint32_t)(p * 1024)) : "memory");
        }
    };
    v4f64 acc[TR];
#pragma unroll
    for (int t = 0; t < TR; ++t) acc[t] = (v4f64){0.0, 0.0, 0.0, 0.0};
    const double *xrow = U + Rw.a(rowok ? myrow : Rw.n - 1) * ldu; // results past the end read the last one's row; they are never written
    auto fetch = [&](int kcol, double *xs) {
        if (vec_ok && kcol + 4 <= k) {
            v2f64 t0 = *reinterpret_cast<const v2f64 *>(xrow + kcol);
            v2f64 t1 = *reinterpret_cast<const v2f64 *>(xrow + kcol + 2);
            xs[0] = t0.x;
            xs[1] = t0.y;
            xs[2] = t1.x;
            xs[3] = t1.y;
        } else {
#pragma unroll
            for (int s = 0; s < 4; ++s) xs[s] = (kcol + s < k) ? xrow[kcol + s] : 0.0;
        }
    };
    double xa[4], xb[4];
    stage(0);
    fetch(4 * kk, xa);
    fetch(16 + 4 * kk, xb);
    asm volatile("s_waitcnt vmcnt(0)" : : : "memory");
    __builtin_amdgcn_s_barrier();
    for (int ci = 0; ci < nchunks; ++ci) {
        if (ci + 1 < nchunks) stage(ci + 1); // into the buffer every wave left at the barrier above
        double xc[4], xd[4];
        fetch((ci + 1) * KC + 4 * kk, xc); // past k: zeros, no load
        fetch((ci + 1) * KC + 16 + 4 * kk, xd);
        const double *cb = Cs + (size_t)(ci & 1) * (KC * RL);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const double *crow = &cb[(4 * kk + s) * RL + li];
#pragma unroll
            for (int t = 0; t < TR; ++t) acc[t] = mfma_f64(xa[s], crow[16 * t], acc[t]);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const double *crow = &cb[(16 + 4 * kk + s) * RL + li];
#pragma unroll
            for (int t = 0; t < TR; ++t) acc[t] = mfma_f64(xb[s], crow[16 * t], acc[t]);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            xa[s] = xc[s];
            xb[s] = xd[s];
        }
        // the next chunk has landed (this wave's pieces; then everybody's) and nobody reads this chunk's buffer any more
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" : : : "memory");
        __builtin_amdgcn_s_barrier();
    }
    // P[row kk + 4v][column 16t + li] is in acc[t][v]: times U's row b(.) at the same column, summed over the columns
    double q[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const int64_t row = r0 + kk + 4 * v;
        const double *urow = U + Rw.b(row < Rw.n ? row : Rw.n - 1) * ldu + j0;
#pragma unroll
        for (int t = 0; t < TR; ++t) {
            const int j = 16 * t + li;
            const double u = urow[j < r ? j : 0]; // columns past the slice: acc is zero there (zero padding of the packed S)
            q[v] += acc[t][v] * (j < r ? u : 0.0);
        }
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) q[v] += __shfl_xor(q[v], off, 64);
    }
    if (li == 0) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int64_t row = r0 + kk + 4 * v;
            if (row >= Rw.n) continue;
            double *dst = out + row * ldo;
            *dst = accumulate ? *dst + q[v] : q[v];
        }
    }
