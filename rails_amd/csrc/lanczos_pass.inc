// lanczos_pass.inc -- the one body of the pass kernels of lanczos.hip, included by k_lanczos_pass<NCH, U> (SP = false: B is the dense
// panel a.B) and k_lanczos_pass_sparse<NCH, U> (SP = true: B is the sparse right-hand side sp, a.p = 0 and a.B unused; B's part of r comes
// from sparse_rows, and c'_B is made by k_sprhs_bt, not here).  In scope: NCH, U, constexpr bool SP, LzArgs a, sp.
    __shared__ double red[4][(4 * NCH + 2) * 64 + 1];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const bool init = a.step < 0;
    const double done = a.state[lz::DONE];
    const int ncoef = 2 * a.k + a.p + 1;
    double *myp = a.partial + (int64_t)blockIdx.x * ncoef;
    if (done != 0.0) {
        for (int i = threadIdx.x; i < ncoef; i += 256) myp[i] = 0.0;
        return;
    }
    const double alpha = init ? 0.0 : a.state[lz::ALPHA];
    const double betap = init ? 0.0 : a.state[lz::BETA_PREV];
    const double invb = init ? 1.0 : a.state[lz::INV_BETA];

    v2f64 gav[NCH], gmv[NCH], gb;
    bool ok0[NCH], ok1[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        int col = 2 * (lane + 64 * c);
        ok0[c] = col < a.k;
        ok1[c] = col + 1 < a.k;
        gav[c].x = (!init && ok0[c]) ? a.coef[col] : 0.0;
        gav[c].y = (!init && ok1[c]) ? a.coef[col + 1] : 0.0;
        gmv[c].x = (!init && ok0[c]) ? a.coef[a.k + col] : 0.0;
        gmv[c].y = (!init && ok1[c]) ? a.coef[a.k + col + 1] : 0.0;
    }
    const bool bok0 = 2 * lane < a.p, bok1 = 2 * lane + 1 < a.p;
    // clamped (always valid, 16-B aligned) column offsets for the unconditional loads: lanes past the last column pair
    // re-read that pair (same cache line as their neighbour: no extra HBM traffic), never the padding beyond it
    int cav_off[NCH], cmv_off[NCH];
    {
        const int klast = a.k > 1 ? ((a.k - 1) & ~1) : 0;
        const int lim_av = klast < a.av_room - 2 ? klast : a.av_room - 2;
        const int lim_mv = klast < a.mv_room - 2 ? klast : a.mv_room - 2;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int col = 2 * (lane + 64 * c);
            cav_off[c] = col < lim_av ? col : lim_av;
            cmv_off[c] = col < lim_mv ? col : lim_mv;
        }
    }
    const int plast = a.p > 1 ? ((a.p - 1) & ~1) : 0;
    const int lim_b = plast < a.b_room - 2 ? plast : a.b_room - 2;
    const int cb_off = 2 * lane < lim_b ? 2 * lane : lim_b;
    gb.x = (!init && bok0) ? a.coef[2 * a.k + 2 * lane] : 0.0;
    gb.y = (!init && bok1) ? a.coef[2 * a.k + 2 * lane + 1] : 0.0;
    v2f64 cav[NCH], cmv[NCH], cb;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        cav[c] = (v2f64){0.0, 0.0};
        cmv[c] = (v2f64){0.0, 0.0};
    }
    cb = (v2f64){0.0, 0.0};
    double rr = 0.0;

    double *q_cur = a.Qc + (int64_t)(init ? 0 : a.step) * a.mpad;
    const double *q_prev = a.Qc + (int64_t)((init || a.step == 0) ? 0 : a.step - 1) * a.mpad;
    double *q_next = a.Qc + (int64_t)(a.step + 1) * a.mpad;
    const bool have_prev = (!init && a.step > 0);

    const int64_t ngroups = a.mpad / 64;
    for (int64_t grp = (int64_t)blockIdx.x * 4 + wave; grp < ngroups; grp += (int64_t)gridDim.x * 4) {
        const int64_t row0 = grp * 64;
        double qn = q_cur[row0 + lane] * invb; // rows >= m hold zeros
        double qm = have_prev ? q_prev[row0 + lane] : 0.0;
        if (!init) q_cur[row0 + lane] = qn; // store the normalised q_i
        double rvec = 0.0;
        const int nrows = (int)((a.m - row0) < 64 ? (a.m - row0) : 64);
        double sB = 0.0;
        if constexpr (SP)
            if (!init && nrows > 0) sB = sparse_rows(sp, row0, nrows, lane);
        // U rows per trip of the loop: their 2*NCH+1 row loads are all issued before the first reduction, the
        // U wave reductions are independent chains (rows are independent of each other)
        for (int j0 = 0; j0 < nrows; j0 += U) {
            // all row loads are UNCONDITIONAL (clamped row / column, values masked afterwards with selects): a load
            // under a lane-dependent branch makes hipcc wait vmcnt(0) at the join and serialises the loads
            v2f64 xav[U][NCH], xmv[U][NCH], xb[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int jr = (j0 + u) < nrows ? (j0 + u) : (nrows - 1);
                const int64_t row = row0 + jr;
                const double *pav = a.AV + row * a.ldav;
                const double *pmv = a.MV + row * a.ldmv;
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    xav[u][c] = *reinterpret_cast<const v2f64 *>(pav + cav_off[c]);
                    xmv[u][c] = *reinterpret_cast<const v2f64 *>(pmv + cmv_off[c]);
                }
                if constexpr (!SP) xb[u] = *reinterpret_cast<const v2f64 *>(a.B + row * a.ldb + cb_off);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    xav[u][c].x = ok0[c] ? xav[u][c].x : 0.0;
                    xav[u][c].y = ok1[c] ? xav[u][c].y : 0.0;
                    xmv[u][c].x = ok0[c] ? xmv[u][c].x : 0.0;
                    xmv[u][c].y = ok1[c] ? xmv[u][c].y : 0.0;
                }
                if constexpr (!SP) {
                    xb[u].x = bok0 ? xb[u].x : 0.0;
                    xb[u].y = bok1 ? xb[u].y : 0.0;
                }
            }
            double r[U];
            if (init) {
#pragma unroll
                for (int u = 0; u < U; ++u) r[u] = ((j0 + u) < nrows) ? readlane_f64(qn, (j0 + u) & 63) : 0.0;
            } else {
                double t[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    double tt = 0.0;
#pragma unroll
                    for (int c = 0; c < NCH; ++c) {
                        tt = __builtin_fma(xav[u][c].x, gav[c].x, tt);
                        tt = __builtin_fma(xav[u][c].y, gav[c].y, tt);
                        tt = __builtin_fma(xmv[u][c].x, gmv[c].x, tt);
                        tt = __builtin_fma(xmv[u][c].y, gmv[c].y, tt);
                    }
                    if constexpr (!SP) {
                        tt = __builtin_fma(xb[u].x, gb.x, tt);
                        tt = __builtin_fma(xb[u].y, gb.y, tt);
                    }
                    t[u] = tt;
                }
#pragma unroll
                for (int u = 0; u < U; ++u) t[u] = wave_sum(t[u]);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int jj = (j0 + u) & 63;
                    const double qi = readlane_f64(qn, jj);
                    const double qmi = readlane_f64(qm, jj);
                    if constexpr (SP)
                        r[u] = ((j0 + u) < nrows) ? ((t[u] + readlane_f64(sB, jj)) - alpha * qi - betap * qmi) : 0.0;
                    else
                        r[u] = ((j0 + u) < nrows) ? (t[u] - alpha * qi - betap * qmi) : 0.0;
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    cav[c].x = __builtin_fma(xav[u][c].x, r[u], cav[c].x);
                    cav[c].y = __builtin_fma(xav[u][c].y, r[u], cav[c].y);
                    cmv[c].x = __builtin_fma(xmv[u][c].x, r[u], cmv[c].x);
                    cmv[c].y = __builtin_fma(xmv[u][c].y, r[u], cmv[c].y);
                }
                if constexpr (!SP) {
                    cb.x = __builtin_fma(xb[u].x, r[u], cb.x);
                    cb.y = __builtin_fma(xb[u].y, r[u], cb.y);
                }
                rr = __builtin_fma(r[u], r[u], rr);
                rvec = (lane == j0 + u) ? r[u] : rvec;
            }
        }
        if (!init) q_next[row0 + lane] = rvec;
    }

    // block reduction in a fixed order: wave 0 += wave 1, 2, 3
    double *mine = red[wave];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        mine[(4 * c + 0) * 64 + lane] = cav[c].x;
        mine[(4 * c + 1) * 64 + lane] = cav[c].y;
        mine[(4 * c + 2) * 64 + lane] = cmv[c].x;
        mine[(4 * c + 3) * 64 + lane] = cmv[c].y;
    }
    if constexpr (!SP) {
        mine[(4 * NCH + 0) * 64 + lane] = cb.x;
        mine[(4 * NCH + 1) * 64 + lane] = cb.y;
    }
    if (lane == 0) mine[(4 * NCH + 2) * 64] = rr;
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                int slot = (4 * c + e) * 64 + lane;
                double s = ((red[0][slot] + red[1][slot]) + red[2][slot]) + red[3][slot];
                int col = 2 * (lane + 64 * c) + (e & 1);
                if (col < a.k) myp[(e < 2 ? 0 : a.k) + col] = s;
            }
        }
        if constexpr (!SP) {
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                int slot = (4 * NCH + e) * 64 + lane;
                double s = ((red[0][slot] + red[1][slot]) + red[2][slot]) + red[3][slot];
                int col = 2 * lane + e;
                if (col < a.p) myp[2 * a.k + col] = s;
            }
        }
        if (lane == 0) {
            int slot = (4 * NCH + 2) * 64;
            myp[2 * a.k + a.p] = ((red[0][slot] + red[1][slot]) + red[2][slot]) + red[3][slot];
        }
    }
