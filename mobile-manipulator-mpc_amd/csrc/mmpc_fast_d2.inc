// part of mmpc_fast.h (mmpc_solve_fast), included twice: MMPC_SOCM 0 = the regular pass, 1 = the corrected pass of the second-order
// correction, which takes the residuals h + t of the circle / self-collision rows from io.soc instead of forming them.  Plain text on
// purpose: as a generic lambda instantiated twice the same code cost the regular pass 5-15 % in every phase it was used in.
        LANES_BEGIN
        auto &ls = MMPC_LS;
        // fraction to the boundary without divisions or branches: alpha = min(1, tau / max_i(-dt_i / t_i)) (1/t_i is at hand),
        // likewise for the multipliers with 1/z_i
        double rp = 0.0, rd = 0.0, dphi = 0.0;
        // a row's share: -dt / t, -dz / z with dz = mu / t - z - (z / t) dt, and its term of the barrier's slope.  One reciprocal per row,
        // r = 1 / (t z):  1 / t = r z,  -dz / z = 1 + dt / t - mu r   (MMPC_D2_ONE_RCP 0: the two reciprocals 1 / t, 1 / z of rounds 1-3)
#undef MMPC_D2_ROW
#if MMPC_D2_ONE_RCP
#define MMPC_D2_ROW(t, z, dtv) { const double r_ = mmpc_rcp((t) * (z)), a_ = (dtv) * (r_ * (z));                                  \
            rp = mmpc_vmax(rp, -a_); rd = mmpc_vmax(rd, (1.0 + a_) - mu * r_); dphi -= mu * a_; }
#else
#define MMPC_D2_ROW(t, z, dtv) { const double it_ = mmpc_rcp(t), dzv_ = mu * it_ - (z) - (z) * it_ * (dtv);                        \
            rp = mmpc_vmax(rp, -(dtv) * it_); rd = mmpc_vmax(rd, -dzv_ * mmpc_rcp(z)); dphi -= mu * (dtv) * it_; }
#endif
        if (RG > 1 && M > 0) {   // circle rows where RG lanes share a stage
            MMPC_ROW_LANE
            if (rlane) {
                const double dx0 = DXU[MMPC_MUL24(rk, NV)], dx1 = DXU[MMPC_MUL24(rk, NV) + 1], dsk = DS[rk];
                const double px = XU[MMPC_MUL24(rk, NV)], py = XU[MMPC_MUL24(rk, NV) + 1], sk = S[rk];
                double ob[MCR * 3];
#pragma unroll
                for (int r = 0; r < MCR; r++) {
                    const MmpcObs o = obs_ptr(rk, rs + RG * r < M ? rs + RG * r : 0);
                    ob[3 * r] = o.x(); ob[3 * r + 1] = o.y(); ob[3 * r + 2] = o.r();
                }
#pragma unroll
                for (int r = 0; r < MCR; r++) {
                    if (rs + RG * r < M) {
                        const double ddx = px - ob[3 * r], ddy = py - ob[3 * r + 1], m2 = ddx * ddx + ddy * ddy, id = mmpc_rsqrt(m2), d = m2 * id;
                        const double hv = (ob[3 * r + 2] + MMPC_BASE_R) - d - sk;
                        const double t = ls.ct[r], z = ls.cz[r];
                        const double jd = -(ddx * dx0 + ddy * dx1) * id - dsk;
                        double res = hv + t;
                        if constexpr (socm) res = io.soc[O_AR + rk * NRS + rs + RG * r];
                        const double dtv = -res - jd;
                        ls.cdt[r] = dtv;
                        MMPC_D2_ROW(t, z, dtv)
                    }
                }
            }
        }
        if (lane < NS) {
            const int k = lane;
            const double *dx = DXU + MMPC_MUL24(k, NV);
            const double dsk = DS[k], dsks = DS[slack_idx(k)];
            const double px = XU[MMPC_MUL24(k, NV)], py = XU[MMPC_MUL24(k, NV) + 1], sk = S[k];
            double ob[(MC > 0 ? MC : 1) * 3];
#pragma unroll
            for (int m = 0; m < (RG > 1 ? 0 : M); m++) { const MmpcObs o = obs_ptr(k, m); ob[3 * m] = o.x(); ob[3 * m + 1] = o.y(); ob[3 * m + 2] = o.r(); }
#pragma unroll
            for (int m = 0; m < (RG > 1 ? 0 : M); m++) {
                const double ddx = px - ob[3 * m], ddy = py - ob[3 * m + 1], m2 = ddx * ddx + ddy * ddy, id = mmpc_rsqrt(m2), d = m2 * id;
                const double hv = (ob[3 * m + 2] + MMPC_BASE_R) - d - sk;
                const double t = ls.ct[m], z = ls.cz[m];
                const double jd = -(ddx * dx[0] + ddy * dx[1]) * id - dsk;
                double res = hv + t;
                if constexpr (socm) res = io.soc[O_AR + k * NRS + m];
                const double dtv = -res - jd;
                ls.cdt[m] = dtv;
                MMPC_D2_ROW(t, z, dtv)
            }
            double sn = 0.0, cs = 0.0, dr[3] = {0, 0, 0}, dz[3] = {0, 0, 0};
            if (NSELF) {
                sn = TRG[MMPC_MUL24(k, F::TRGS)]; cs = TRG[MMPC_MUL24(k, F::TRGS) + 1];
#pragma unroll
                for (int a = 0; a < 3; a++) { dr[a] = TRG[MMPC_MUL24(k, F::TRGS) + 2 + a]; dz[a] = TRG[MMPC_MUL24(k, F::TRGS) + 5 + a]; }
            }
            const double sks = S[slack_idx(k)];
#pragma unroll
            for (int i = 0; i < NSELF; i++) {
                double g6[6];
                const double hv = mmpc_self_row(i, px, py, cs, sn, dr, dz, g6) - sks;
                const double t = ls.st[i], z = ls.sz[i];
                double jd = -dsks;
#pragma unroll
                for (int a = 0; a < 6; a++) jd += g6[a] * dx[mmpc_y(a)];
                double res = hv + t;
                if constexpr (socm) res = io.soc[O_AR + k * NRS + M + i];
                const double dtv = -res - jd;
                ls.sdt[i] = dtv;
                MMPC_D2_ROW(t, z, dtv)
            }
            dphi += 2 * Sw * S[k] * dsk;
        }
        MMPC_PAIR_SETUP
#pragma unroll
        for (int p = 0; p < NPASS; p++) {
            MMPC_PAIR(p)
            if (pok) {
                const double lo = ls.b_lo[p], hi = ls.b_hi[p];
                const bool alo = lo > -1e299, ahi = hi < 1e299;
                const double val = XU[idx], dv = DXU[idx];
                dphi += RB[idx] * dv;   // RB = plain cost gradient of this variable (kept by the evaluation)
                if (alo) {
                    const double t = mmpc_box_t(val - lo), z = ls.lo_z[p], dtv = dv;
                    MMPC_D2_ROW(t, z, dtv)
                }
                if (ahi) {
                    const double t = mmpc_box_t(hi - val), z = ls.hi_z[p], dtv = -dv;
                    MMPC_D2_ROW(t, z, dtv)
                }
            }
        }
        MMPC_WR(0) = rp; MMPC_WR(1) = rd; MMPC_WR(2) = dphi;
        LANES_END
