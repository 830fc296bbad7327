// part of mmpc_fast.h (mmpc_solve_fast), included twice: MMPC_SOCM 0 = the regular pass, 1 = the corrected pass of the second-order
// correction, which takes the residuals h + t of the circle / self-collision rows from io.soc instead of forming them.  Plain text on
// purpose: as a generic lambda instantiated twice the same code cost the regular pass 5-15 % in every phase it was used in.
            if (RG > 1 && M > 0) {
                LANES_BEGIN
                auto &ls = MMPC_LS;
                MMPC_ROW_LANE
                double cp[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
                if (rlane) {
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
                            const double g0 = -ddx * id, g1 = -ddy * id, hv = (ob[3 * r + 2] + MMPC_BASE_R) - d - sk;
                            const double t = ls.ct[r], z = ls.cz[r], it_ = mmpc_rcp(t), w = z * it_;
                            double res = hv + t;
                            if constexpr (socm) res = io.soc[O_AR + rk * NRS + rs + RG * r];   // corrected pass: (h + t)_soc
                            const double zh = mu * it_ + w * res;
                            cp[0] += w * g0 * g0; cp[1] += w * g1 * g0; cp[2] += w * g1 * g1;
                            if (exact) { const double zi = z * id; cp[0] -= zi * (1 - g0 * g0); cp[1] += zi * g0 * g1; cp[2] -= zi * (1 - g1 * g1); }
                            cp[3] += g0 * zh; cp[4] += g1 * zh;
                            cp[5] += w; cp[6] -= zh; cp[7] += w * g0; cp[8] += w * g1;
                        }
                    }
                    if (rs > 0) {
                        double *cpo = HXX + MMPC_MUL24(rk, NXX) + (rs - 1) * 9;
#pragma unroll
                        for (int q = 0; q < 9; q++) cpo[q] = cp[q];
                    }
                }
#pragma unroll
                for (int q = 0; q < 9; q++) ls.cp[q] = cp[q];
                LANES_END
            }
