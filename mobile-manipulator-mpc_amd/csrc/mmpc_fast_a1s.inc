// part of mmpc_fast.h (mmpc_solve_fast), included twice: MMPC_SOCM 0 = the regular pass, 1 = the corrected pass of the second-order
// correction, which takes the residuals h + t of the circle / self-collision rows from io.soc instead of forming them.  Plain text on
// purpose: as a generic lambda instantiated twice the same code cost the regular pass 5-15 % in every phase it was used in.
            LANES_BEGIN
            auto &ls = MMPC_LS;
            if (lane < NS) {
                const int k = lane, k1 = k < N ? k + 1 : k;
                // every LDS word of this stage first (one round trip instead of one per block below)
                double hxx[NXX], qx[NX], wd[NX], ob[RG > 1 ? (RG - 1) * 9 : (MC > 0 ? MC : 1) * 3];   // (ob: as in the evaluation)
#pragma unroll
                for (int j = 0; j < NX; j++) { wd[j] = CST[(k < N ? MMPC_C_WQ : MMPC_C_WP) + j]; qx[j] = RB[MMPC_MUL24(k, NV) + j]; }
                const double *cv = CV + MMPC_MUL24(k, MMPC_NCV);
                const double l3 = LAM[MMPC_MUL24(k1, NX) + 3], l4 = LAM[MMPC_MUL24(k1, NX) + 4], cv3 = cv[3], cv4 = cv[4], cv9 = cv[9], cv10 = cv[10];
                const double px = XU[MMPC_MUL24(k, NV)], py = XU[MMPC_MUL24(k, NV) + 1], sk = S[k], sks = S[slack_idx(k)];
                if (RG > 1) {
#pragma unroll
                    for (int q = 0; q < (RG - 1) * 9; q++) ob[q] = M > 0 ? HXX[MMPC_MUL24(k, NXX) + q] : 0.0;
                } else {
#pragma unroll
                    for (int m = 0; m < M; m++) { const MmpcObs o = obs_ptr(k, m); ob[3 * m] = o.x(); ob[3 * m + 1] = o.y(); ob[3 * m + 2] = o.r(); }
                }
                double sn = 0.0, cs = 0.0, dr[3] = {0, 0, 0}, dz[3] = {0, 0, 0};
                if (NSELF) {
                    sn = TRG[MMPC_MUL24(k, F::TRGS)]; cs = TRG[MMPC_MUL24(k, F::TRGS) + 1];
#pragma unroll
                    for (int a = 0; a < 3; a++) { dr[a] = TRG[MMPC_MUL24(k, F::TRGS) + 2 + a]; dz[a] = TRG[MMPC_MUL24(k, F::TRGS) + 5 + a]; }
                }
#pragma unroll
                for (int e = 0; e < NXX; e++) hxx[e] = 0.0;
#pragma unroll
                for (int j = 0; j < NX; j++) hxx[j * (j + 1) / 2 + j] = wd[j] + reg;
                double h02 = 0.0;
                if (k < N && dyn_curv) {
                    hxx[5] += l3 * cv4 - l4 * cv3;
                    hxx[19] += dt * l3;
                    hxx[18] -= dt * l4;
                    h02 = -(-l3 * cv10 + l4 * cv9);
                }
                double hss = 2 * Sw, gss = 2 * Sw * sk, vx[6] = {0, 0, 0, 0, 0, 0};
                if (RG > 1 && M > 0) {   // circle rows: own lane's sums first, then the other lanes' in lane order
#pragma unroll
                    for (int q = 0; q < 9; q++) {
                        double c = ls.cp[q];
#pragma unroll
                        for (int g = 0; g < RG - 1; g++) c += ob[9 * g + q];
                        if (q < 3) hxx[q] += c; else if (q < 5) qx[q - 3] += c; else if (q == 5) hss += c; else if (q == 6) gss += c; else vx[q - 7] += c;
                    }
                }
#pragma unroll
                for (int m = 0; m < (RG > 1 ? 0 : M); m++) {
                    // row geometry is re-derived from x_k (cheaper than keeping it in registers)
                    const double *o = ob + 3 * m;
                    const double ddx = px - o[0], ddy = py - o[1], m2 = ddx * ddx + ddy * ddy, id = mmpc_rsqrt(m2), d = m2 * id;
                    const double g0 = -ddx * id, g1 = -ddy * id, hv = (o[2] + MMPC_BASE_R) - d - sk;
                    const double t = ls.ct[m], z = ls.cz[m], it_ = mmpc_rcp(t), w = z * it_;
                    double res = hv + t;
                    if constexpr (socm) res = io.soc[O_AR + k * NRS + m];   // corrected pass: (h + t)_soc
                    const double zh = mu * it_ + w * res;
                    hxx[0] += w * g0 * g0; hxx[1] += w * g1 * g0; hxx[2] += w * g1 * g1;
                    if (exact) { const double zi = z * id; hxx[0] -= zi * (1 - g0 * g0); hxx[1] += zi * g0 * g1; hxx[2] -= zi * (1 - g1 * g1); }
                    qx[0] += g0 * zh; qx[1] += g1 * zh;
                    hss += w; gss -= zh; vx[0] += w * g0; vx[1] += w * g1;
                }
                if (NSELF) {
#pragma unroll
                    for (int i = 0; i < NSELF; i++) {
                        double g6[6];
                        const double hv = mmpc_self_row(i, px, py, cs, sn, dr, dz, g6) - sks;
                        const double t = ls.st[i], z = ls.sz[i], it_ = mmpc_rcp(t), w = z * it_;
                        double res = hv + t;
                        if constexpr (socm) res = io.soc[O_AR + k * NRS + M + i];
                        const double zh = mu * it_ + w * res;
                        // (the terminal stage's self rows belong to s_{N-1}, quirk Q1: they do not enter this lane's s_k block)
                        const double wk = k < N ? w : 0.0, zhk = k < N ? zh : 0.0;
#pragma unroll
                        for (int a = 0; a < 6; a++) {
                            const double wa = w * g6[a];
#pragma unroll
                            for (int b = 0; b <= a; b++) hxx[mmpc_y(a) * (mmpc_y(a) + 1) / 2 + mmpc_y(b)] += wa * g6[b];
                            qx[mmpc_y(a)] += g6[a] * zh;
                            vx[a] += wk * g6[a];
                        }
                        hss += wk; gss -= zhk;
                    }
                }
                // Q1: terminal self rows -> s_{N-1}.  a = v + A^T vN, b = B^T vN, gamma = g_s - vN.c.  Lane N-1 publishes
                // (a, b, gamma, 1/h_ss); the dense rank-one blocks are applied by all lanes in the next phase, so this lane
                // stores its blocks WITHOUT the elimination of s (weight 0 below; one store sequence for every lane)
                const bool q1 = NSELF && k == N - 1;
                if (q1) {
                    const double hssN = SN[0], gssN = -(mu * SN[1] + SN[2]);
                    hss += hssN; gss += gssN;
                }
                const double ih = mmpc_rcp(hss), ihs = q1 ? 0.0 : ih;
                if (!NSELF && k == N - 1) {
                    for (int c = 0; c < NU * NX; c++) HUXL[c] = 0.0;
                    for (int c = 0; c < NUU; c++) HUUL[c] = 0.0;
                }
                {
                    constexpr int ny = NSELF ? 6 : 2;
#pragma unroll
                    for (int a = 0; a < ny; a++) {
#pragma unroll
                        for (int b = 0; b <= a; b++) hxx[mmpc_y(a) * (mmpc_y(a) + 1) / 2 + mmpc_y(b)] -= vx[a] * vx[b] * ihs;
                        qx[mmpc_y(a)] += vx[a] * gss * ihs;
                    }
                    if (k < N) {
#pragma unroll
                        for (int c = 0; c < NU; c++) QXU[MMPC_MUL24(k, NV) + NX + c] = RB[MMPC_MUL24(k, NV) + NX + c];
                    }
#pragma unroll
                    for (int e = 0; e < NXX; e++) HXX[MMPC_MUL24(k, NXX) + e] = hxx[e];
#pragma unroll
                    for (int j = 0; j < NX; j++) QXU[MMPC_MUL24(k, NV) + j] = qx[j];
                }
                if (q1) {
                    double vf[NX], a[NX], b[NU];
#pragma unroll
                    for (int j = 0; j < NX; j++) { vf[j] = 0.0; a[j] = 0.0; }
#pragma unroll
                    for (int q = 0; q < 6; q++) { vf[mmpc_y(q)] = SN[4 + q]; a[mmpc_y(q)] = vx[q]; }
                    const double *cv = CV + MMPC_MUL24(k, MMPC_NCV);
                    a[0] += vf[0]; a[1] += vf[1];
                    a[2] += vf[2] + cv[3] * vf[3] + cv[4] * vf[4];
                    a[3] += vf[3] + dt * vf[0] + cv[5] * vf[4];
                    a[4] += vf[4] + dt * vf[1] + cv[6] * vf[3];
                    a[5] += vf[5] + dt * vf[2] + cv[7] * vf[3] + cv[8] * vf[4];
                    b[0] = cv[9] * vf[3] + cv[10] * vf[4];
                    b[1] = dt * vf[5];
                    if (KIND == 0) { a[6] += vf[6]; a[7] += vf[7]; a[8] += vf[8]; b[2] = dt * vf[6]; b[3] = dt * vf[7]; b[4] = dt * vf[8]; }
                    double gam = gss;
#pragma unroll
                    for (int j = 0; j < NX; j++) gam -= vf[j] * CD[MMPC_MUL24(k, NX) + j];
#pragma unroll
                    for (int j = 0; j < NX; j++) Q1V[j] = a[j];
#pragma unroll
                    for (int c = 0; c < NU; c++) Q1V[NX + c] = b[c];
                    Q1V[NV] = gam * ih; Q1V[NV + 1] = ih;
                }
                ls.hss = hss; ls.gss = gss;
#pragma unroll
                for (int a = 0; a < 6; a++) ls.vx[a] = vx[a];
                HUX02[k] = h02;
#pragma unroll
                for (int c = 0; c < NU; c++) HUUD[MMPC_MUL24(k, NU) + c] = CST[MMPC_C_RW2 + c * NU + c] + reg;
            }
            LANES_END
