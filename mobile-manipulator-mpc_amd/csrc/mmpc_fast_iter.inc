// The body of the iteration loop of mmpc_solve_fast (mmpc_fast.h), included TWICE:
//   MMPC_ITER_SOC 0  the loop every solve runs in.  It carries no code of the second-order correction beyond the test that asks
//                    for one (which leaves the loop);
//   MMPC_ITER_SOC 1  the same iteration with the correction's state machine (states 1-3, see mmpc_fast.h), entered only while a
//                    correction is in progress and left at the top of the first iteration after it.
// Both copies work on the same variables, so control passes between them at the loop top without any hand-over.  One loop
// with the correction's branches inside cost every solve 2.3 % (register allocation and code layout of the regular path;
// 6.80 against 6.65 ms per 8192 whole-body solves), the correction itself runs in 0.2 % of the iterations.
        MMPC_TS(0)
        // ============================================================ E1 (circle rows where RG lanes share a stage)
        if (RG > 1 && M > 0) {
            LANES_BEGIN
            auto &ls = MMPC_LS;
            double e_p = 0.0, tzmax = 0.0, tzmin = 1e300, zsum = 0.0, th = 0.0, rb0 = 0.0, rb1 = 0.0, rz = 0.0;
            MmpcLogAcc la; la.init();
            MMPC_ROW_LANE
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
                        const double dx = px - ob[3 * r], dy = py - ob[3 * r + 1], m2 = dx * dx + dy * dy, id = mmpc_rsqrt(m2), d = m2 * id;
                        const double nxv = dx * id, nyv = dy * id;
                        const double h = (ob[3 * r + 2] + MMPC_BASE_R) - d - sk;
                        const double t = ls.ct[r], z = ls.cz[r];
                        rb0 -= nxv * z; rb1 -= nyv * z; rz += z;
                        e_p = mmpc_vmax(e_p, fabs(h + t)); th += fabs(h + t); la.mul(t);
                        tzmax = mmpc_vmax(tzmax, t * z); tzmin = mmpc_vmin(tzmin, t * z); zsum += z;
                    }
                }
                // the stage lane (rs = 0) keeps its sums in registers, the others hand theirs over through the stage's Hessian block
                if (rs > 0) { double *cpo = HXX + MMPC_MUL24(rk, NXX) + (rs - 1) * 3; cpo[0] = rb0; cpo[1] = rb1; cpo[2] = rz; }
            }
            ls.cp[0] = rb0; ls.cp[1] = rb1; ls.cp[2] = rz;
            MMPC_WR(1) = e_p; MMPC_WR(2) = tzmax; MMPC_WR(3) = tzmin; MMPC_WR(4) = zsum; MMPC_WR(6) = th; MMPC_WR(7) = la.mant; MMPC_WR(0) = (double)la.ex;
            LANES_END
        }
        // ============================================================ E1 (stage lanes)
        LANES_BEGIN
        auto &ls = MMPC_LS;
        double e_p = 0.0, tzmax = 0.0, tzmin = 1e300, zsum = 0.0, zeq = 0.0, phi = 0.0, th = 0.0, slog = 0.0;
        MmpcLogAcc la; la.init();
        if (RG > 1 && M > 0) {
            e_p = MMPC_WR(1); tzmax = MMPC_WR(2); tzmin = MMPC_WR(3); zsum = MMPC_WR(4); th = MMPC_WR(6); la.mant = MMPC_WR(7); la.ex = (int)MMPC_WR(0);
        }
        if (lane < NS) {
            const int k = lane, k1 = k < N ? k + 1 : k;
            // every LDS word of this stage first (the stores below would otherwise pin each later load behind them)
            // (ob: the obstacles of this stage where the stage lane owns all circle rows, else the sums of the other lanes' rows)
            double xk[NV], xn1[NX], ln[NX], rb[NV], ob[RG > 1 ? (RG - 1) * 3 : (MC > 0 ? MC : 1) * 3];
#pragma unroll
            for (int j = 0; j < NV; j++) { xk[j] = XU[MMPC_MUL24(k, NV) + j]; rb[j] = 0.0; }
#pragma unroll
            for (int j = 0; j < NX; j++) { xn1[j] = XU[MMPC_MUL24(k1, NV) + j]; ln[j] = LAM[MMPC_MUL24(k1, NX) + j]; rb[j] = k >= 1 ? LAM[MMPC_MUL24(k, NX) + j] : 0.0; }
            if (RG > 1) {
#pragma unroll
                for (int q = 0; q < (RG - 1) * 3; q++) ob[q] = M > 0 ? HXX[MMPC_MUL24(k, NXX) + q] : 0.0;
            } else {
#pragma unroll
                for (int m = 0; m < M; m++) { const MmpcObs o = obs_ptr(k, m); ob[3 * m] = o.x(); ob[3 * m + 1] = o.y(); ob[3 * m + 2] = o.r(); }
            }
            const double sk = S[k], sks_ld = S[slack_idx(k)];
            double sn, cs;
            mmpc_sincos(xk[2], &sn, &cs);
            double *cv = CV + MMPC_MUL24(k, MMPC_NCV);
            if (k < N) {
                const double *uk = xk + NX;
                const double a32 = -dt * uk[0] * sn, a42 = dt * uk[0] * cs, a43 = dt * xk[5], a34 = -dt * xk[5],
                             a35 = -dt * xk[4], a45 = dt * xk[3], b30 = dt * cs, b40 = dt * sn;
                cv[0] = 0.0; cv[1] = 1.0; cv[2] = dt; cv[3] = a32; cv[4] = a42; cv[5] = a43; cv[6] = a34; cv[7] = a35;
                cv[8] = a45; cv[9] = b30; cv[10] = b40;
                double c[NX];
                c[0] = xk[0] + dt * xk[3] - xn1[0]; c[1] = xk[1] + dt * xk[4] - xn1[1]; c[2] = xk[2] + dt * xk[5] - xn1[2];
                c[3] = xk[3] + dt * (uk[0] * cs - xk[4] * xk[5]) - xn1[3];
                c[4] = xk[4] + dt * (uk[0] * sn + xk[3] * xk[5]) - xn1[4];
                c[5] = xk[5] + dt * uk[1] - xn1[5];
                if (KIND == 0) { c[6] = xk[6] + dt * uk[2] - xn1[6]; c[7] = xk[7] + dt * uk[3] - xn1[7]; c[8] = xk[8] + dt * uk[4] - xn1[8]; }
#pragma unroll
                for (int j = 0; j < NX; j++) { CD[MMPC_MUL24(k, NX) + j] = c[j]; e_p = mmpc_vmax(e_p, fabs(c[j])); th += fabs(c[j]); zeq += fabs(ln[j]); }
                // - A^T lam_{k+1}, - B^T lam_{k+1}  (sparse, base.py:19-26)
                rb[0] -= ln[0]; rb[1] -= ln[1];
                rb[2] -= ln[2] + a32 * ln[3] + a42 * ln[4];
                rb[3] -= ln[3] + dt * ln[0] + a43 * ln[4];
                rb[4] -= ln[4] + dt * ln[1] + a34 * ln[3];
                rb[5] -= ln[5] + dt * ln[2] + a35 * ln[3] + a45 * ln[4];
                rb[NX + 0] -= b30 * ln[3] + b40 * ln[4];
                rb[NX + 1] -= dt * ln[5];
                if (KIND == 0) {
                    rb[6] -= ln[6]; rb[7] -= ln[7]; rb[8] -= ln[8];
                    rb[NX + 2] -= dt * ln[6]; rb[NX + 3] -= dt * ln[7]; rb[NX + 4] -= dt * ln[8];
                }
            }
            double rds = 2 * Sw * sk, selfz = 0.0;
            phi += Sw * sk * sk;
            if (RG > 1 && M > 0) {   // circle rows of this stage: own rows first, then the other lanes' sums in lane order
                double c0 = ls.cp[0], c1 = ls.cp[1], c2 = ls.cp[2];
#pragma unroll
                for (int g = 0; g < RG - 1; g++) { c0 += ob[3 * g]; c1 += ob[3 * g + 1]; c2 += ob[3 * g + 2]; }
                rb[0] += c0; rb[1] += c1; rds -= c2;
            }
#pragma unroll
            for (int m = 0; m < (RG > 1 ? 0 : M); m++) {
                const double dx = xk[0] - ob[3 * m], dy = xk[1] - ob[3 * m + 1], m2 = dx * dx + dy * dy, id = mmpc_rsqrt(m2), d = m2 * id;
                const double nxv = dx * id, nyv = dy * id;
                const double h = (ob[3 * m + 2] + MMPC_BASE_R) - d - sk;
                const double t = ls.ct[m], z = ls.cz[m];
                rb[0] -= nxv * z; rb[1] -= nyv * z; rds -= z;
                e_p = mmpc_vmax(e_p, fabs(h + t)); th += fabs(h + t); la.mul(t);
                tzmax = mmpc_vmax(tzmax, t * z); tzmin = mmpc_vmin(tzmin, t * z); zsum += z;
            }
            if (NSELF) {
                double dr[3], dz[3];
                mmpc_arm_segments(xk[NX - 3], xk[NX - 2], xk[NX - 1], dr, dz);
                TRG[MMPC_MUL24(k, F::TRGS) + 0] = sn; TRG[MMPC_MUL24(k, F::TRGS) + 1] = cs;
#pragma unroll
                for (int a = 0; a < 3; a++) { TRG[MMPC_MUL24(k, F::TRGS) + 2 + a] = dr[a]; TRG[MMPC_MUL24(k, F::TRGS) + 5 + a] = dz[a]; }
                const double sks = sks_ld;
                double sw = 0.0, sit = 0.0, swr = 0.0, swg[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int i = 0; i < NSELF; i++) {
                    double g6[6];
                    const double h = mmpc_self_row(i, xk[0], xk[1], cs, sn, dr, dz, g6) - sks;
                    const double t = ls.st[i], z = ls.sz[i];
#pragma unroll
                    for (int a = 0; a < 6; a++) rb[mmpc_y(a)] += g6[a] * z;
                    selfz += z;
                    e_p = mmpc_vmax(e_p, fabs(h + t)); th += fabs(h + t); la.mul(t);
                    tzmax = mmpc_vmax(tzmax, t * z); tzmin = mmpc_vmin(tzmin, t * z); zsum += z;
                    if (k == N) {
                        const double it_ = mmpc_rcp(t), w = z * it_;
                        sw += w; sit += it_; swr += w * (h + t);
#pragma unroll
                        for (int a = 0; a < 6; a++) swg[a] += w * g6[a];
                    }
                }
                if (k == N) {   // terminal self rows belong to s_{N-1} (Q1): hand their sums to lane N-1
                    SN[0] = sw; SN[1] = sit; SN[2] = swr; SN[3] = selfz;
#pragma unroll
                    for (int a = 0; a < 6; a++) SN[4 + a] = swg[a];
                }
            }
            if (k < N) rds -= selfz;
            RDS[k] = rds;
#pragma unroll
            for (int j = 0; j < NV; j++) RB[MMPC_MUL24(k, NV) + j] = rb[j];
        }
        if (RG > 1 || lane < NS) slog = la.value();
        MMPC_WR(1) = e_p; MMPC_WR(2) = tzmax; MMPC_WR(3) = tzmin; MMPC_WR(4) = zsum; MMPC_WR(5) = phi; MMPC_WR(6) = th; MMPC_WR(7) = slog;
        MMPC_WR(8) = zeq;   // |multipliers of the dynamics|: s_d counts them, s_c does not
        if (NSELF == 0 && lane == 0) { for (int a = 0; a < 10; a++) SN[a] = 0.0; }
        LANES_END
        MMPC_TS(1)
        // ============================================================ E1 (pair lanes) + s residual
        LANES_BEGIN
        auto &ls = MMPC_LS;
        double e_d = 0.0, e_p = MMPC_WR(1), tzmax = MMPC_WR(2), tzmin = MMPC_WR(3), zsum = MMPC_WR(4), phi = MMPC_WR(5), th = MMPC_WR(6);
        MmpcLogAcc la; la.init();
        // long horizons read the references and the previous inputs from HBM / L2: the loads of ALL passes ahead of the loop (one
        // exposed round trip instead of one per pass)
        double g_ref[SLIM ? NPASS : 1], g_ul[SLIM ? NPASS : 1];
        static_assert(ENV::SLIM_MAP_OK, "the padded pair map is not written for the slim layout");
        if (SLIM) {
#pragma unroll
            for (int p = 0; p < NPASS; p++) {
                const int idx = lane + MMPC_WAVE * p, ii = idx < NPAIR ? idx : 0;
                const int k = ii / NV, v = ii % NV;
                const bool isu = v >= NX && k < N;
                g_ref[p] = ref_at(ii, k, v);
                g_ul[p] = ulast_at(isu ? k : 0, isu ? v - NX : 0);
            }
        }
        MMPC_PAIR_SETUP
        // padded map: the addresses of the previous input and of the cost weight as base + p * stride too (column < NX: state of
        // stage 4p+g, weight Q; NX <= column < NV: input, weights R and W, previous input of that stage; column NV: state 4p+g of the
        // terminal stage, weight P)
        const bool pu_ = F::PADMAP && pc_ >= NX && pc_ < NV;
        const int pul_b = pu_ ? pg_ * NU + pc_ - NX : 0, pul_s = pu_ ? 4 * NU : 0, pau_ = pu_ ? pc_ - NX : 0;
        const int pwq_b = pt_ ? MMPC_C_WP + pg_ : (pu_ ? MMPC_C_WR + pc_ - NX : MMPC_C_WQ + (pc_ < NX ? pc_ : 0)), pwq_s = pt_ ? 4 : 0;
        (void)pul_b; (void)pul_s; (void)pau_; (void)pwq_b; (void)pwq_s;
#pragma unroll
        for (int p = 0; p < NPASS; p++) {
            MMPC_PAIR(p)
            if (pok) {
                MMPC_PAIR_KV(p)
                const double lo = ls.b_lo[p], hi = ls.b_hi[p];
                const bool alo = lo > -1e299, ahi = hi < 1e299;
                // every LDS word this pair needs, ahead of the arithmetic and of the per-side blocks (one round trip per pass);
                // the input-only terms read a valid dummy address for state variables and carry weight 0 there
                const bool isu = F::PADMAP ? pu_ : (v >= NX && k < N);
                const int au = F::PADMAP ? pau_ : (isu ? v - NX : 0);
                const double val = XU[idx], ref = SLIM ? g_ref[SLIM ? p : 0] : ref_at(idx, k, v), rb0 = RB[idx];
                const double ul = SLIM ? g_ul[SLIM ? p : 0] : (F::PADMAP ? ULAST[pul_b + p * pul_s] : ulast_at(isu ? k : 0, au)), ww0 = CST[MMPC_C_WW + au];
                const double wq = CST[F::PADMAP ? pwq_b + p * pwq_s : (v < NX ? (k < N ? MMPC_C_WQ : MMPC_C_WP) + v : MMPC_C_WR + v - NX)];
                // cost gradient / value (diagonal weights): mpc_wholebody_qref.py:192-201,240-242
                double e = val - ref;
                if (KIND == 1 && v == 2) e = mmpc_angle_diff(val, ref);
                const double wqe = (F::PADMAP || v < NX || k < N) ? wq : 0.0, ww = isu ? ww0 : 0.0, e2 = val - ul;
                double g = wqe * e + ww * e2;
                phi += 0.5 * wqe * e * e + 0.5 * ww * e2 * e2;
                double r = rb0 + g;
                {   // both sides without branches: an absent side has z = 0 and is given t = 1 (log 1 = 0)
                    const double tl = alo ? mmpc_box_t(val - lo) : 1.0, zl = ls.lo_z[p], th_ = ahi ? mmpc_box_t(hi - val) : 1.0, zh = ls.hi_z[p];
                    const double pl = tl * zl, ph = th_ * zh;
                    r += zh - zl; la.mul(tl); la.mul(th_);
                    tzmax = mmpc_vmax(tzmax, mmpc_vmax(pl, ph));
                    tzmin = mmpc_vmin(tzmin, mmpc_vmin(alo ? pl : 1e300, ahi ? ph : 1e300));
                    zsum += zl + zh;
                }
                RB[idx] = g;   // keep the plain cost gradient for the assembly / directional derivative
                const bool isvar = F::PADMAP ? idx >= NX : (v < NX ? (k >= 1) : (k < N));   // (x_0 is data)
                if (isvar) e_d = mmpc_vmax(e_d, fabs(r));
            }
        }
        MMPC_WR(7) += la.value();   // sum of log t over all rows (the barrier term is applied after the mu update)
        if (lane < NS) e_d = mmpc_vmax(e_d, fabs(RDS[lane] - (lane == N - 1 ? SN[3] : 0.0)));
        MMPC_WR(0) = e_d; MMPC_WR(1) = e_p; MMPC_WR(2) = tzmax; MMPC_WR(3) = -tzmin; MMPC_WR(4) = zsum; MMPC_WR(5) = phi; MMPC_WR(6) = th;
        LANES_END
        // (four maxima - the smallest complementarity product as the largest of the negated ones - and four sums in one butterfly each)
        {
            double r4[4];
            MMPC_RED4_MAX(0, 1, 2, 3, r4);
            err_d = r4[0]; err_p = r4[1]; tzmax = r4[2]; tzmin = -r4[3];
            MMPC_RED4_SUM(4, 5, 6, 7, r4);
            zsum = r4[0]; cost_c = r4[1]; th_c = r4[2]; sumlog = r4[3];
        }
        const double zeq_c = MMPC_RED_SUM(8);
        if (in_ls) {
            // ---- filter test of the trial point just evaluated (Waechter-Biegler; + filter reset heuristic)
            const double phi = cost_c - mu * sumlog, th = th_c;
            bool okf = th < th_max;
            for (int i = 0; i < nfilt && okf; i++) if (th >= FILT[2 * i] && phi >= FILT[2 * i + 1]) okf = false;
#if MMPC_ITER_SOC
            const double a_t = soc_st == 2 ? alpha0 : alpha;   // (a corrected step is tested with the length of the step it corrects)
#else
            const double a_t = alpha;
#endif
            const bool ftype = dphi < 0 && th0 <= th_min && a_t * mmpc_powf(-dphi, 2.3f) > mmpc_powf(th0, 1.1f);
            bool accepted = false, augment = false;
            if (okf) {
                if (ftype) accepted = phi <= phi0 + 1e-8 * a_t * dphi + 1e-14 * fabs(phi0);
                else if (th <= (1 - 1e-5) * th0 || phi <= phi0 - 1e-5 * th0) { accepted = true; augment = true; }
            }
            if (augment) {
                int slot = nfilt;
                if (nfilt >= MMPC_FCAP) { slot = 0; for (int i = 1; i < MMPC_FCAP; i++) if (FILT[2 * i] > FILT[2 * slot]) slot = i; }
                else nfilt++;
                LANES_BEGIN
                if (lane == 0) { FILT[2 * slot] = (1 - 1e-5) * th0; FILT[2 * slot + 1] = phi0 - 1e-5 * th0; }
                LANES_END
            }
#if MMPC_ITER_SOC
            if (soc_st == 2) {
                if (accepted) { soc_st = 0; alpha = a_soc; }
                else if (th > 0.99 * th_prev || soc_p + 1 >= MMPC_SOC_MAX) {
                    // the correction failed: back to x_k, the uncorrected direction restored, evaluated there again (state 3)
                    apply_step(-a_soc, false);
                    soc_dir(false);
                    soc_st = 3; in_ls = 0;
                    continue;
                } else {
                    soc_rows(false, false);
                    apply_step(-a_soc, false);
                    soc_p++; a_prev = a_soc; th_prev = th; soc_st = 1; in_ls = 0;
                    continue;
                }
            }
#else
            if (__builtin_expect(!accepted && MMPC_SOC_MAX > 0 && lsi == 0 && lspass == 0 && io.soc && th >= th0 && th0 <= th_min, 0)) {
                // first trial rejected without reducing the infeasibility, theta(x_k) <= theta_min: second-order correction - in the
                // second copy of the loop (below), which alone carries its code
                th_prev = th; soc_enter = true;
                break;
            }
#endif
            if (!accepted) {
                double anext = alpha;
                bool retry = false;
                if (lsi < MMPC_MAX_LS - 1) { anext = 0.5 * alpha; lsi++; retry = true; }
                else if (lspass == 0 && nfilt > 0) { nfilt = 0; lspass = 1; lsi = 0; anext = ap; retry = true; }   // filter reset heuristic
                if (retry) { apply_step(anext - alpha, false); alpha = anext; continue; }
            }
            in_ls = 0;   // accepted (or every trial rejected: the last one is kept, as IPOPT without restoration would stall too)
            mmpc_prox_update(ap, alpha, prox, nsmall);
            MMPC_TS(12)
#if MMPC_ITER_SOC
            break;   // the corrected step is accepted: on in the regular copy of the loop, which evaluates the point once more (every
                     // regular iteration runs in ONE copy of the code: a solve cut into launches by an iteration budget stays bitwise
                     // what the uninterrupted solve computes)
#endif
        }
#if MMPC_ITER_SOC
        if (soc_st == 1) soc_rows(true, soc_p == 0);
#else
        {
        // IPOPT's termination test (Waechter & Biegler 2006, eq. 5-6): stationarity over s_d (all multipliers), complementarity over
        // s_c (the row multipliers alone)
        double sd = (zsum + zeq_c) * inv_rows, sc = zsum * inv_nrows;
        sd = (sd > 100.0 ? sd : 100.0) * 0.01;
        sc = (sc > 100.0 ? sc : 100.0) * 0.01;
        const double isd = mmpc_rcp(sd), isc = mmpc_rcp(sc);
        E0 = mmpc_vmax(mmpc_vmax(err_d * isd, err_p), tzmax * isc);
        if (!mmpc_finite(E0) || !mmpc_finite(th_c + cost_c + zsum + zeq_c)) {   // NaN or inf anywhere in the point or its data (the sums carry them)
#ifdef MMPC_EMU_DEBUG
            fprintf(stderr, "E0 nan it %d: err_d %g err_p %g tzmax %g tzmin %g zsum %g sumlog %g\n", it, err_d, err_p, tzmax, tzmin, zsum, sumlog);
#endif
            status = 2; MMPC_ITER_LEAVE }
        if (E0 <= tol) { status = 0; MMPC_ITER_LEAVE }
        if (it == P.max_iter) MMPC_ITER_LEAVE
        if (CONT && io.budget > 0 && it - it_start >= io.budget && io.state) {
            // ---- iteration budget of this launch used up: park the solve (the point has just been evaluated and is not
            //      converged; a resumed launch re-evaluates it and continues with the barrier update below)
            double *const st_xu = io.state, *const st_s = io.state + ST_S, *const st_lam = io.state + ST_LAM,
                   *const st_filt = io.state + ST_FILT, *const st_scal = io.state + ST_SCAL, *const st_lane = io.state + ST_LANE;
            LANES_BEGIN
            auto &ls = MMPC_LS;
            for (int i = lane; i < NPAIR; i += MMPC_WAVE) st_xu[i] = XU[i];
            for (int i = lane; i < NS; i += MMPC_WAVE) st_s[i] = S[i];
            for (int i = lane; i < NS * NX; i += MMPC_WAVE) st_lam[i] = LAM[i];
            for (int i = lane; i < 2 * MMPC_FCAP; i += MMPC_WAVE) st_filt[i] = i < 2 * nfilt ? FILT[i] : 0.0;
            double *q = st_lane + lane * NLREG;
#pragma unroll
            for (int p = 0; p < NPASS; p++) { q[p] = ls.lo_z[p]; q[NPASS + p] = ls.hi_z[p]; }
#pragma unroll
            for (int m = 0; m < MCR; m++) { q[2 * NPASS + m] = ls.ct[m]; q[2 * NPASS + MCS + m] = ls.cz[m]; }
#pragma unroll
            for (int i = 0; i < 4; i++) { q[2 * NPASS + 2 * MCS + i] = ls.st[i]; q[2 * NPASS + 2 * MCS + 4 + i] = ls.sz[i]; }
            if (lane == 0) {
                st_scal[0] = mu; st_scal[1] = th_max; st_scal[2] = th_min; st_scal[3] = prox;
                st_scal[4] = (double)it; st_scal[5] = (double)nfilt; st_scal[6] = (double)filt_init; st_scal[7] = (double)nsmall; st_scal[8] = delta_last; st_scal[9] = delta_prev;
                st_scal[10] = CST[MMPC_C_SCALE];   // (objective scaling: the factor of this solve, read back by its continuation)
            }
            LANES_END
            status = 3;   // MMPC_STATUS_SUSPENDED
            MMPC_ITER_LEAVE
        }
        {
            bool changed = false;
            for (;;) {
                const double compmu = mmpc_vmax(fabs(tzmax - mu), fabs(tzmin - mu));
                const double Emu = mmpc_vmax(mmpc_vmax(err_d * isd, err_p), compmu * isc);
                if (!(Emu <= 10.0 * mu && mu > tol / 10)) break;
                mu = mmpc_vmax(tol / 10, mmpc_vmin(0.2 * mu, mu * sqrt(mu)));
                changed = true;
            }
            if (changed) filt_init = 0;
        }
        phi0 = cost_c - mu * sumlog;   // barrier objective at the current point for the (possibly new) mu
        th0 = th_c;
        }
#endif

        MMPC_TS(2)
        // ============================================================ Newton direction
        int failed = 0;
        double dw = delta_prev > MMPC_IC_SKIP0 ? mmpc_vmax(1e-20, MMPC_IC_DN * delta_last) : 0.0;   // (see MMPC_IC_SKIP0)
#if MMPC_ITER_SOC
        if (soc_st != 3)   // (after a failed correction only the row steps D2 are formed again: the direction is back from io.soc)
#endif
        {
#pragma unroll 1
        // (exact Lagrangian Hessian, + delta_w I by IPOPT's inertia correction where a pivot of the recursion is not positive - see mmpc_core.h)
        for (;;) {
            // (always true.  Kept a run-time value on purpose: as a compile-time constant the curvature terms of the circle rows
            //  join the basic blocks around them, the scheduler moves their loads up and the kernel spills 76 instead of 44
            //  vector registers - the branch the old Hessian ladder needed is the cheaper of the two)
            const bool exact = P.max_iter >= 0;
            constexpr bool dyn_curv = true;
            const double reg = prox + dw;
            int ric_bad = 0;   // a pivot of this pass was not positive (every lane factorises the same matrix: uniform)
            // ---- A1 (circle rows where RG lanes share a stage): w g g^T (+ exact curvature), gradient and s_k coupling of the
            //      lane's rows: cp = (Hxx, Hxy, Hyy, qx, qy, h_ss, g_ss, vx, vy)
            {
            constexpr bool socm = MMPC_ITER_SOC != 0; (void)socm;   // (the second copy of the loop only assembles corrected passes)
#include "mmpc_fast_a1r.inc"
            }
            // ---- A1 (stage lanes): stage Hessian incl. elimination of s_k
            {
            constexpr bool socm = MMPC_ITER_SOC != 0; (void)socm;   // (the second copy of the loop only assembles corrected passes)
#include "mmpc_fast_a1s.inc"
            }
            if (NSELF) {
                // ---- dense rank-one blocks of stage N-1 (the elimination of s_{N-1} reaches x_N through the dynamics):
                //      Hxx -= a a^T/h, Hux = -b a^T/h, Huu = -b b^T/h, q += (a; b) gamma/h
                //      One item per (lane, slot): which two words of Q1V, where to, accumulate or set - decoded once per solve into
                //      ls.q1d (the triangular index decode and the four-way branch of the item loop ran in every backward pass:
                //      ~400 instructions and eight LDS round trips for 119 products).
                LANES_BEGIN
                auto &ls = MMPC_LS;
                const double nih = -Q1V[NV + 1];
#pragma unroll
                for (int t = 0; t < 2; t++) {
                    const unsigned d = ls.q1d[t];
                    double *dst = lds + (d >> 12);
                    const double a = Q1V[d & 31u], b = Q1V[(d >> 5) & 31u], old = *dst;
                    const double base = (d & 1024u) ? old : 0.0;
                    // (gradient items: q_j gamma / h as one fma; block items: -(q_i q_j) / h)
                    *dst = (d & 2048u) ? fma(a, b, base) : fma(nih, a * b, base);
                }
                LANES_END
            }
            MMPC_TS(3)
            // ---- A1 (pair lanes): barrier terms of the box rows (diagonal entries, unique owners)
            LANES_BEGIN
            auto &ls = MMPC_LS;
            MMPC_PAIR_SETUP
            // padded map: the diagonal entry's address as base + p * stride (+ the part of the terminal states' packed index that is
            // quadratic in the pass: e(v) = v (v + 3) / 2 with v = 4p + g is e(g) + 4 g p + 8 p^2 + 6 p)
            const bool pu_ = F::PADMAP && pc_ >= NX && pc_ < NV;
            const int pvs_ = pc_ < NX ? pc_ : 0;
            const int phd_b = pt_ ? L.HXX + N * NXX + pg_ * (pg_ + 3) / 2 : (pu_ ? L.HUUD + pg_ * NU + pc_ - NX : L.HXX + pg_ * NXX + pvs_ * (pvs_ + 3) / 2),
                      phd_s = pt_ ? 4 * pg_ : (pu_ ? 4 * NU : 4 * NXX);
            (void)phd_b; (void)phd_s;
#pragma unroll
            for (int p = 0; p < NPASS; p++) {
                MMPC_PAIR(p)
                if (pok) {
                    MMPC_PAIR_KV(p)
                    const double lo = ls.b_lo[p], hi = ls.b_hi[p];
                    const bool alo = lo > -1e299, ahi = hi < 1e299;
                    // the diagonal Hessian entry this pair owns (state: HXX[k] diagonal, input: HUUD[k]); loads first
                    double *hd = F::PADMAP ? lds + (phd_b + p * phd_s + (pt_ ? 8 * p * p + 6 * p : 0))
                                           : (v < NX ? HXX + k * NXX + v * (v + 1) / 2 + v : HUUD + (k < N ? k : 0) * NU + v - NX);
                    const double val = XU[idx], q0 = QXU[idx], h0 = *hd;
                    double wsum = 0.0, gsum = 0.0;
                    if (alo) { const double it_ = mmpc_rcp(mmpc_box_t(val - lo)); wsum += ls.lo_z[p] * it_; gsum -= mu * it_; }
                    if (ahi) { const double it_ = mmpc_rcp(mmpc_box_t(hi - val)); wsum += ls.hi_z[p] * it_; gsum += mu * it_; }
                    if (alo || ahi) { QXU[idx] = q0 + gsum; *hd = h0 + wsum; }
                }
            }
            LANES_END
            MMPC_TS(4)
            // ---- R0: terminal cost-to-go [P_N p_N; p_N^T .] = stage-N Hessian and gradient, in accumulator layout;
            //      operands of stage N-1: rAB = homogeneous dynamics rows 4r+g, rM = stage matrix (accumulator input)
            LANES_BEGIN
            auto &ls = MMPC_LS;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const unsigned o = ls.h_o[r];
                ls.rP[r] = ((ls.h_m >> r) & 1u) ? lds[(o & 0xffffu) + N * (int)(o >> 16)] : 0.0;
                ls.rM[r] = lds[(o & 0xffffu) + (N - 1) * (int)(o >> 16)] + lds[ls.h_l[r]];
            }
#pragma unroll
            for (int r = 0; r < NKB; r++) { const unsigned o = ls.ab_o[r]; ls.rAB[r] = lds[(o & 0xffffu) + (N - 1) * (int)(o >> 16)]; }
#pragma unroll
            for (int q = 0; q < 4; q++) ls.mg[q] = (lane >> 4) == q ? 1.0 : 0.0;   // lane-group masks of the elimination legs
            LANES_END
#pragma unroll RIC_UNROLL
            for (int k = N - 1; k >= 0; k--) {
                MMPC_TSF(5)
                if (ric_bad) break;   // (uniform: every lane factorises the same matrix) the pass is redone with a (larger) inertia correction
                // R1: T = [P p; p^T .] [A B c; 0 0 1]   (symmetric: its accumulator registers are the A operand; the affine
                // part rides along as row / column NX, so the chain starts from a zero accumulator)
                MMPC_MFMA0(rT, ls.rP[0], ls.rAB[0])
                MMPC_MFMA(rT, ls.rP[1], ls.rAB[1])
                if (NKB > 2) MMPC_MFMA(rT, ls.rP[NKB > 2 ? 2 : 0], ls.rAB[NKB > 2 ? 2 : 0])
                // R2: M = [A B c; 0 0 1]^T T + stage matrix  ->  [F gx G^T; gx^T . gu^T; G gu Hh]
                MMPC_MFMA(rM, ls.rAB[0], ls.rT[0])
                MMPC_MFMA(rM, ls.rAB[1], ls.rT[1])
                if (NKB > 2) MMPC_MFMA(rM, ls.rAB[NKB > 2 ? 2 : 0], ls.rT[NKB > 2 ? 2 : 0])
                MMPC_TSF(6)
#define MMPC_NEXT_OPERANDS                                                                                                         \
                LANES_BEGIN_NL                                                                                                             \
                auto &ls = MMPC_LS;                                                                                                        \
                if (k > 0) {                                                                                                               \
                    _Pragma("unroll")                                                                                                      \
                    for (int r = 0; r < NKB; r++) { const unsigned o = ls.ab_o[r]; ls.nab[r] = lds[(o & 0xffffu) + (k - 1) * (int)(o >> 16)]; }   \
                    _Pragma("unroll")                                                                                                      \
                    for (int r = 0; r < 4; r++) { const unsigned o = ls.h_o[r]; ls.nhm[r] = lds[(o & 0xffffu) + (k - 1) * (int)(o >> 16)]; }     \
                }                                                                                                                          \
                LANES_END_REG
                // R3: the inputs are eliminated ON the tile (block L D L^T = Schur complement).  For input a with pivot row
                // c = M[NX+1+a][.] and pivot d = c[NX+1+a] > 0,  M <- M - c c^T / d  is one rank-one MFMA whose only non-zero
                // K-slot is supplied by the lane group that already holds the row in its accumulator (row index mod 4 = lane
                // group = K-slot: no LDS exchange).  Two inputs whose rows sit in neighbouring lane groups of the same
                // accumulator register go together (one MFMA with two K-slots: the serial chain accumulator -> pivot ->
                // reciprocal -> MFMA is what a stage costs): M <- M - c0 c0^T / d0 - c1' c1'^T / d1 with c1' = c1 - (d01/d0) c0,
                // the second group fetching its partner's row entry from lane ^ 16.  What is left in rows / columns (x, 1) after the
                // last input is [P_k p_k; p_k^T .].  The normalised rows c / d are kept: u_a = -(c/d) . (dx, 1,
                // u_b>a), from which the gains are formed for all stages at once after the pass.
                constexpr bool PAIRS = F::PAIRS;                          // first input row even -> rows (2q, 2q+1) share a register
                constexpr int NLEG = F::NLEG;
                // A stage is 9 products of 64 cycles - during which this wave issues no other vector instruction (measured, round 4: eight
                // independent v_fma_f64 behind a leg's product cost what they cost in front of it; only LDS and scalar instructions
                // overlap) - plus its vector instructions at ~4 cycles each, ~8 when they depend on the one before.  So a leg is written
                // for few instructions and short chains: the lane-group selects are arithmetic on the 0 / 1 masks mg[q] = (lane group
                // == q): -w = c (-(1/d0) mg[ga] - (1/d1) mg[ga+1]) is zero outside the pivot rows' groups, which makes the K-slots of the
                // other groups vanish whatever their B operand is, so that operand is the plain register; the partner's row entry comes
                // from v_permlane16_swap without the select of a full xor-16 exchange (the second row of a pair sits in an odd row of 16
                // lanes); -w itself is what is stored for the gains (no sign flip on either side).
#pragma unroll
                for (int leg = 0; leg < NLEG; leg++) {
                    const int a0 = PAIRS ? 2 * leg : leg;
                    const bool pair = PAIRS && a0 + 1 < NU;
                    const int ta = NX + 1 + a0, ra = ta >> 2, ga = ta & 3;
                    LANES_BEGIN_NL
                    auto &ls = MMPC_LS;
                    const double c = ls.rM[ra];
                    if (pair) {
                        const double d00 = MMPC_LANE_GET(rM[ra], 16 * ga + ta), d01 = MMPC_LANE_GET(rM[ra], 16 * ga + ta + 1),
                                     d11 = MMPC_LANE_GET(rM[ra], 16 * (ga + 1) + ta + 1);
                        const double co = MMPC_LANE_LOWER16(rM[ra]);
#if MMPC_LEG_DET
                        // both pivots' reciprocals side by side: 1/d0, and 1/d1 = d0 / (d0 d11 - d01^2) from the 2 x 2 determinant (the
                        // sequential form d1 = d11 - (d01/d0) d01 puts reciprocal -> refinement -> multiply -> fma -> reciprocal ->
                        // refinement in a row; the determinant's rounding, eps d0 d11 against d0 d1, is that of the sequential d1)
                        const double det = fma(-d01, d01, d00 * d11), n1 = -(d00 * ls.mg[ga + 1]);
                        double i0 = mmpc_rcp_piv(d00), rdet = mmpc_rcp_piv(det);
                        const double l = d01 * i0;
                        const double cb = fma(-l * ls.mg[ga + 1], co, c);
                        const double wn = cb * fma(rdet, n1, -(i0 * ls.mg[ga]));
                        ls.pv0 = d00; ls.pv1 = det;
#else
                        const double i0 = mmpc_rcp_piv(d00), l = d01 * i0, d1 = fma(-l, d01, d11), i1 = mmpc_rcp_piv(d1);
                        const double cb = fma(-l * ls.mg[ga + 1], co, c);
                        const double wn = cb * fma(-i1, ls.mg[ga + 1], -i0 * ls.mg[ga]);
                        ls.pv0 = d00; ls.pv1 = d1;
#endif
                        ls.opa = wn;
                        ls.opb = cb;
                    } else {
                        const double d = MMPC_LANE_GET(rM[ra], 16 * ga + ta);
                        const double wn = c * (-mmpc_rcp_piv(d) * ls.mg[ga]);
                        ls.opa = wn;
                        ls.opb = c;
                        ls.pv0 = d; ls.pv1 = d;
                    }
                    LANES_END_REG
                    MMPC_MFMA(rM, ls.opa, ls.opb)
                    // operands of the next stage travel while this one eliminates its inputs: issued behind the first leg's product
                    if (leg == 0) { MMPC_NEXT_OPERANDS }
                    LANES_BEGIN_NL
                    auto &ls = MMPC_LS;
                    if (!(ls.pv0 > 0.0 && ls.pv1 > 0.0)) ric_bad = 1;   // (NaN fails too) the pass stops at the next stage and is redone with a (larger) inertia correction
                    // (lanes that hold no entry of the row write to their dump slot - no branch; in the gain block of the long horizons a
                    //  masked store - exec handling on the chain of every leg - measured 300 k against 314 k solves/s on C5, for 10 % less
                    //  write traffic out of L2)
                    *(double *)((char *)KBASE + (unsigned)(ls.kl_b[leg] + MMPC_MUL24(k, ls.kl_s[leg]))) = ls.opa;   // (-w: see the gains below)
                    LANES_END_REG
                }
#undef MMPC_NEXT_OPERANDS
                MMPC_TSF(7)
                LANES_BEGIN_NL
                auto &ls = MMPC_LS;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    ls.rP[r] = ls.rM[r];
                    const unsigned o = ls.p_o[r];   // (entries that are not stored go to a dump slot: no branch)
                    lds[(o & 0xffffu) + k * (int)(o >> 16)] = ls.rM[r];
                    ls.rM[r] = ls.nhm[r];
                }
#pragma unroll
                for (int r = 0; r < NKB; r++) ls.rAB[r] = ls.nab[r];
                LANES_END
            }
            if (ric_bad) failed = 1;
            if (!failed) {
                if (dw > 0.0) delta_last = dw;
#if !MMPC_ITER_SOC
                delta_prev = dw;
#endif
                break;
            }
            dw = dw == 0.0 ? (delta_last == 0.0 ? MMPC_IC_D0 : mmpc_vmax(1e-20, MMPC_IC_DN * delta_last)) : MMPC_IC_UP * dw;
            if (dw > 1e40) break;
            failed = 0;
        }
        if (failed) {
#ifdef MMPC_EMU_DEBUG
            fprintf(stderr, "riccati failed twice it %d\n", it);
#endif
            status = 2; fatal = 1; }
        if (!fatal) {
        // ---- gains of all stages from the normalised pivot rows, by back-substitution over the inputs (the last eliminated
        //      input depends on x only): K_a = -(w_a[x,1] + sum_{b>a} w_a[u_b] K_b), in place, one lane per (stage, column).  The legs
        //      stored s = -w (the product's operand as it stands): K_a = s_a[x,1] + sum_{b>a} s_a[u_b] K_b - the same bits, no negations
        // (Long horizons: the legs' stores to the gain block in global memory are read here by other lanes of the SAME wave.  The vector
        //  memory instructions of a wavefront are issued and processed in order, so the wavefront-scope fence of LANES_END (compiler
        //  ordering only, no s_waitcnt) is all that is needed, here and after the back-substitution - waiting for the stores'
        //  acknowledgement with a workgroup-scope fence cost 2 x ~1 k cycles per iteration.)
        LANES_BEGIN
        if constexpr (!GK && NX + 1 <= 16) {
            // gains in LDS: a row of 16 lanes takes one stage per trip, the lane's column is the column of [K_k | kf_k] (stage 4 t + lane / 16,
            // column lane % 16 <= NX): every address is base(lane) + constant - no division per item
            const int g = lane >> 4, c = lane & 15;
            const bool col = c <= NX;
            constexpr int NTRIP = (N + 3) / 4;
            const int kb = MMPC_MUL24(g, NU * KS) + (col ? c : 0), ub = MMPC_MUL24(g, NPU);   // word of stage g, input 0 in the lane's column; couplings of stage g
            double kv[NTRIP][NU], cu[NTRIP][NPU > 0 ? NPU : 1];
#pragma unroll
            for (int t = 0; t < NTRIP; t++) {
                const bool in = 4 * (t + 1) <= N || 4 * t + g < N;   // (only the last trip of a horizon that is no multiple of 4 has rows without a stage)
                const int kt = in ? kb + t * 4 * NU * KS : 0, ut = in ? ub + t * 4 * NPU : 0;
#pragma unroll
                for (int a = 0; a < NU; a++) kv[t][a] = KK[kt + a * KS];
#pragma unroll
                for (int q = 0; q < NPU; q++) cu[t][q] = KU[ut + q];
            }
#pragma unroll
            for (int t = 0; t < NTRIP; t++) {
#pragma unroll
                for (int a = NU - 1; a >= 0; a--) {
                    double v = kv[t][a];
#pragma unroll
                    for (int b2 = a + 1; b2 < NU; b2++) v += cu[t][a * (2 * NU - a - 1) / 2 + (b2 - a - 1)] * kv[t][b2];
                    kv[t][a] = v;
                }
                if (col && (4 * (t + 1) <= N || 4 * t + g < N)) {
#pragma unroll
                    for (int a = 0; a < NU; a++) KK[kb + t * 4 * NU * KS + a * KS] = kv[t][a];
                }
            }
        } else
        {
            // two (stage, column) items per lane at a time, the loads of both ahead of the arithmetic: the update is in place, so the
            // compiler cannot move the loads of one item above the stores of the one before
            constexpr int NITEM = N * (NX + 1), NTRIP = (NITEM + MMPC_WAVE - 1) / MMPC_WAVE;
            // entry (stage, input, column) of [K_k | kf_k]; in the gain block one access with a selected offset (a select between two
            // global accesses becomes a branch per access)
            auto kref = [&](int kq, int a, int jq) -> double & {
                if constexpr (GK) return gk(io.gscr, jq < NX ? GB::KK + (kq * NU + a) * NX + jq : GB::KF + kq * NU + a);
                else return KK[(kq * NU + a) * KS + jq];
            };
            // (gain block in global memory: the loads of half of the lane's items ahead of their arithmetic - two exposed round trips to L2
            //  instead of one per pair of items)
            constexpr int TSTEP = GK ? (NTRIP + 1) / 2 : 2;
#pragma unroll
            for (int t0 = 0; t0 < NTRIP; t0 += TSTEP) {
                double kv[TSTEP][NU], cu[TSTEP][NPU > 0 ? NPU : 1];
                int kk[TSTEP], jj[TSTEP];
                bool ok[TSTEP];
#pragma unroll
                for (int u = 0; u < TSTEP; u++) {
                    const int i = lane + MMPC_WAVE * (t0 + u);
                    ok[u] = t0 + u < NTRIP && i < NITEM;
                    const int ii = ok[u] ? i : 0;
                    kk[u] = ii / (NX + 1); jj[u] = ii % (NX + 1);
#pragma unroll
                    for (int a = 0; a < NU; a++) kv[u][a] = kref(kk[u], a, jj[u]);
#pragma unroll
                    for (int q = 0; q < NPU; q++) cu[u][q] = gk(KU, kk[u] * NPU + q);
                }
#pragma unroll
                for (int u = 0; u < TSTEP; u++) {
#pragma unroll
                    for (int a = NU - 1; a >= 0; a--) {
                        double v = kv[u][a];
#pragma unroll
                        for (int b2 = a + 1; b2 < NU; b2++) v += cu[u][a * (2 * NU - a - 1) / 2 + (b2 - a - 1)] * kv[u][b2];
                        kv[u][a] = v;
                    }
                }
#pragma unroll
                for (int u = 0; u < TSTEP; u++) {
                    if (ok[u]) {
#pragma unroll
                        for (int a = 0; a < NU; a++) kref(kk[u], a, jj[u]) = kv[u][a];
                    }
                }
            }
        }
        LANES_END
        MMPC_TS(8)
        // ---- forward roll-out: lane i < NX carries dx_k[i] in a register; a stage broadcasts the NX values through scalar
        //      registers (v_readlane), forms the input step of its row and the next dx - no LDS round trip on the chain.
        //      The operands of a stage (gain row, coefficients) do not depend on the chain and are fetched one stage ahead;
        //      dx and du are stored for the phases that follow, nothing in the loop reads them back.
        {
            double nkr[NX], nkf = 0.0, nc0 = 0.0, ncf[5];
            LANES_BEGIN
            auto &ls = MMPC_LS;
            for (int j = lane; j < NV; j += MMPC_WAVE) DXU[j] = 0.0;
            ls.fw[MMPC_FW_SLOT(0)] = 0.0;
            {   // (lanes that own no row / no input write to their dump slot: no branch in the loop)
                const int a = (int)MMPC_B(ls.f_x, 2) - 1;
                ls.fw_a[0] = lane < NX ? L.DXU + NV + lane : L.DUMP + lane;
                ls.fw_a[1] = (lane < NX && a >= 0 && lane != 4) ? L.DXU + NX + a : L.DUMP + lane;
                ls.fw_a[2] = lane < NX ? NV : 0;
                ls.fw_a[3] = lane < NX ? lane : 0;        // row of the dynamics this lane carries
                ls.fw_a[4] = a < 0 ? 0 : a;               // the input that enters this row
            }
            LANES_END
#ifndef MMPC_EMU
            // Gains in global memory (GK): lane l < GRS carries element l of a stage's (K_k, kf_k).  A ring of four stage slots in
            // LDS - over the stage-matrix extras HUXL .. HUUD, dead since the backward pass - is filled two stages ahead of the
            // chain from registers that were loaded from the gain block three stages before that; the row lanes read their gain
            // row from the ring one stage ahead, as they read it from the LDS copy of the short horizons.
            constexpr int GRS = ENV::GRS;
            static_assert(ENV::RING_FITS, "the gain ring must fit the stage-matrix extras");
            static_assert(ENV::RING_UNROLLED, "the gain ring's registers rotate statically: the roll-out must be fully unrolled");
            double *const RING = lds + L.HUXL;
            double gpre[3] = {0.0, 0.0, 0.0};
            unsigned g_off = 0, g_st = 0;
            int r_off = 0, r_st = 0;
            auto gload = [&](int stage) -> double { return *(const double *)((const char *)io.gscr + (size_t)(g_off + (unsigned)stage * g_st)); };
            if (GK) {
                const int lane = mmpc_lane_id();
                const bool isk = lane < NU * NX, isf = !isk && lane < GRS;
                g_off = (unsigned)(isk ? GB::KK + lane : (isf ? GB::KF + lane - NU * NX : GB::DUMP + lane)) * 8u;
                g_st = isk ? (unsigned)(NU * NX) * 8u : (isf ? (unsigned)NU * 8u : 0u);
                r_off = lane < GRS ? L.HUXL + lane : L.DUMP + lane;
                r_st = lane < GRS ? GRS : 0;
                const double e0 = gload(0), e1 = N > 1 ? gload(1) : 0.0;
#pragma unroll
                for (int q = 0; q < 3; q++) if (q + 2 < N) gpre[q] = gload(q + 2);
                lds[r_off] = e0; lds[r_off + r_st] = e1;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
            {   // operands of stage 0
                const int lane = mmpc_lane_id();
                auto &ls = MMPC_LS;
                const int i = lane < NX ? lane : 0, a = (int)MMPC_B(ls.f_x, 2) - 1, aa = a < 0 ? 0 : a;
#pragma unroll
                for (int j = 0; j < NX; j++) nkr[j] = GK ? RING[aa * NX + j] : KK[aa * KS + j];
                nkf = GK ? RING[NU * NX + aa] : KF[aa * KFS]; nc0 = CD[i];
#pragma unroll
                for (int q = 0; q < 4; q++) ncf[q] = CV[MMPC_B(ls.f_v, q)];
                ncf[4] = CV[MMPC_B(ls.f_x, 1)];
            }
#endif
#pragma unroll FWD_UNROLL
            for (int k = 0; k < N; k++) {
                LANES_BEGIN_NL
                auto &ls = MMPC_LS;
                const int i = ls.fw_a[3], aa = ls.fw_a[4];
                const int fw_dx = ls.fw_a[0], fw_du = ls.fw_a[1], fw_st = ls.fw_a[2];
                double kr[NX], cf[5], kf0, c0;
#ifdef MMPC_EMU
                {
                    const double *cv = CV + k * MMPC_NCV;
                    for (int j = 0; j < NX; j++) kr[j] = KK[(k * NU + aa) * KS + j];
                    kf0 = KF[(k * NU + aa) * KFS]; c0 = CD[k * NX + i];
                    for (int q = 0; q < 4; q++) cf[q] = cv[MMPC_B(ls.f_v, q)];
                    cf[4] = cv[MMPC_B(ls.f_x, 1)];
                }
#else
#pragma unroll
                for (int j = 0; j < NX; j++) kr[j] = nkr[j];
                kf0 = nkf; c0 = nc0;
#pragma unroll
                for (int q = 0; q < 5; q++) cf[q] = ncf[q];
                if (k + 1 < N) {
                    const double *cv = CV + (k + 1) * MMPC_NCV;
#pragma unroll
                    for (int j = 0; j < NX; j++) nkr[j] = GK ? RING[((k + 1) & 3) * GRS + aa * NX + j] : KK[((k + 1) * NU + aa) * KS + j];
                    nkf = GK ? RING[((k + 1) & 3) * GRS + NU * NX + aa] : KF[((k + 1) * NU + aa) * KFS]; nc0 = CD[(k + 1) * NX + i];
#pragma unroll
                    for (int q = 0; q < 4; q++) ncf[q] = cv[MMPC_B(ls.f_v, q)];
                    ncf[4] = cv[MMPC_B(ls.f_x, 1)];
                }
                if (GK) {
                    if (k + 2 < N) {
                        lds[r_off + ((k + 2) & 3) * r_st] = gpre[k % 3];
                        // other lanes read this slot two stages on: ordering for the compiler (no instruction; the LDS unit processes a
                        // wave's accesses in issue order)
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    }
                    if (k + 5 < N) gpre[k % 3] = gload(k + 5);
                }
#endif
                double dx[NX];
#ifndef MMPC_EMU
                // (the rows of the dynamics sit in lanes 0 .. NX-1, all in the first row of 16 lanes: dx_k[j] by a row broadcast; the
                //  other rows of the wave broadcast their own lanes' don't-care values and store to their dump slots)
                static_assert(ENV::ROLL_ROW_OK, "the roll-out's row lanes must share a row of 16 lanes");
                mmpc_rowbcast_all<0, NX>(ls.fw[MMPC_FW_SLOT(k)], dx);
#else
#pragma unroll
                for (int j = 0; j < NX; j++) dx[j] = MMPC_LANE_GET(fw[MMPC_FW_SLOT(k)], j);
#endif
                // du_a = kf_a + K_a dx in three partial sums; the terms of dx+ that do not need du meanwhile
                double d0 = kf0, d1 = 0.0, d2 = 0.0;
#pragma unroll
                for (int j = 0; j < NX; j += 3) {
                    d0 += kr[j] * dx[j];
                    if (j + 1 < NX) d1 += kr[j + 1] * dx[j + 1];
                    if (j + 2 < NX) d2 += kr[j + 2] * dx[j + 2];
                }
                double v = c0 + ls.fw[MMPC_FW_SLOT(k)];
                double w = cf[0] * dx[2];
                v += cf[1] * dx[3];
                w += cf[2] * dx[4];
                v += cf[3] * dx[5];
                const double du = d0 + (d1 + d2);
                v = (v + w) + cf[4] * du;
                ls.fw[MMPC_FW_SLOT(k + 1)] = v;
                // (lanes that own no row / no input write to their dump slot: no branch)
                lds[fw_du + k * fw_st] = du;
                lds[fw_dx + k * fw_st] = v;
                LANES_END_REG
            }
            LANES_BEGIN
            LANES_END
        }
        MMPC_TS(9)
        // ---- D1: multiplier step and slack-variable step (stage lanes)
        LANES_BEGIN
        auto &ls = MMPC_LS;
        if (lane < NS) {
            const int k = lane;
            // lam_k + dlam_k = -(P_k dx_k + p_k): every load ahead of the arithmetic, the stores at the end (a store inside the
            // row loop makes the compiler wait for each load: it cannot tell DLAM from HXX)
            double dx[NX], pk[NXX], y[NX];
#pragma unroll
            for (int j = 0; j < NX; j++) { dx[j] = DXU[MMPC_MUL24(k, NV) + j]; y[j] = QXU[MMPC_MUL24(k, NV) + j] + LAM[MMPC_MUL24(k, NX) + j]; }
#pragma unroll
            for (int e = 0; e < NXX; e++) pk[e] = HXX[MMPC_MUL24(k, NXX) + e];
#pragma unroll
            for (int i = 0; i < NX; i++) {
#pragma unroll
                for (int j = 0; j < NX; j++) y[i] += pk[i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i] * dx[j];
            }
#pragma unroll
            for (int i = 0; i < NX; i++) DLAM[MMPC_MUL24(k, NX) + i] = -y[i];
            double vdx = 0.0;
            constexpr int ny = NSELF ? 6 : 2;
#pragma unroll
            for (int a = 0; a < ny; a++) vdx += ls.vx[a] * dx[mmpc_y(a)];
            if (k == N - 1 && NSELF) {
#pragma unroll
                for (int a = 0; a < 6; a++) vdx += SN[4 + a] * DXU[N * NV + mmpc_y(a)];
            }
            DS[k] = -(ls.gss - vdx) * mmpc_rcp(ls.hss);
            if (k == N) { for (int c = 0; c < NU; c++) DXU[N * NV + NX + c] = 0.0; }
        }
        LANES_END
        }   // !fatal
        }   // soc_st != 3
        if (fatal) MMPC_ITER_LEAVE
        MMPC_TS(10)
        // ---- D2: row steps, fraction-to-boundary, directional derivative
        const double tau = mmpc_vmax(0.99, 1.0 - mu);
#if MMPC_ITER_SOC
        if (soc_st == 1) {
        constexpr bool socm = true; (void)socm;
#include "mmpc_fast_d2.inc"
        } else
#endif
        {
        constexpr bool socm = false; (void)socm;
#include "mmpc_fast_d2.inc"
        }
        {
            double r4[4];
            MMPC_RED4_MAX(0, 1, 0, 1, r4);   // (two maxima through the four-at-a-time butterfly: 29 instructions instead of 60)
            const double rp_ = r4[0], rd_ = r4[1], ap_n = rp_ > tau ? tau * mmpc_rcp(rp_) : 1.0;
#if MMPC_ITER_SOC
            if (soc_st == 1) {
                // corrected direction: its primal step from x_k (the multipliers have taken their step; the acceptance test
                // uses the length and the slope of the step it corrects)
                a_soc = ap_n;
                apply_step(a_soc, false);
                soc_st = 2; in_ls = 1;
                continue;
            }
#endif
            ap = ap_n; ad = rd_ > tau ? tau * mmpc_rcp(rd_) : 1.0; dphi = MMPC_RED_SUM(2);
#if MMPC_ITER_SOC
            if (soc_st == 3) {
                // the correction failed: the row steps of the uncorrected direction are back in the registers, the line search
                // goes on with its second trial
                alpha = 0.5 * ap; lsi = 1; lspass = 0;
                apply_step(alpha, false);
                soc_st = 0; in_ls = 1;
                continue;
            }
#endif
        }

#if !MMPC_ITER_SOC
        MMPC_TS(11)
        if (!filt_init) { nfilt = 0; th_max = 1e4 * mmpc_vmax(1.0, th0); th_min = 1e-4 * mmpc_vmax(1.0, th0); filt_init = 1; }
        // ---- first trial of the line search: multipliers with alpha_d, primal variables / slacks with alpha = alpha_p
        alpha = ap; lspass = 0; lsi = 0;
        apply_step(alpha, true);
        in_ls = 1;
        it++;
#endif
