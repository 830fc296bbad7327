// mmpc_prim_ops.h - TEST ONLY.  The scalar primitives of the kernels (mmpc_tile.h, mmpc_core.h, mmpc_fast.h) behind one
// numbered entry point, compiled twice: by hipcc into tests/gpu_prim/mmpc_prim.hip (what the GPU executes: v_rcp_f64 seeds,
// v_max_f64, v_exp_f32, ...) and by g++ -DMMPC_EMU into tests/emu/mmpc_emu.cpp (the stand-ins the CPU suite rests on).
// It CALLS the product's functions and macros; it restates none of them.  Included after mmpc_fast.h.
#pragma once

// X(name, id, doubles in, doubles out)
#define MMPC_PRIM_OPS(X)                                                                                                  \
    X(RCP, 0, 1, 1) X(RCP3, 1, 1, 1) X(RCP_PIV, 2, 1, 1) X(RSQRT, 3, 1, 1) X(SQRT_PAIR, 4, 1, 2) X(VMAX, 5, 2, 1)           \
    X(VMIN, 6, 2, 1) X(ZSAFE_FAST, 7, 3, 1) X(ZSAFE, 8, 3, 1) X(POWF, 9, 2, 1) X(MUL24, 10, 2, 1) X(SINCOS, 11, 1, 2)       \
    X(ARM, 12, 3, 6) X(ARM_FAST, 13, 3, 6) X(LOGACC, 14, 15, 2) X(SELF_ROW, 15, 7, 7) X(BOX_T, 16, 1, 1) X(MAX_ERR, 17, 2, 1) \
    X(LOG_MANT, 18, 1, 2)
#define MMPC_PRIM_NOPS 19
#define MMPC_PRIM_LOGACC_K 14   // factors of a LOGACC item (unused ones are 1.0: an exact factor)

enum {
#define X(name, id, nin, nout) MMPC_PRIM_##name = id,
    MMPC_PRIM_OPS(X)
#undef X
};

MMPC_HD constexpr int mmpc_prim_nin(int op) {
#define X(name, id, nin, nout) if (op == id) return nin;
    MMPC_PRIM_OPS(X)
#undef X
    return -1;
}
MMPC_HD constexpr int mmpc_prim_nout(int op) {
#define X(name, id, nin, nout) if (op == id) return nout;
    MMPC_PRIM_OPS(X)
#undef X
    return -1;
}

MMPC_DEV void mmpc_prim_map_one(int op, const double *in, double *out) {
    switch (op) {
    case MMPC_PRIM_RCP: out[0] = mmpc_rcp(in[0]); break;
    case MMPC_PRIM_RCP3: out[0] = mmpc_rcp3(in[0]); break;
    case MMPC_PRIM_RCP_PIV: out[0] = mmpc_rcp_piv(in[0]); break;
    case MMPC_PRIM_RSQRT: out[0] = mmpc_rsqrt(in[0]); break;
    case MMPC_PRIM_SQRT_PAIR: mmpc_sqrt_pair(in[0], &out[0], &out[1]); break;
    case MMPC_PRIM_VMAX: out[0] = mmpc_vmax(in[0], in[1]); break;
    case MMPC_PRIM_VMIN: out[0] = mmpc_vmin(in[0], in[1]); break;
    case MMPC_PRIM_ZSAFE_FAST: out[0] = mmpc_z_safeguard_fast(in[0], in[1], in[2]); break;
    case MMPC_PRIM_ZSAFE: out[0] = mmpc_z_safeguard(in[0], in[1], in[2]); break;
    case MMPC_PRIM_POWF: out[0] = mmpc_powf(in[0], (float)in[1]); break;
    case MMPC_PRIM_MUL24: { const int a = (int)in[0], b = (int)in[1]; out[0] = (double)MMPC_MUL24(a, b); } break;
    case MMPC_PRIM_SINCOS: mmpc_sincos(in[0], &out[0], &out[1]); break;
    case MMPC_PRIM_ARM: mmpc_arm_segments(in[0], in[1], in[2], out, out + 3); break;
    case MMPC_PRIM_ARM_FAST: mmpc_arm_segments_fast(in[0], in[1], in[2], out, out + 3); break;
    case MMPC_PRIM_LOGACC: {   // in[0..13]: the factors, in[14]: the exponent handed in; out: value(), the product itself
        MmpcLogAcc la; la.init(); la.ex = (int)in[MMPC_PRIM_LOGACC_K];
        for (int j = 0; j < MMPC_PRIM_LOGACC_K; j++) la.mul(in[j]);
        out[0] = la.value(); out[1] = la.mant;
    } break;
    case MMPC_PRIM_SELF_ROW: {   // in: row, x, y, psi, q1, q2, q3 (as the evaluation phase calls it); out: h, dh/d(x,y,psi,q1,q2,q3)
        double sn, cs, dr[3], dz[3];
        mmpc_sincos(in[3], &sn, &cs);
        mmpc_arm_segments_fast(in[4], in[5], in[6], dr, dz);
        out[0] = mmpc_self_row((int)in[0], in[1], in[2], cs, sn, dr, dz, out + 1);
    } break;
    case MMPC_PRIM_BOX_T: out[0] = mmpc_box_t(in[0]); break;
    case MMPC_PRIM_MAX_ERR: out[0] = mmpc_max_err(in[0], in[1]); break;
    case MMPC_PRIM_LOG_MANT: { int e = 0; out[0] = mmpc_log_mant(in[0], &e); out[1] = (double)e; } break;
    default: break;
    }
}

// rows of 64 doubles a cross-lane item returns (one row per exchange, every lane's result)
#define MMPC_PRIM_LANE_READLANE 0     // 64 rows: MMPC_LANE_GET(v, J), J = 0..63
#define MMPC_PRIM_LANE_ROWBCAST 64    // 16 rows: mmpc_rowbcast_f64<J>, J = 0..15
#define MMPC_PRIM_LANE_RBALL9 80      // 9 rows: mmpc_rowbcast_all<0, 9>
#define MMPC_PRIM_LANE_RBALL6 89      // 6 rows: mmpc_rowbcast_all<0, 6>
#define MMPC_PRIM_LANE_DPP 95         // 4 rows: mmpc_dpp_f64<0xB1>, <0x4E>, <0x141>, <0x140>
#define MMPC_PRIM_LANE_XOR16 99       // MMPC_LANE_XOR16(v)
#define MMPC_PRIM_LANE_LOWER16 100    // MMPC_LANE_LOWER16(v)
#define MMPC_PRIM_LANE_XOR32 101      // mmpc_xor32_f64
#define MMPC_PRIM_LANE_ROWS 102
// rows of a reduction item: MMPC_RED_SUM / MAX / MIN (mmpc_wave_*), MMPC_GRED_SUM / MAX / MIN / MAXERR (mmpc_gwave_*)
#define MMPC_PRIM_RED_ROWS 7
