// Host lane-emulation build of the HIP solver core (TEST ONLY - never part of the product).
// Compiles mobile-manipulator-mpc_amd/csrc/mmpc_core.h with -DMMPC_EMU so that the phase
// structured kernel runs on the CPU: each phase is a loop over the 64 lanes.  Used by
// tests/test_emu_kernel.py to check the kernel logic (and its memory accesses, under ASAN)
// against the oracle before anything is launched on a GPU.  `reverse` runs the lanes of every
// phase in the opposite order: a result that changes exposes an intra-phase data race.
#define MMPC_EMU 1
#include "../emu_common/mmpc_emu_poison.h"
#include "../../mobile-manipulator-mpc_amd/csrc/mmpc_fast.h"
#include "../../mobile-manipulator-mpc_amd/csrc/mmpc_ik.h"
#include <stdlib.h>
#include <string.h>

template <int KIND>
static void run(const MmpcParams *P, int B, const double *x_init, const double *traj_ref, const double *u_ref,
                const double *u_last, const double *x_guess, const double *obs, double *X, double *U, double *s,
                int *status, int *iters, double *cost, double *err, int reverse) {
    typedef MmpcDims<KIND> D;
    const int N = P->N, M = P->M;
    MmpcLayout L = mmpc_layout<KIND>(N, M, P->obs_per_stage, (KIND == 0 && P->L > 0) ? 6 : 0,
                                     (KIND == 0 && P->L >= 2 && P->as_written) ? 6 * (P->L - 1) : 0);
    const size_t so = (size_t)(P->obs_per_stage ? N + 1 : 1) * M * 3;
    MmpcEmuBlock lds_b, soc_b;   // (mmpc_emu_poison.h: what the blocks hold at the start of an instance is the caller's choice, NaN by default)
    for (int b = 0; b < B; b++) {
        // exact-size heap slab so that ASAN sees any out-of-slab access
        double *lds = lds_b.next(L.total);
        // scratch of the second-order correction (global memory on the device), exact size as the slab
        double *soc = soc_b.next(mmpc_soc_doubles(N, D::NX, D::NU, L.NR));
        // (the scratch is this instance's own: stride 0)
        MmpcIO io;
        mmpc_instance_io<KIND>(io, *P, b, N, so, x_init, traj_ref, u_ref, u_last, x_guess, obs, X, U, s, status, iters, cost, err,
                               soc, 0);
        MmpcEmu emu = reverse ? MmpcEmu{63, -1, -1} : MmpcEmu{0, 64, 1};
        mmpc_solve_one<KIND>(*P, io, lds, emu);
    }
}

template <int KIND, int N, int MC>
static void run_fast(const MmpcParams *P, int B, const double *x_init, const double *traj_ref, const double *u_ref,
                     const double *u_last, const double *x_guess, const double *obs, double *X, double *U, double *s,
                     int *status, int *iters, double *cost, double *err, int reverse, int budget = 0, double *state = nullptr,
                     int resume = 0) {
    typedef MmpcDims<KIND> D;
    const int M = MC;
    MmpcFastLayout L = mmpc_fast_layout<KIND, N>(M, P->obs_per_stage);
    const size_t so = (size_t)(P->obs_per_stage ? N + 1 : 1) * M * 3;
    MmpcEmuBlock lds_b, gscr_b, soc_b;
    for (int b = 0; b < B; b++) {
        const int sd = mmpc_fast_state_doubles<KIND, N>(MC);
        if (resume && status[b] != 3) continue;   // a continuation launch only runs the suspended instances
        double *lds = lds_b.next(L.total);
        MmpcEmu emu = reverse ? MmpcEmu{63, -1, -1} : MmpcEmu{0, 64, 1};
        // gain block of the long horizons (global memory on the device)
        double *gscr = gscr_b.next(MmpcGainBlock<KIND, N>::total);
        double *soc = soc_b.next(mmpc_soc_doubles(N, D::NX, D::NU, MC + D::NSELF));
        MmpcIO io;
        mmpc_instance_io<KIND>(io, *P, b, N, so, x_init, traj_ref, u_ref, u_last, x_guess, obs, X, U, s, status, iters, cost, err,
                               soc, 0);
        io.state = state ? state + (size_t)b * sd : nullptr; io.budget = budget; io.resume = resume; io.gscr = gscr;   // (as mmpc_fast_kernel)
        if (budget > 0 || resume) mmpc_solve_fast<KIND, N, MC, true>(*P, io, lds, emu); else mmpc_solve_fast<KIND, N, MC, false>(*P, io, lds, emu);
    }
}

// fast path (template on the horizon): returns -1 when this (kind, N, M) has no fast instantiation
extern "C" int mmpc_emu_solve_fast(int kind, const MmpcParams *P, int B, const double *x_init, const double *traj_ref,
                                   const double *u_ref, const double *u_last, const double *x_guess, const double *obs,
                                   double *X, double *U, double *s, int *status, int *iters, double *cost, double *err,
                                   int reverse) {
#define MMPC_FAST_CASE(K, NN, MM) if (kind == K && P->N == NN && P->M == MM) { run_fast<K, NN, MM>(P, B, x_init, traj_ref, u_ref, u_last, x_guess, obs, X, U, s, status, iters, cost, err, reverse); return 0; }
    MMPC_FAST_CASE(0, 20, 5) MMPC_FAST_CASE(0, 20, 3) MMPC_FAST_CASE(0, 30, 8) MMPC_FAST_CASE(0, 20, 0) MMPC_FAST_CASE(1, 15, 3)
#undef MMPC_FAST_CASE
    return -1;
}
// same with an iteration budget: state = [B][mmpc_emu_fast_state_doubles] save area; resume != 0 continues the instances whose
// status[] is 3 (MMPC_STATUS_SUSPENDED) and leaves the others alone
extern "C" int mmpc_emu_solve_fast_budget(int kind, const MmpcParams *P, int B, const double *x_init, const double *traj_ref,
                                          const double *u_ref, const double *u_last, const double *x_guess, const double *obs,
                                          double *X, double *U, double *s, int *status, int *iters, double *cost, double *err,
                                          int budget, double *state, int resume) {
#define MMPC_FAST_CASE(K, NN, MM) if (kind == K && P->N == NN && P->M == MM) { run_fast<K, NN, MM>(P, B, x_init, traj_ref, u_ref, u_last, x_guess, obs, X, U, s, status, iters, cost, err, 0, budget, state, resume); return 0; }
    MMPC_FAST_CASE(0, 20, 5) MMPC_FAST_CASE(0, 20, 3) MMPC_FAST_CASE(0, 30, 8) MMPC_FAST_CASE(1, 15, 3)
#undef MMPC_FAST_CASE
    return -1;
}
extern "C" int mmpc_emu_fast_state_doubles(int kind, int N, int M) {
    if (kind == 0 && N == 20) return mmpc_fast_state_doubles<0, 20>(M);
    if (kind == 0 && N == 30) return mmpc_fast_state_doubles<0, 30>(M);
    if (kind == 1 && N == 15) return mmpc_fast_state_doubles<1, 15>(M);
    return -1;
}
// where the MMPC_NSCAL scalars of a suspended solve start in its save area: the kernel's own constant (ST_SCAL of the park / resume
// code, which asserts that it is this function's value), the same for every M and obstacle mode of a (kind, N)
extern "C" int mmpc_emu_fast_state_scal_offset(int kind, int N) {
    if (kind == 0 && N == 20) return mmpc_fast_state_scal_offset<0, 20>();
    if (kind == 0 && N == 30) return mmpc_fast_state_scal_offset<0, 30>();
    if (kind == 1 && N == 15) return mmpc_fast_state_scal_offset<1, 15>();
    return -1;
}
extern "C" int mmpc_emu_fcap() { return MMPC_FCAP; }
extern "C" int mmpc_emu_fast_lds_doubles(int kind, int N, int M, int obs_per_stage) {
    if (kind == 0 && N == 20) return mmpc_fast_layout<0, 20>(M, obs_per_stage).total;
    if (kind == 0 && N == 30) return mmpc_fast_layout<0, 30>(M, obs_per_stage).total;
    if (kind == 1 && N == 15) return mmpc_fast_layout<1, 15>(M, obs_per_stage).total;
    return -1;
}

extern "C" int mmpc_emu_solve(int kind, const MmpcParams *P, int B, const double *x_init, const double *traj_ref,
                              const double *u_ref, const double *u_last, const double *x_guess, const double *obs,
                              double *X, double *U, double *s, int *status, int *iters, double *cost, double *err,
                              int reverse) {
    if (kind == 0) run<0>(P, B, x_init, traj_ref, u_ref, u_last, x_guess, obs, X, U, s, status, iters, cost, err, reverse);
    else if (kind == 1) run<1>(P, B, x_init, traj_ref, u_ref, u_last, x_guess, obs, X, U, s, status, iters, cost, err, reverse);
    else run<2>(P, B, x_init, traj_ref, u_ref, u_last, x_guess, obs, X, U, s, status, iters, cost, err, reverse);
    return 0;
}
// LDS slab of the generic kernel as mmpc_create sizes it: nhs = half-space rows per stage (6 when L > 0), nq = as-written extra
// rows per stage (6 (L - 1)); both whole-body kind only
extern "C" int mmpc_emu_lds_doubles(int kind, int N, int M, int obs_per_stage, int nhs, int nq) {
    return kind == 0 ? mmpc_layout<0>(N, M, obs_per_stage, nhs, nq).total : kind == 1 ? mmpc_layout<1>(N, M, obs_per_stage).total : mmpc_layout<2>(N, M, obs_per_stage).total;
}
extern "C" int mmpc_emu_params_size() { return (int)sizeof(MmpcParams); }

// arm inverse kinematics (mmpc_ik.h is plain scalar code: the same function the GPU kernel calls per lane)
extern "C" void mmpc_emu_ik(int B, const double *q0, const double *target, double *q, int *status, int *iters) {
    for (int b = 0; b < B; b++) status[b] = mmpc_ik_solve(q0 + 3 * b, target[2 * b], target[2 * b + 1], q + 3 * b, iters + b);
}

// ---- the primitives one at a time (tests/test_primitives_cpu.py, tests/test_gpu_primitives.py): the host twin of
// tests/gpu_prim/mmpc_prim.hip with the same entry points, item layouts and row numbers.  The scalar functions come from the
// shared mmpc_prim_ops.h; the cross-lane exchanges, reductions and the matrix-core tile go through the stand-ins of this
// build (MMPC_LANE_*, mmpc_emu_red / _red4 / _red_arr, the fma loops of MMPC_MFMA) exactly as the emulated solver uses them.
#include "../gpu_prim/mmpc_prim_ops.h"
extern "C" int mmpc_emu_prim_op_shape(int op, int *nin, int *nout) {
    *nin = mmpc_prim_nin(op); *nout = mmpc_prim_nout(op);
    return *nin > 0 ? 0 : -1;
}
extern "C" int mmpc_emu_prim_map(int op, int n, const double *in, double *out) {
    const int nin = mmpc_prim_nin(op), nout = mmpc_prim_nout(op);
    if (n <= 0 || nin <= 0) return -1;
    for (int i = 0; i < n; i++) {
        for (int j = 0; j < nout; j++) out[(size_t)i * nout + j] = 0.0;
        mmpc_prim_map_one(op, in + (size_t)i * nin, out + (size_t)i * nout);
    }
    return 0;
}
// only the exchanges this build has a stand-in for: the rows MMPC_PRIM_LANE_READLANE + j, _XOR16, _LOWER16 (the others stay 0;
// the roll-out's row broadcast is replaced by MMPC_LANE_GET, the butterflies' DPP steps by the partner index of mmpc_emu_red)
struct MmpcPrimLane { double v; };
extern "C" int mmpc_emu_prim_lanes(int nvec, const double *in, double *out) {
    if (nvec <= 0) return -1;
    for (int b = 0; b < nvec; b++) {
        MmpcPrimLane ls_all[MMPC_WAVE];
        double *o = out + (size_t)b * MMPC_PRIM_LANE_ROWS * MMPC_WAVE;
        for (int i = 0; i < MMPC_PRIM_LANE_ROWS * MMPC_WAVE; i++) o[i] = 0.0;
        for (int lane = 0; lane < MMPC_WAVE; lane++) ls_all[lane].v = in[(size_t)b * MMPC_WAVE + lane];
        for (int lane = 0; lane < MMPC_WAVE; lane++) {
            for (int j = 0; j < MMPC_WAVE; j++) o[MMPC_WAVE * (MMPC_PRIM_LANE_READLANE + j) + lane] = MMPC_LANE_GET(v, j);
            o[MMPC_WAVE * MMPC_PRIM_LANE_XOR16 + lane] = MMPC_LANE_XOR16(v);
            o[MMPC_WAVE * MMPC_PRIM_LANE_LOWER16 + lane] = MMPC_LANE_LOWER16(v);
        }
    }
    return 0;
}
extern "C" int mmpc_emu_prim_red(int nvec, const double *in, double *out) {
    if (nvec <= 0) return -1;
    for (int b = 0; b < nvec; b++) {
        double wr_all[MMPC_WAVE][9], RED[MMPC_WAVE], r[MMPC_PRIM_RED_ROWS];
        for (int lane = 0; lane < MMPC_WAVE; lane++) {
            for (int i = 0; i < 9; i++) wr_all[lane][i] = -7.0;
            wr_all[lane][3] = RED[lane] = in[(size_t)b * MMPC_WAVE + lane];
        }
        r[0] = MMPC_RED_SUM(3); r[1] = MMPC_RED_MAX(3); r[2] = MMPC_RED_MIN(3);
        r[3] = MMPC_GRED_SUM(RED); r[4] = MMPC_GRED_MAX(RED); r[5] = MMPC_GRED_MIN(RED); r[6] = MMPC_GRED_MAXERR(RED);
        for (int q = 0; q < MMPC_PRIM_RED_ROWS; q++)   // (a value the emulated lanes share: every "lane" gets it)
            for (int lane = 0; lane < MMPC_WAVE; lane++) out[((size_t)b * MMPC_PRIM_RED_ROWS + q) * MMPC_WAVE + lane] = r[q];
    }
    return 0;
}
extern "C" int mmpc_emu_prim_red4(int nvec, const double *in, double *out) {
    if (nvec <= 0) return -1;
    for (int b = 0; b < nvec; b++) {
        double wr_all[MMPC_WAVE][9], s4[4], m4[4];
        const double *v = in + (size_t)b * 4 * MMPC_WAVE;
        for (int lane = 0; lane < MMPC_WAVE; lane++) {
            for (int i = 0; i < 9; i++) wr_all[lane][i] = -7.0;
            wr_all[lane][1] = v[lane]; wr_all[lane][4] = v[MMPC_WAVE + lane]; wr_all[lane][6] = v[2 * MMPC_WAVE + lane]; wr_all[lane][8] = v[3 * MMPC_WAVE + lane];
        }
        MMPC_RED4_SUM(1, 4, 6, 8, s4);
        MMPC_RED4_MAX(1, 4, 6, 8, m4);
        for (int j = 0; j < 4; j++)
            for (int lane = 0; lane < MMPC_WAVE; lane++) {
                out[((size_t)b * 8 + j) * MMPC_WAVE + lane] = s4[j]; out[((size_t)b * 8 + 4 + j) * MMPC_WAVE + lane] = m4[j];
            }
    }
    return 0;
}
struct MmpcPrimTile { MmpcAcc acc, s, d; double a, b; };
extern "C" int mmpc_emu_prim_mfma(int nvec, const double *in, double *out) {
    if (nvec <= 0) return -1;
    for (int b = 0; b < nvec; b++) {
        MmpcPrimTile ls_all[MMPC_WAVE];
        const double *v = in + (size_t)b * 6 * MMPC_WAVE;
        double *o = out + (size_t)b * 8 * MMPC_WAVE;
        for (int l = 0; l < MMPC_WAVE; l++) { ls_all[l].a = v[l]; ls_all[l].b = v[MMPC_WAVE + l]; }
        MMPC_MFMA0(acc, ls.a, ls.b)
        for (int l = 0; l < MMPC_WAVE; l++) for (int r = 0; r < 4; r++) { o[r * MMPC_WAVE + l] = ls_all[l].acc[r]; ls_all[l].acc[r] = v[(2 + r) * MMPC_WAVE + l]; }
        MMPC_MFMA(acc, ls.a, ls.b)
        for (int l = 0; l < MMPC_WAVE; l++) for (int r = 0; r < 4; r++) o[(4 + r) * MMPC_WAVE + l] = ls_all[l].acc[r];
    }
    return 0;
}
extern "C" int mmpc_emu_prim_chain(int nvec, const double *in, double *out) {
    if (nvec <= 0) return -1;
    for (int b = 0; b < nvec; b++) {
        MmpcPrimTile ls_all[MMPC_WAVE];
        const double *v = in + (size_t)b * 8 * MMPC_WAVE;
        double *o = out + (size_t)b * 8 * MMPC_WAVE;
        for (int l = 0; l < MMPC_WAVE; l++) for (int r = 0; r < 4; r++) { ls_all[l].s[r] = v[r * MMPC_WAVE + l]; ls_all[l].d[r] = v[(4 + r) * MMPC_WAVE + l]; }
        MMPC_MFMA0(acc, ls.s[0], ls.d[0])
        MMPC_MFMA(acc, ls.s[1], ls.d[1])
        MMPC_MFMA(acc, ls.s[2], ls.d[2])
        MMPC_MFMA(acc, ls.s[3], ls.d[3])
        for (int l = 0; l < MMPC_WAVE; l++) for (int r = 0; r < 4; r++) o[r * MMPC_WAVE + l] = ls_all[l].acc[r];
        MMPC_MFMA0(acc, ls.d[0], ls.s[0])
        MMPC_MFMA(acc, ls.d[1], ls.s[1])
        MMPC_MFMA(acc, ls.d[2], ls.s[2])
        MMPC_MFMA(acc, ls.d[3], ls.s[3])
        for (int l = 0; l < MMPC_WAVE; l++) for (int r = 0; r < 4; r++) o[(4 + r) * MMPC_WAVE + l] = ls_all[l].acc[r];
    }
    return 0;
}
