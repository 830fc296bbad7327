// Host lane-emulation build of the solver kernels for the objective scaling (TEST ONLY - never part of the product).
// The lane loop of tests/emu_motion/mmpc_emu_motion.cpp (each phase a loop over the 64 lanes, `reverse` runs them in the opposite
// order, an exact-size heap slab per instance) with what that source does not pass: the two scaling fields of MmpcIO -
// scale_max_grad (0: off) and a scale_out array [B] (null: not wanted) - set after mmpc_instance_io the way the device kernel
// wrappers set them, and an X guess.  With scale_max_grad = 0 the entry points are plain solves, so one library solves an
// instance with the option on and its twin with scaled weights and the option off.
#define MMPC_EMU 1
#include "../emu_common/mmpc_emu_poison.h"
#include "../../mobile-manipulator-mpc_amd/csrc/mmpc_fast.h"
#include <stdlib.h>
#include <string.h>

static size_t obs_stride(const MmpcParams *P, int N, int M) {
    return P->obs_per_stage == 2 ? (size_t)M * 5 : (size_t)(P->obs_per_stage ? N + 1 : 1) * M * 3;
}
// exact-size copy of one instance's obstacles
static double *obs_copy(const double *obs, int b, size_t so) {
    double *o = (double *)malloc(sizeof(double) * (so ? so : 1));
    if (so) memcpy(o, obs + (size_t)b * so, sizeof(double) * so);
    return o;
}

template <int KIND>
static void run(const MmpcParams *P, int B, const double *x_init, const double *traj_ref, const double *u_ref, const double *u_last,
                const double *x_guess, const double *obs, double *X, double *U, double *s, int *status, int *iters, double *cost,
                double *err, int reverse, double scale_max_grad, double *scale_out) {
    typedef MmpcDims<KIND> D;
    const int N = P->N, M = P->M;
    // (half-space planes and their rows as written size the slab too: the fixtures of tools/objective_scaling_probe.py have some)
    const MmpcLayout L = mmpc_layout<KIND>(N, M, P->obs_per_stage, (KIND == 0 && P->L > 0) ? 6 : 0,
                                           (KIND == 0 && P->L >= 2 && P->as_written) ? 6 * (P->L - 1) : 0);
    const size_t so = obs_stride(P, N, M);
    MmpcEmuBlock lds_b, soc_b;   // (mmpc_emu_poison.h: what the blocks hold at the start of an instance is the caller's choice, NaN by default)
    for (int b = 0; b < B; b++) {
        double *lds = lds_b.next(L.total);
        double *soc = soc_b.next(mmpc_soc_doubles(N, D::NX, D::NU, L.NR));
        double *ob = obs_copy(obs, b, so);
        MmpcIO io;
        mmpc_instance_io<KIND>(io, *P, b, N, so, x_init, traj_ref, u_ref, u_last, x_guess, obs, X, U, s, status, iters, cost, err, soc, 0);
        io.obs = ob;
        io.scale_max_grad = scale_max_grad; if (scale_out) io.scale_out = scale_out + b;
        MmpcEmu emu = reverse ? MmpcEmu{63, -1, -1} : MmpcEmu{0, 64, 1};
        mmpc_solve_one<KIND>(*P, io, lds, emu);
        free(ob);
    }
}

template <int KIND, int N, int MC>
static void run_fast(const MmpcParams *P, int B, const double *x_init, const double *traj_ref, const double *u_ref, const double *u_last,
                     const double *x_guess, const double *obs, double *X, double *U, double *s, int *status, int *iters, double *cost,
                     double *err, int reverse, int budget, double *state, int resume, double scale_max_grad, double *scale_out) {
    typedef MmpcDims<KIND> D;
    const MmpcFastLayout L = mmpc_fast_layout<KIND, N>(MC, P->obs_per_stage);
    const size_t so = obs_stride(P, N, MC);
    const int sd = mmpc_fast_state_doubles<KIND, N>(MC);
    MmpcEmuBlock lds_b, gscr_b, soc_b;
    for (int b = 0; b < B; b++) {
        if (resume && status[b] != 3) continue;   // a continuation launch only runs the suspended instances
        double *lds = lds_b.next(L.total);
        double *gscr = gscr_b.next(MmpcGainBlock<KIND, N>::total);
        double *soc = soc_b.next(mmpc_soc_doubles(N, D::NX, D::NU, MC + D::NSELF));
        double *ob = obs_copy(obs, b, so);
        MmpcIO io;
        mmpc_instance_io<KIND>(io, *P, b, N, so, x_init, traj_ref, u_ref, u_last, x_guess, obs, X, U, s, status, iters, cost, err, soc, 0);
        io.obs = ob;
        io.state = state ? state + (size_t)b * sd : nullptr; io.budget = budget; io.resume = resume; io.gscr = gscr;
        io.scale_max_grad = scale_max_grad; if (scale_out) io.scale_out = scale_out + b;
        MmpcEmu emu = reverse ? MmpcEmu{63, -1, -1} : MmpcEmu{0, 64, 1};
        if (budget > 0 || resume) mmpc_solve_fast<KIND, N, MC, true>(*P, io, lds, emu); else mmpc_solve_fast<KIND, N, MC, false>(*P, io, lds, emu);
        free(ob);
    }
}

extern "C" int mmpc_emus_solve(int kind, const MmpcParams *P, int B, const double *x_init, const double *traj_ref, const double *u_ref,
                               const double *u_last, const double *x_guess, const double *obs, double *X, double *U, double *s,
                               int *status, int *iters, double *cost, double *err, int reverse, double scale_max_grad, double *scale_out) {
    if (kind == 0) run<0>(P, B, x_init, traj_ref, u_ref, u_last, x_guess, obs, X, U, s, status, iters, cost, err, reverse, scale_max_grad, scale_out);
    else if (kind == 1) run<1>(P, B, x_init, traj_ref, u_ref, u_last, x_guess, obs, X, U, s, status, iters, cost, err, reverse, scale_max_grad, scale_out);
    else if (kind == 2) run<2>(P, B, x_init, traj_ref, u_ref, u_last, x_guess, obs, X, U, s, status, iters, cost, err, reverse, scale_max_grad, scale_out);
    else return -1;
    return 0;
}
#define MMPC_EMUS_SHAPES(X) X(0, 20, 5) X(0, 30, 8) X(0, 20, 3) X(1, 15, 3)
// specialised kernels; budget > 0 / resume as mmpc_fast_kernel (state: [B][mmpc_emus_fast_state_doubles]); -1: no such shape
extern "C" int mmpc_emus_solve_fast(int kind, const MmpcParams *P, int B, const double *x_init, const double *traj_ref,
                                    const double *u_ref, const double *u_last, const double *x_guess, const double *obs, double *X,
                                    double *U, double *s, int *status, int *iters, double *cost, double *err, int reverse, int budget,
                                    double *state, int resume, double scale_max_grad, double *scale_out) {
#define MMPC_X(K, NN, MM) if (kind == K && P->N == NN && P->M == MM) { run_fast<K, NN, MM>(P, B, x_init, traj_ref, u_ref, u_last, x_guess, obs, X, U, s, status, iters, cost, err, reverse, budget, state, resume, scale_max_grad, scale_out); return 0; }
    MMPC_EMUS_SHAPES(MMPC_X)
#undef MMPC_X
    return -1;
}
extern "C" int mmpc_emus_fast_state_doubles(int kind, int N, int M) {
#define MMPC_X(K, NN, MM) if (kind == K && N == NN && M == MM) return mmpc_fast_state_doubles<K, NN>(MM);
    MMPC_EMUS_SHAPES(MMPC_X)
#undef MMPC_X
    return -1;
}
extern "C" int mmpc_emus_fast_lds_doubles(int kind, int N, int M, int obs_per_stage) {
#define MMPC_X(K, NN, MM) if (kind == K && N == NN && M == MM) return mmpc_fast_layout<K, NN>(MM, obs_per_stage).total;
    MMPC_EMUS_SHAPES(MMPC_X)
#undef MMPC_X
    return -1;
}
extern "C" int mmpc_emus_lds_doubles(int kind, int N, int M, int obs_per_stage, int nhs, int nq) {
    return kind == 0 ? mmpc_layout<0>(N, M, obs_per_stage, nhs, nq).total : kind == 1 ? mmpc_layout<1>(N, M, obs_per_stage, nhs, nq).total : mmpc_layout<2>(N, M, obs_per_stage, nhs, nq).total;
}
extern "C" int mmpc_emus_params_size() { return (int)sizeof(MmpcParams); }
