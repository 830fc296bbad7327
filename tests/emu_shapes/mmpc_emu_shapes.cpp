// Host lane-emulation build of the specialised template at ONE shape outside MMPC_FAST_LIST (TEST ONLY - never part of the product):
// -DMMPC_EMUSH_KIND= -DMMPC_EMUSH_N= -DMMPC_EMUSH_M=, one library per shape (tests/shape_helper.py), so that the shapes compile side
// by side.  The lane loop of tests/emu_scaling/mmpc_emu_scaling.cpp (each phase a loop over the 64 lanes, `reverse` runs them in
// the opposite order, an exact-size heap slab per instance) with the tick array of tests/emu_motion/mmpc_emu_motion.cpp, and next
// to it the generic kernel's emulation of the same configuration.  Build with -ffp-contract=off (the motion centres are defined
// operation by operation).  -DMMPC_EMUSH_MAIN adds a main(): the stand-alone program of the sanitizer run, which solves the
// instances of a file written by shape_helper.write_case and exits 0 when every one of them converged.
#define MMPC_EMU 1
#include "../emu_common/mmpc_emu_poison.h"
#include "../../mobile-manipulator-mpc_amd/csrc/mmpc_fast.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#if !defined(MMPC_EMUSH_KIND) || !defined(MMPC_EMUSH_N) || !defined(MMPC_EMUSH_M)
#error "build with -DMMPC_EMUSH_KIND= -DMMPC_EMUSH_N= -DMMPC_EMUSH_M= (tests/shape_helper.py)"
#endif
static_assert(mmpc_fast_shape_ok(MMPC_EMUSH_KIND, MMPC_EMUSH_N, MMPC_EMUSH_M), "the shape is outside the specialised envelope");

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
                const double *obs, const long long *tick, double *X, double *U, double *s, int *status, int *iters, double *cost,
                double *err, int reverse) {
    typedef MmpcDims<KIND> D;
    const int N = P->N, M = P->M;
    const MmpcLayout L = mmpc_layout<KIND>(N, M, P->obs_per_stage, 0, 0);
    const size_t so = obs_stride(P, N, M);
    MmpcEmuBlock lds_b, soc_b;   // (mmpc_emu_poison.h: what the blocks hold at the start of an instance is the caller's choice, NaN by default)
    for (int b = 0; b < B; b++) {
        double *lds = lds_b.next(L.total);
        double *soc = soc_b.next(mmpc_soc_doubles(N, D::NX, D::NU, L.NR));
        double *ob = obs_copy(obs, b, so);
        MmpcIO io;
        mmpc_instance_io<KIND>(io, *P, b, N, so, x_init, traj_ref, u_ref, u_last, nullptr, obs, X, U, s, status, iters, cost, err, soc, 0);
        io.obs = ob;
        if (P->obs_per_stage == 2 && tick) io.tick = tick + b;
        MmpcEmu emu = reverse ? MmpcEmu{63, -1, -1} : MmpcEmu{0, 64, 1};
        mmpc_solve_one<KIND>(*P, io, lds, emu);
        free(ob);
    }
}

template <int KIND, int N, int MC>
static void run_fast(const MmpcParams *P, int B, const double *x_init, const double *traj_ref, const double *u_ref, const double *u_last,
                     const double *obs, const long long *tick, double *X, double *U, double *s, int *status, int *iters, double *cost,
                     double *err, int reverse, int budget, double *state, int resume, const double *x_guess = nullptr) {
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
        if (P->obs_per_stage == 2 && tick) io.tick = tick + b;
        MmpcEmu emu = reverse ? MmpcEmu{63, -1, -1} : MmpcEmu{0, 64, 1};
        if (budget > 0 || resume) mmpc_solve_fast<KIND, N, MC, true>(*P, io, lds, emu); else mmpc_solve_fast<KIND, N, MC, false>(*P, io, lds, emu);
        free(ob);
    }
}

static bool shape_of(int kind, const MmpcParams *P) { return kind == MMPC_EMUSH_KIND && P->N == MMPC_EMUSH_N && P->M == MMPC_EMUSH_M; }

// the generic kernel at the library's shape
extern "C" int mmpc_emush_solve(int kind, const MmpcParams *P, int B, const double *x_init, const double *traj_ref, const double *u_ref,
                                const double *u_last, const double *obs, const long long *tick, double *X, double *U, double *s,
                                int *status, int *iters, double *cost, double *err, int reverse) {
    if (!shape_of(kind, P)) return -1;
    run<MMPC_EMUSH_KIND>(P, B, x_init, traj_ref, u_ref, u_last, obs, tick, X, U, s, status, iters, cost, err, reverse);
    return 0;
}
// the specialised kernel; budget > 0 / resume as mmpc_fast_kernel (state: [B][mmpc_emush_fast_state_doubles]); x_guess: [B][N+1][NX], the
// launch argument of the same name, or null; -1: not this library's shape
extern "C" int mmpc_emush_solve_fast_guess(int kind, const MmpcParams *P, int B, const double *x_init, const double *traj_ref,
                                           const double *u_ref, const double *u_last, const double *obs, const long long *tick, double *X,
                                           double *U, double *s, int *status, int *iters, double *cost, double *err, int reverse, int budget,
                                           double *state, int resume, const double *x_guess) {
    if (!shape_of(kind, P)) return -1;
    run_fast<MMPC_EMUSH_KIND, MMPC_EMUSH_N, MMPC_EMUSH_M>(P, B, x_init, traj_ref, u_ref, u_last, obs, tick, X, U, s, status, iters, cost, err,
                                                          reverse, budget, state, resume, x_guess);
    return 0;
}
extern "C" int mmpc_emush_solve_fast(int kind, const MmpcParams *P, int B, const double *x_init, const double *traj_ref,
                                     const double *u_ref, const double *u_last, const double *obs, const long long *tick, double *X,
                                     double *U, double *s, int *status, int *iters, double *cost, double *err, int reverse, int budget,
                                     double *state, int resume) {
    return mmpc_emush_solve_fast_guess(kind, P, B, x_init, traj_ref, u_ref, u_last, obs, tick, X, U, s, status, iters, cost, err, reverse, budget,
                                       state, resume, nullptr);
}
extern "C" int mmpc_emush_fast_state_doubles() { return mmpc_fast_state_doubles<MMPC_EMUSH_KIND, MMPC_EMUSH_N>(MMPC_EMUSH_M); }
extern "C" int mmpc_emush_fast_state_scal_offset() { return mmpc_fast_state_scal_offset<MMPC_EMUSH_KIND, MMPC_EMUSH_N>(); }   // (the scalars of the save area)
extern "C" int mmpc_emush_fast_lds_doubles(int obs_per_stage) { return mmpc_fast_layout<MMPC_EMUSH_KIND, MMPC_EMUSH_N>(MMPC_EMUSH_M, obs_per_stage).total; }
extern "C" int mmpc_emush_lds_doubles(int obs_per_stage) { return mmpc_layout<MMPC_EMUSH_KIND>(MMPC_EMUSH_N, MMPC_EMUSH_M, obs_per_stage, 0, 0).total; }
extern "C" int mmpc_emush_padmap() { return MmpcFastDims<MMPC_EMUSH_KIND, MMPC_EMUSH_N>::PADMAP ? 1 : 0; }
extern "C" int mmpc_emush_params_size() { return (int)sizeof(MmpcParams); }
// the envelope predicate as the device build evaluates it (mmpc_shape_supported without a HIP library)
extern "C" int mmpc_emush_shape_ok(int kind, int N, int M) { return mmpc_fast_shape_ok(kind, N, M) ? 1 : 0; }

#ifdef MMPC_EMUSH_MAIN
// case file: int32 B | MmpcParams | x_init | traj_ref | u_ref | u_last | obs (static record), all float64, this library's shape
int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s case-file\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    typedef MmpcDims<MMPC_EMUSH_KIND> D;
    const int N = MMPC_EMUSH_N, M = MMPC_EMUSH_M, NX = D::NX, NU = D::NU;
    int B = 0;
    MmpcParams P;
    if (fread(&B, sizeof(int), 1, f) != 1 || B < 1 || B > 64 || fread(&P, sizeof(P), 1, f) != 1 || P.N != N || P.M != M || P.obs_per_stage != 0) {
        fprintf(stderr, "bad case file\n"); return 2;
    }
    const size_t n_x = (size_t)B * NX, n_t = (size_t)B * (N + 1) * NX, n_u = (size_t)B * N * NU, n_o = (size_t)B * M * 3, n_s = (size_t)B * (N + 1);
    double *x_init = new double[n_x], *traj = new double[n_t], *uref = new double[n_u], *ulast = new double[n_u], *obs = new double[n_o ? n_o : 1];
    if (fread(x_init, 8, n_x, f) != n_x || fread(traj, 8, n_t, f) != n_t || fread(uref, 8, n_u, f) != n_u || fread(ulast, 8, n_u, f) != n_u ||
        fread(obs, 8, n_o, f) != n_o) { fprintf(stderr, "short case file\n"); return 2; }
    fclose(f);
    double *X = new double[n_t], *U = new double[n_u], *s = new double[n_s], *cost = new double[B], *err = new double[B];
    int *status = new int[B], *iters = new int[B];
    int bad = 0;
    for (int reverse = 0; reverse < 2; reverse++) {
        if (mmpc_emush_solve_fast(MMPC_EMUSH_KIND, &P, B, x_init, traj, uref, ulast, obs, nullptr, X, U, s, status, iters, cost, err, reverse, 0, nullptr, 0)) return 2;
        for (int b = 0; b < B; b++) { printf("reverse %d instance %d: status %d iters %d cost %.17g\n", reverse, b, status[b], iters[b], cost[b]); bad += status[b] != 0; }
    }
    delete[] x_init; delete[] traj; delete[] uref; delete[] ulast; delete[] obs; delete[] X; delete[] U; delete[] s; delete[] cost; delete[] err;
    delete[] status; delete[] iters;
    return bad ? 1 : 0;
}
#endif
