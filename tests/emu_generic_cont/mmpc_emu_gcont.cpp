// Host lane-emulation build of the GENERIC solver core with its iteration budget / continuation code (TEST ONLY - never part of
// the product).  Compiles mobile-manipulator-mpc_amd/csrc/mmpc_core.h with -DMMPC_EMU and instantiates mmpc_solve_one both ways:
// CONT = false (what every default handle runs) and CONT = true (what a handle created with cfg.generic_budget runs).  Used by
// tests/test_generic_continuation_cpu.py through tests/generic_cont_helper.py.  -DMMPC_EMUG_MAIN adds a main() that cuts one small
// batch at every iteration, so that the same code can be built as a stand-alone program under a sanitizer.
#define MMPC_EMU 1
#include "../emu_common/mmpc_emu_poison.h"
#include "../../mobile-manipulator-mpc_amd/csrc/mmpc_core.h"
#include <stdlib.h>
#include <string.h>

template <int KIND>
static MmpcLayout layout_of(const MmpcParams *P) {
    return mmpc_layout<KIND>(P->N, P->M, P->obs_per_stage, (KIND == 0 && P->L > 0) ? 6 : 0,
                             (KIND == 0 && P->L >= 2 && P->as_written) ? 6 * (P->L - 1) : 0);
}

// cont: the CONT = true instantiation (budget, state, resume as the kernel wrapper sets them); a continuation launch (resume != 0)
// runs the instances whose status[] is 3 and leaves the others alone.  Slab, correction scratch: exact-size heap blocks filled as
// mmpc_emu_poison.h says (NaN by default), as tests/emu/mmpc_emu.cpp - a continuation that reads a word it has not restored or
// recomputed reads what the test put there.
template <int KIND>
static void run(const MmpcParams *P, int B, const double *x_init, const double *traj_ref, const double *u_ref, const double *u_last,
                const double *x_guess, const double *obs, const long long *tick, double *X, double *U, double *s, int *status, int *iters,
                double *cost, double *err, int cont, int budget, double *state, int resume, double scale_max_grad, double *scale_out) {
    typedef MmpcDims<KIND> D;
    const int N = P->N, M = P->M;
    const MmpcLayout L = layout_of<KIND>(P);
    const int sd = mmpc_gen_state(D::NX, D::NU, N, L.R).total;
    const size_t so = P->obs_per_stage == 2 ? (size_t)M * 5 : (size_t)(P->obs_per_stage ? N + 1 : 1) * M * 3;
    MmpcEmuBlock lds_b, soc_b;
    for (int b = 0; b < B; b++) {
        if (resume && status[b] != 3) continue;
        double *lds = lds_b.next(L.total);
        double *soc = soc_b.next(mmpc_soc_doubles(N, D::NX, D::NU, L.NR));
        MmpcIO io;
        mmpc_instance_io<KIND>(io, *P, b, N, so, x_init, traj_ref, u_ref, u_last, x_guess, obs, X, U, s, status, iters, cost, err, soc, 0);
        if (P->obs_per_stage == 2 && tick) io.tick = tick + b;
        io.scale_max_grad = scale_max_grad; if (scale_out) io.scale_out = scale_out + b;
        const MmpcEmu emu = MmpcEmu{0, 64, 1};
        if (cont) {
            io.state = state ? state + (size_t)b * sd : nullptr; io.budget = budget; io.resume = resume;
            mmpc_solve_one<KIND, 0, -1, -1, -1, -1, true>(*P, io, lds, emu);
        } else
            mmpc_solve_one<KIND>(*P, io, lds, emu);
    }
}

extern "C" int mmpc_emug_solve(int kind, const MmpcParams *P, int B, const double *x_init, const double *traj_ref, const double *u_ref,
                               const double *u_last, const double *x_guess, const double *obs, const long long *tick, double *X, double *U,
                               double *s, int *status, int *iters, double *cost, double *err, int cont, int budget, double *state,
                               int resume, double scale_max_grad, double *scale_out) {
    if (kind < 0 || kind > 2 || (!cont && (budget || resume))) return -1;
#define MMPC_EMUG_ARGS P, B, x_init, traj_ref, u_ref, u_last, x_guess, obs, tick, X, U, s, status, iters, cost, err, cont, budget, state, resume, scale_max_grad, scale_out
    if (kind == 0) run<0>(MMPC_EMUG_ARGS); else if (kind == 1) run<1>(MMPC_EMUG_ARGS); else run<2>(MMPC_EMUG_ARGS);
#undef MMPC_EMUG_ARGS
    return 0;
}
// the save area's layout, from the kernel's own function: out[0..10] = X, U, S, LAM, T, Z, FILT, NUEQ, SIGW, SCAL, total
extern "C" int mmpc_emug_state_layout(int kind, const MmpcParams *P, int *out) {
    if (kind < 0 || kind > 2) return -1;
    const MmpcLayout L = kind == 0 ? layout_of<0>(P) : kind == 1 ? layout_of<1>(P) : layout_of<2>(P);
    const MmpcGenState g = mmpc_gen_state(kind == 1 ? 6 : 9, kind == 1 ? 2 : 5, P->N, L.R);
    const int v[11] = {g.X, g.U, g.S, g.LAM, g.T, g.Z, g.FILT, g.NUEQ, g.SIGW, g.SCAL, g.total};
    for (int i = 0; i < 11; i++) out[i] = v[i];
    return L.R;
}
extern "C" int mmpc_emug_params_size() { return (int)sizeof(MmpcParams); }
extern "C" int mmpc_emug_fcap() { return MMPC_FCAP; }
extern "C" int mmpc_emug_nscal() { return MMPC_GEN_NSCAL; }

#ifdef MMPC_EMUG_MAIN
// Stand-alone form (its own main, for a sanitizer build): a whole-body (12, 2) batch of four straight-line problems past an obstacle,
// solved uninterrupted and as a chain of one-iteration launches; exit status 0 when the two agree bit for bit.
#include <stdio.h>
int main() {
    enum { N = 12, M = 2, B = 4 };
    MmpcParams P;
    memset(&P, 0, sizeof(P));
    P.N = N; P.M = M; P.max_iter = 200; P.dt = 0.1; P.tol = 1e-8; P.mu_init = 1.0; P.S = 1e5;
    const double q[9] = {25, 25, 0, 0, 0, 5, 5, 5, 5}, r[5] = {0.1, 0.1, 0, 0, 0}, w[5] = {0, 0, 0.1, 0.1, 0.1};
    for (int i = 0; i < 9; i++) P.Q2[i * 9 + i] = P.P2[i * 9 + i] = 2 * q[i];
    for (int i = 0; i < 5; i++) { P.R2[i * 5 + i] = 2 * r[i]; P.W2[i * 5 + i] = 2 * w[i]; P.RW2[i * 5 + i] = 2 * r[i] + 2 * w[i]; }
    const double ul[5] = {2, 3.141592653589793, 1, 1, 1}, dl[5] = {INFINITY, INFINITY, 0.5, 0.5, 0.5};
    const double xlo[9] = {-100, -100, -INFINITY, -2, -2, -3.141592653589793, -1.5707963267948966, -3.141592653589793, 0};
    const double xhi[9] = {100, 100, INFINITY, 2, 2, 3.141592653589793, 1.5707963267948966, 0, 4.71238898038469};
    for (int j = 0; j < 5; j++) { P.ulim[0][j] = -ul[j]; P.ulim[1][j] = ul[j]; P.dulim[0][j] = -dl[j]; P.dulim[1][j] = dl[j]; }
    for (int j = 0; j < 9; j++) { P.xlim[0][j] = xlo[j]; P.xlim[1][j] = xhi[j]; }
    static double x0[B][9], ref[B][N + 1][9], uref[B][N][5], ulast[B][N][5], obs[B][M][3];
    for (int b = 0; b < B; b++) {
        const double x[9] = {0, 0.05 * b, 0.1 * b, 0.3, 0, 0, 0.2, -1.0, 1.0};
        for (int j = 0; j < 9; j++) x0[b][j] = x[j];
        for (int k = 0; k <= N; k++) { for (int j = 0; j < 9; j++) ref[b][k][j] = x[j]; ref[b][k][0] = 0.15 * k; ref[b][k][3] = 0; }
        obs[b][0][0] = 0.9; obs[b][0][1] = 0.1 - 0.05 * b; obs[b][0][2] = 0.3;
        obs[b][1][0] = 3.0; obs[b][1][1] = 3.0; obs[b][1][2] = 0.2;
    }
    int lay[11];
    mmpc_emug_state_layout(0, &P, lay);
    const int sd = lay[10];
    MmpcEmuBlock state_b;
    double *state = state_b.next((size_t)sd * B);
    static double X[2][B][N + 1][9], U[2][B][N][5], s[2][B][N + 1], cost[2][B], err[2][B];
    static int status[2][B], iters[2][B];
#define MMPC_EMUG_OUT(v) &X[v][0][0][0], &U[v][0][0][0], &s[v][0][0], status[v], iters[v], cost[v], err[v]
#define MMPC_EMUG_IN &x0[0][0], &ref[0][0][0], &uref[0][0][0], &ulast[0][0][0], nullptr, &obs[0][0][0], nullptr
    mmpc_emug_solve(0, &P, B, MMPC_EMUG_IN, MMPC_EMUG_OUT(0), 0, 0, nullptr, 0, 0.0, nullptr);
    int launches = 0;
    for (int resume = 0;; resume = 1) {
        mmpc_emug_solve(0, &P, B, MMPC_EMUG_IN, MMPC_EMUG_OUT(1), 1, 1, state, resume, 0.0, nullptr);
        launches++;
        bool any = false;
        for (int b = 0; b < B; b++) any = any || status[1][b] == 3;
        if (!any || launches > 1000) break;
    }
    const bool same = !memcmp(X[0], X[1], sizeof(X[0])) && !memcmp(U[0], U[1], sizeof(U[0])) && !memcmp(s[0], s[1], sizeof(s[0])) &&
                      !memcmp(cost[0], cost[1], sizeof(cost[0])) && !memcmp(err[0], err[1], sizeof(err[0])) &&
                      !memcmp(status[0], status[1], sizeof(status[0])) && !memcmp(iters[0], iters[1], sizeof(iters[0]));
    printf("launches %d, iterations %d %d %d %d, status %d %d %d %d: %s\n", launches, iters[0][0], iters[0][1], iters[0][2], iters[0][3],
           status[0][0], status[0][1], status[0][2], status[0][3], same ? "bitwise equal" : "DIFFERENT");
    return same ? 0 : 1;
}
#endif
