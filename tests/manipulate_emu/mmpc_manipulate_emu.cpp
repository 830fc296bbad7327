// Host lane-emulation build of the fleet manipulate kernel (TEST ONLY - never part of the product).
// Compiles mobile-manipulator-mpc_amd/csrc/mmpc_manipulate.h with -DMMPC_EMU -ffp-contract=off: every phase is a loop over the 64
// lanes; `reverse` runs the lanes of every phase in the opposite order (a result that changes exposes an intra-phase race) and the
// robots in the opposite order too (the list may come in any order).  The arguments are those of mmpc_manipulate_prepare_device,
// with the handle replaced by what the kernel reads of it; the counts are zeroed here, as the entry point does before its launch.
#define MMPC_EMU 1
#include "../emu_common/mmpc_emu_poison.h"
#include "../../mobile-manipulator-mpc_amd/csrc/mmpc_manipulate.h"
#include <stdlib.h>

extern "C" int mmpc_manipulate_emu_lds_doubles() { return MMPC_TICK_LDS; }

// the endpoint the finish test compares with the pose target, for one state
extern "C" void mmpc_manipulate_emu_endpoint(const double *x, double *e) { mmpc_manip_endpoint(x, e); }

// the endpoint target in the arm frame that the transition hands to the inverse kinematics, for one state and pose target
extern "C" void mmpc_manipulate_emu_target(const double *x, const double *g, double *t) { mmpc_manip_target(x, g, t, t + 1); }

extern "C" int mmpc_manipulate_emu_prepare(int N, int M, double dt, const double *xlim, int B, double *x, long long *tick, int *phase,
                                           const double *U_prev, const double *pose, int nplan, double *plan, double *qgoal,
                                           int *ik_status, const double *obs0, const double *vel, double *x_in, double *traj_ref,
                                           int *start, double *obs, int *list, int *counts, int reverse) {
    MmpcParams *P = (MmpcParams *)calloc(1, sizeof(MmpcParams));
    P->N = N; P->M = M; P->obs_per_stage = 1; P->dt = dt;
    for (int r = 0; r < 2; r++) for (int j = 0; j < 9; j++) P->xlim[r][j] = xlim[r * 9 + j];
    for (int i = 0; i < 2; i++) counts[i] = 0;
    MmpcEmuBlock lds_b;   // (mmpc_emu_poison.h: what the slab holds at the start of a robot is the caller's choice, NaN by default)
    for (int i = 0; i < B; i++) {
        const int b = reverse ? B - 1 - i : i;
        // exact-size heap slab so that a sanitizer build sees any access outside it
        double *lds = lds_b.next(MMPC_TICK_LDS);
        MmpcEmu emu = reverse ? MmpcEmu{63, -1, -1} : MmpcEmu{0, 64, 1};
        mmpc_manipulate_robot(*P, b, B, x, tick, phase, U_prev, pose, nplan, plan, qgoal, ik_status, obs0, vel, x_in, traj_ref, start, obs,
                              list, counts, lds, emu);
    }
    free(P);
    return 0;
}
