// Host lane-emulation build of the mission's warm-start kernel (TEST ONLY - never part of the product).
// Compiles mobile-manipulator-mpc_amd/csrc/mmpc_guess.h with -DMMPC_EMU -ffp-contract=off: the kernel's one phase is a loop over
// the 64 lanes; `reverse` runs them in the opposite order (a result that changes exposes an intra-phase race).
// The arguments are those of mmpc_shift_guess_device, with the handle replaced by what the kernel reads of it.
#define MMPC_EMU 1
#include "../../mobile-manipulator-mpc_amd/csrc/mmpc_guess.h"
#include <stdlib.h>

extern "C" int mmpc_guess_emu_shift(int N, double dt, int B, const int *phase, const double *U_prev, const double *x_in, double *u_guess,
                                    double *x_guess, int reverse) {
    MmpcParams *P = (MmpcParams *)calloc(1, sizeof(MmpcParams));
    P->N = N; P->dt = dt;
    for (int b = 0; b < B; b++) {
        MmpcEmu emu = reverse ? MmpcEmu{63, -1, -1} : MmpcEmu{0, 64, 1};
        mmpc_guess_robot(*P, b, phase, U_prev, x_in, u_guess, x_guess, emu);
    }
    free(P);
    return 0;
}
