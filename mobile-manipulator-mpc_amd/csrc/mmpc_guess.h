// mmpc_guess.h - the shifted warm start of a fleet whose robots are not all solved by one handle, one 64-lane workgroup per robot.
//
// The tick kernel (mmpc_tick.h) forms the engine's opt-in initial point in its step 6: the previous optimum shifted one stage and
// the roll-out of the plant under it from the solve's x_init.  A mission (mmpc_mission.h, mmpc_manipulate.h) has two kernels that
// write x_in, one per group of phases, and neither writes a guess.  This kernel runs after both, on the x_in they left, and writes
// the same initial point for the robots that are solved in this tick - those whose phase is MOVE, APPROACH, ROTATE or MANIPULATE,
// the codes that appear in a solve list.  Nothing of any other robot is read or written.
//
// Same shared-source style as mmpc_tick.h (hipcc for gfx950, g++ -DMMPC_EMU -ffp-contract=off for the host: tests/guess_emu), whose
// plant step it uses unchanged: the operations are those of step 6 of mmpc_tick_one on the same pieces, so on one machine the two
// agree bit for bit.  x_in is read from memory (the tick kernel keeps it in LDS): no LDS here.  The roll-out reads U_prev, never
// u_guess, which other lanes of the same phase write.
#pragma once
#include "mmpc_tick.h"
#include "../../include/mmpc.h"

// the phases a mission solves a robot in
MMPC_DEV bool mmpc_guess_solved(int p) {
    return p == MMPC_PHASE_MOVE || p == MMPC_PHASE_APPROACH || p == MMPC_PHASE_ROTATE || p == MMPC_PHASE_MANIPULATE;
}

// one robot: U_prev [N][5], x_in [9] -> u_guess [N][5], x_guess [N+1][9]
MMPC_DEV void mmpc_guess_one(int N, double dt, const double *U_prev, const double *x_in, double *u_guess, double *x_guess MMPC_EMU_ARG) {
    LANES_BEGIN
    // u_guess[k] = U_prev[k + 1], the last row twice
    for (int i = lane; i < 5 * N; i += MMPC_WAVE) {
        const int k = i / 5, a = i - 5 * k;
        u_guess[i] = U_prev[(k + 1 < N ? k + 1 : N - 1) * 5 + a];
    }
    // x_guess = the roll-out of the plant under it from x_in: a serial chain of N steps on one lane
    if (lane == 0) {
        double xk[9], xn[9];
        for (int i = 0; i < 9; i++) { xk[i] = x_in[i]; x_guess[i] = xk[i]; }
        for (int k = 0; k < N; k++) {
            mmpc_tick_plant(dt, xk, U_prev + (k + 1 < N ? k + 1 : N - 1) * 5, xn);
            for (int i = 0; i < 9; i++) { xk[i] = xn[i]; x_guess[(k + 1) * 9 + i] = xn[i]; }
        }
    }
    LANES_END
}

// robot b of the batch arrays of mmpc_shift_guess_device (include/mmpc.h); phase may be null (every row)
MMPC_DEV void mmpc_guess_robot(const MmpcParams &P, int b, const int *phase, const double *U_prev, const double *x_in, double *u_guess,
                               double *x_guess MMPC_EMU_ARG) {
    const size_t N = (size_t)P.N, r = (size_t)b;
    if (phase && !mmpc_guess_solved(phase[r])) return;
#ifdef MMPC_EMU
    mmpc_guess_one(P.N, P.dt, U_prev + r * N * 5, x_in + r * 9, u_guess + r * N * 5, x_guess + r * (N + 1) * 9, emu);
#else
    mmpc_guess_one(P.N, P.dt, U_prev + r * N * 5, x_in + r * 9, u_guess + r * N * 5, x_guess + r * (N + 1) * 9);
#endif
}
