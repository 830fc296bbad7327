// mmpc_tick.h - what a receding-horizon fleet does between two solves, one 64-lane workgroup per robot.
//
// Replaces, for the whole-body kind with a per-stage obstacle table, the torch glue of fleet.py:DeviceFleet.plant / .inputs and the
// host loop that builds the shifted warm start (bench.py:run_all(shifted=True)): the reference's closed loop without the simulator
// (interface_wholebody_qref.py:100-143) - plant step x <- f(clip(x), u0) (:143, robot_models/base.py:17-31), nearest point of the
// global plan and the window of N + 1 rows behind it (calcLocalRefTraj, :353-396), plus the build's moving-obstacle table
// c + v (tick + k) dt and the engine's opt-in initial point (previous optimum shifted one stage, its roll-out).
//
// Shared source in the style of mmpc_core.h: phases of lane work separated by LANES_END, compiled by hipcc for gfx950 and by
// g++ -DMMPC_EMU (tests/tick_emu).  In-place data (x, tick) is read in the first phases and written in the last one, so that a
// phase never reads what another lane of the same phase writes.
//
// Arithmetic: every operation of the plant step, of the distance and of the obstacle table is rounded on its own, in the order of
// the numpy / torch expressions it replaces - `#pragma clang fp contract(off)` in every function (hipcc contracts a * b + c into
// an FMA by default; the host build passes -ffp-contract=off).  sin / cos are mmpc_sincos (mmpc_core.h: <= 2 ulp for |x| <= 8, its
// explicit fma calls are part of its definition and give the same bits on host and device).
#pragma once
#include "mmpc_core.h"

struct MmpcTickIO {
    double *x;               // [9]      in/out: the robot's state (unclipped)
    long long *tick;         // [1]      in/out: ticks taken so far
    const double *U_prev;    // [N][5]   the previous optimum (null: no advance, no warm start)
    const double *glob;      // [nglob][9] global plan
    int nglob;
    const double *obs0, *vel;   // [M][3] centres + radius at tick 0, [M][2] velocities
    double *x_in;            // [9]      clip(x): x_init of the solve
    double *traj_ref;        // [N+1][9] window
    int *start;              // [1]      index of the nearest plan row
    double *obs;             // [N+1][M][3]
    double *u_guess;         // [N][5]
    double *x_guess;         // [N+1][9]
};

// LDS of one robot (doubles)
#define MMPC_TICK_XC 0      // clip(x) before the advance [9]
#define MMPC_TICK_XS 9      // the state after the advance, unclipped [9]
#define MMPC_TICK_XI 18     // its clip = x_in [9]
#define MMPC_TICK_RD 27     // arg-min partials: distance [64] ...
#define MMPC_TICK_RJ (27 + MMPC_WAVE)   // ... and plan row [64]
#define MMPC_TICK_LDS (27 + 2 * MMPC_WAVE)
#define MMPC_TICK_NOROW 2147483647.0    // partial of a lane that found no row

// np.clip / torch.minimum(torch.maximum()): a NaN stays a NaN (fmin / fmax would return the bound)
MMPC_DEV double mmpc_tick_clip(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// robot_models/mobile_manipulator.py:f_kinematics = base.py:f_kinematics ++ q + dq dt, operation by operation
MMPC_DEV void mmpc_tick_plant(double dt, const double *x, const double *u, double *o) {
#pragma clang fp contract(off)
    double sn, cs;
    mmpc_sincos(x[2], &sn, &cs);
    const double x3 = x[3], x4 = x[4], x5 = x[5];
    o[0] = x[0] + dt * x3;
    o[1] = x[1] + dt * x4;
    o[2] = x[2] + dt * x5;
    o[3] = x3 + dt * (u[0] * cs - x4 * x5);
    o[4] = x4 + dt * (u[0] * sn + x3 * x5);
    o[5] = x5 + dt * u[1];
    o[6] = x[6] + dt * u[2];
    o[7] = x[7] + dt * u[3];
    o[8] = x[8] + dt * u[4];
}

// |(x, y) - plan row|, as np.linalg.norm over two components: sqrt(dx dx + dy dy)
MMPC_DEV double mmpc_tick_dist(double px, double py, const double *row) {
#pragma clang fp contract(off)
    const double dx = px - row[0], dy = py - row[1];
    return sqrt(dx * dx + dy * dy);
}

// (centre of an obstacle at time t and the time of stage k: mmpc_tick_centre, mmpc_tick_time of mmpc_core.h, which the solver
//  kernels' motion mode shares)

MMPC_DEV void mmpc_tick_one(const MmpcParams &P, const MmpcTickIO io, double *lds MMPC_EMU_ARG) {
    const int N = P.N, M = P.M;
    const double dt = P.dt;
    const bool adv = io.U_prev != nullptr;
    // ---- 1. advance: x <- f(clip(x), U_prev[0]) (into LDS; the state in memory is replaced in the last phase)
    LANES_BEGIN
    if (lane < 9) lds[MMPC_TICK_XC + lane] = mmpc_tick_clip(io.x[lane], P.xlim[0][lane], P.xlim[1][lane]);
    LANES_END
    LANES_BEGIN
    if (adv) {
        if (lane == 0) {
            double o[9];
            mmpc_tick_plant(dt, lds + MMPC_TICK_XC, io.U_prev, o);
            for (int i = 0; i < 9; i++) {
                lds[MMPC_TICK_XS + i] = o[i];
                lds[MMPC_TICK_XI + i] = mmpc_tick_clip(o[i], P.xlim[0][i], P.xlim[1][i]);
            }
        }
    } else if (lane < 9) {
        lds[MMPC_TICK_XS + lane] = io.x[lane];
        lds[MMPC_TICK_XI + lane] = lds[MMPC_TICK_XC + lane];
    }
    LANES_END
    // ---- 2. x_in; 3. nearest plan row: per-lane first minimum over the rows lane, lane + 64, ... (strict '<': calcLocalRefTraj)
    LANES_BEGIN
    if (io.x_in && lane < 9) io.x_in[lane] = lds[MMPC_TICK_XI + lane];
    if (io.glob) {
        const double px = lds[MMPC_TICK_XS], py = lds[MMPC_TICK_XS + 1];
        double bd = INFINITY, bj = MMPC_TICK_NOROW;
        for (int j = lane; j < io.nglob; j += MMPC_WAVE) {
            const double d = mmpc_tick_dist(px, py, io.glob + (size_t)j * 9);
            if (d < bd) { bd = d; bj = (double)j; }
        }
        lds[MMPC_TICK_RD + lane] = bd;
        lds[MMPC_TICK_RJ + lane] = bj;
    }
    LANES_END
    int start = 0;
    if (io.glob) {
        // wave arg-min, the lower row wins a tie (lane l < s takes the better of its pair and lane l + s's: nobody writes what
        // another lane of the phase reads)
        for (int s = MMPC_WAVE / 2; s >= 1; s >>= 1) {
            LANES_BEGIN
            if (lane < s) {
                const double d1 = lds[MMPC_TICK_RD + lane], j1 = lds[MMPC_TICK_RJ + lane];
                const double d2 = lds[MMPC_TICK_RD + lane + s], j2 = lds[MMPC_TICK_RJ + lane + s];
                if (d2 < d1 || (d2 == d1 && j2 < j1)) { lds[MMPC_TICK_RD + lane] = d2; lds[MMPC_TICK_RJ + lane] = j2; }
            }
            LANES_END
        }
        // (no row compares below +inf when the state is not finite: row 0, and the NaN reaches the solve through x_in)
        const double jw = lds[MMPC_TICK_RJ];
        start = jw < (double)io.nglob ? (int)jw : 0;
    }
    // ---- 4. window, 5. obstacle table, 6. shifted warm start
    const long long tick = io.tick ? io.tick[0] + (adv ? 1 : 0) : 0;
    LANES_BEGIN
    if (io.start && lane == 0) io.start[0] = start;
    if (io.traj_ref)
        for (int i = lane; i < 9 * (N + 1); i += MMPC_WAVE) {
            const int k = i / 9, c = i - 9 * k;
            const int r = start + k < io.nglob - 1 ? start + k : io.nglob - 1;
            io.traj_ref[i] = io.glob[(size_t)r * 9 + c];
        }
    if (io.obs)
        for (int i = lane; i < M * (N + 1); i += MMPC_WAVE) {
            const int k = i / M, m = i - M * k;
            const double t = mmpc_tick_time(tick, k, dt);
            io.obs[(size_t)i * 3] = mmpc_tick_centre(io.obs0[3 * m], io.vel[2 * m], t);
            io.obs[(size_t)i * 3 + 1] = mmpc_tick_centre(io.obs0[3 * m + 1], io.vel[2 * m + 1], t);
            io.obs[(size_t)i * 3 + 2] = io.obs0[3 * m + 2];
        }
    if (adv && io.u_guess && io.x_guess) {
        // u_guess[k] = U_prev[k + 1], the last row twice; x_guess = the roll-out of the plant under it from x_in (a serial chain of
        // N steps on one lane, reading U_prev: u_guess is only written here)
        for (int i = lane; i < 5 * N; i += MMPC_WAVE) {
            const int k = i / 5, a = i - 5 * k;
            io.u_guess[i] = io.U_prev[(k + 1 < N ? k + 1 : N - 1) * 5 + a];
        }
        if (lane == 0) {
            double xk[9], xn[9];
            for (int i = 0; i < 9; i++) { xk[i] = lds[MMPC_TICK_XI + i]; io.x_guess[i] = xk[i]; }
            for (int k = 0; k < N; k++) {
                mmpc_tick_plant(dt, xk, io.U_prev + (k + 1 < N ? k + 1 : N - 1) * 5, xn);
                for (int i = 0; i < 9; i++) { xk[i] = xn[i]; io.x_guess[(k + 1) * 9 + i] = xn[i]; }
            }
        }
    }
    LANES_END
    // ---- the state and the tick counter in memory
    LANES_BEGIN
    if (adv) {
        if (lane < 9) io.x[lane] = lds[MMPC_TICK_XS + lane];
        if (lane == 0) io.tick[0] = tick;
    }
    LANES_END
}

// robot b of the batch arrays of mmpc_tick_prepare_device (include/mmpc.h); a null array stays null
MMPC_DEV void mmpc_tick_robot(const MmpcParams &P, int b, double *x, long long *tick, const double *U_prev, const double *glob, int nglob,
                              const double *obs0, const double *vel, double *x_in, double *traj_ref, int *start, double *obs,
                              double *u_guess, double *x_guess, double *lds MMPC_EMU_ARG) {
    const size_t N = (size_t)P.N, M = (size_t)P.M, r = (size_t)b;
    MmpcTickIO io;
    io.x = x + r * 9;
    io.tick = tick ? tick + r : nullptr;
    io.U_prev = U_prev ? U_prev + r * N * 5 : nullptr;
    io.glob = glob ? glob + r * (size_t)nglob * 9 : nullptr;
    io.nglob = glob ? nglob : 0;
    io.obs0 = obs0 ? obs0 + r * M * 3 : nullptr;
    io.vel = vel ? vel + r * M * 2 : nullptr;
    io.x_in = x_in ? x_in + r * 9 : nullptr;
    io.traj_ref = traj_ref ? traj_ref + r * (N + 1) * 9 : nullptr;
    io.start = start ? start + r : nullptr;
    io.obs = (obs && M > 0) ? obs + r * (N + 1) * M * 3 : nullptr;
    const bool warm = U_prev && u_guess && x_guess;      // the warm start is all or nothing
    io.u_guess = warm ? u_guess + r * N * 5 : nullptr;
    io.x_guess = warm ? x_guess + r * (N + 1) * 9 : nullptr;
#ifdef MMPC_EMU
    mmpc_tick_one(P, io, lds, emu);
#else
    mmpc_tick_one(P, io, lds);
#endif
}
