// mmpc_mission.h - the fleet tick of mmpc_tick.h with the reference's task state machine per robot, one 64-lane workgroup per robot.
//
// The reference's closed loop is a state machine (interface_wholebody_qref.py:146-228): 'move' tracks the nearest window of the
// global plan, 'approach' (inside the 2 m box around the goal) and 'rotate' (within 0.2 m) hold the goal pose (calcLocalRefPose,
// :398-410), 'move finish' ends the drive.  The phase decides the reference here and the handle (terminal equality, weights) in
// the driver (fleet.py:DeviceFleet.run_mission), so this kernel also writes, per phase, the list of the robots to solve:
// mmpc_solve_rows_device takes such a list on either kernel family.
//
// Same shared-source style as mmpc_tick.h (hipcc for gfx950, g++ -DMMPC_EMU -ffp-contract=off for the host: tests/mission_emu),
// whose pieces it uses unchanged: clip, plant step, distance, the arg-min tree over the same LDS slots, stage time and obstacle
// centre.  State in memory (x, tick, phase) is read in the first phases and written in the last one.
//
// Arithmetic: as in mmpc_tick.h, every operation rounded on its own (`#pragma clang fp contract(off)`).  The one new piece is
// MPCWholeBody.angleDiff, operation by operation: fmod(a + pi, 2 pi) - pi of both arguments, then the sign cases.  fmod is exact
// (its result is always representable), so host and device agree bit for bit.
#pragma once
#include "mmpc_tick.h"
#include "../../include/mmpc.h"

#define MMPC_MISSION_PI 3.141592653589793
// 0.5 * np.pi / 180, left to right (interface_wholebody_qref.py:194)
#define MMPC_MISSION_ANGLE_TOL (0.5 * MMPC_MISSION_PI / 180)

struct MmpcMissionIO {
    MmpcTickIO t;            // x, tick, U_prev, glob (required), obs0, vel, x_in, traj_ref, start, obs; no warm-start outputs
    int *phase;              // [1]   in/out: the phase the robot was last solved in (MMPC_PHASE_*)
    int *lists;              // [3][B] rows to solve per phase
    int *counts;             // [4]   robots per phase (zeroed before the launch)
    int b, B;
};

#ifdef MMPC_EMU
inline int mmpc_mission_take(int *c) { return (*c)++; }
#else
__device__ __forceinline__ int mmpc_mission_take(int *c) { return atomicAdd(c, 1); }
#endif

// the first line of angleDiff for one argument
MMPC_DEV double mmpc_mission_wrap(double a) {
#pragma clang fp contract(off)
    return fmod(a + MMPC_MISSION_PI, 2 * MMPC_MISSION_PI) - MMPC_MISSION_PI;
}
// ... and its remainder, on wrapped arguments (mpc_wholebody_qref.py:92-117)
MMPC_DEV double mmpc_mission_diff(double a, double b) {
#pragma clang fp contract(off)
    const double d = a - b;
    if (a * b >= 0) return d;
    if (a > b) return d <= MMPC_MISSION_PI ? d : d - 2 * MMPC_MISSION_PI;
    return d > -MMPC_MISSION_PI ? d : d + 2 * MMPC_MISSION_PI;
}

MMPC_DEV void mmpc_mission_one(const MmpcParams &P, const MmpcMissionIO mio, double *lds MMPC_EMU_ARG) {
#pragma clang fp contract(off)
    const MmpcTickIO &io = mio.t;
    const int N = P.N, M = P.M;
    const double dt = P.dt;
    int p = mio.phase[0];
    // a finished robot is frozen: nothing of it is read for output or written (a code outside 0..3 counts as finished)
    if ((unsigned)p >= (unsigned)MMPC_PHASE_DONE) {
        LANES_BEGIN
        if (lane == 0) mmpc_mission_take(mio.counts + MMPC_PHASE_DONE);
        LANES_END
        return;
    }
    const bool adv = io.U_prev != nullptr;
    // ---- 1. advance: x <- f(clip(x), U_prev[0]), as mmpc_tick_one
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
    // ---- 2. state machine on the unclipped state (stateMachineUpdate, :153-197; every lane the same: a comparison with a NaN is
    //         false, so a non-finite robot keeps its phase)
    const double *g = io.glob + (size_t)(io.nglob - 1) * 9;
    const double px = lds[MMPC_TICK_XS], py = lds[MMPC_TICK_XS + 1], psi = lds[MMPC_TICK_XS + 2];
    const double d = mmpc_tick_dist(px, py, g);
    const double wx = mmpc_mission_wrap(psi), wg = mmpc_mission_wrap(g[2]);
    if (p == MMPC_PHASE_MOVE && fabs(px - g[0]) <= 2 && fabs(py - g[1]) <= 2) p = MMPC_PHASE_APPROACH;
    if (p <= MMPC_PHASE_APPROACH && d <= 0.2) p = MMPC_PHASE_ROTATE;
    if (p == MMPC_PHASE_ROTATE && fabs(mmpc_mission_diff(wx, wg)) <= MMPC_MISSION_ANGLE_TOL && d <= 0.01) p = MMPC_PHASE_DONE;
    const bool live = p != MMPC_PHASE_DONE, window = p == MMPC_PHASE_MOVE;
    // ---- 3. x_in; move: nearest plan row (per-lane first minimum, then the wave arg-min of mmpc_tick_one)
    LANES_BEGIN
    if (live && io.x_in && lane < 9) io.x_in[lane] = lds[MMPC_TICK_XI + lane];
    if (window) {
        double bd = INFINITY, bj = MMPC_TICK_NOROW;
        for (int j = lane; j < io.nglob; j += MMPC_WAVE) {
            const double dj = mmpc_tick_dist(px, py, io.glob + (size_t)j * 9);
            if (dj < bd) { bd = dj; bj = (double)j; }
        }
        lds[MMPC_TICK_RD + lane] = bd;
        lds[MMPC_TICK_RJ + lane] = bj;
    }
    LANES_END
    int start = io.nglob - 1;
    if (window) {
        for (int s = MMPC_WAVE / 2; s >= 1; s >>= 1) {
            LANES_BEGIN
            if (lane < s) {
                const double d1 = lds[MMPC_TICK_RD + lane], j1 = lds[MMPC_TICK_RJ + lane];
                const double d2 = lds[MMPC_TICK_RD + lane + s], j2 = lds[MMPC_TICK_RJ + lane + s];
                if (d2 < d1 || (d2 == d1 && j2 < j1)) { lds[MMPC_TICK_RD + lane] = d2; lds[MMPC_TICK_RJ + lane] = j2; }
            }
            LANES_END
        }
        const double jw = lds[MMPC_TICK_RJ];
        start = jw < (double)io.nglob ? (int)jw : 0;
    }
    // approach, rotate: the goal with its heading made continuous with the robot's (calcLocalRefPose: psi + angleDiff(psi_ref, psi))
    const double hold = psi + mmpc_mission_diff(wg, wx);
    // ---- 4. reference, 5. obstacle table
    const long long tick = io.tick ? io.tick[0] + (adv ? 1 : 0) : 0;
    LANES_BEGIN
    if (live) {
        if (io.start && lane == 0) io.start[0] = start;
        if (io.traj_ref)
            for (int i = lane; i < 9 * (N + 1); i += MMPC_WAVE) {
                const int k = i / 9, c = i - 9 * k;
                const int r = start + k < io.nglob - 1 ? start + k : io.nglob - 1;
                io.traj_ref[i] = (!window && c == 2) ? hold : io.glob[(size_t)r * 9 + c];
            }
        if (io.obs)
            for (int i = lane; i < M * (N + 1); i += MMPC_WAVE) {
                const int k = i / M, m = i - M * k;
                const double t = mmpc_tick_time(tick, k, dt);
                io.obs[(size_t)i * 3] = mmpc_tick_centre(io.obs0[3 * m], io.vel[2 * m], t);
                io.obs[(size_t)i * 3 + 1] = mmpc_tick_centre(io.obs0[3 * m + 1], io.vel[2 * m + 1], t);
                io.obs[(size_t)i * 3 + 2] = io.obs0[3 * m + 2];
            }
    }
    LANES_END
    // ---- the state, the tick counter and the phase in memory; the robot's entry in its phase's list
    LANES_BEGIN
    if (adv) {
        if (lane < 9) io.x[lane] = lds[MMPC_TICK_XS + lane];
        if (lane == 0) io.tick[0] = tick;
    }
    if (lane == 0) {
        mio.phase[0] = p;
        const int at = mmpc_mission_take(mio.counts + p);
        if (live && at < mio.B) mio.lists[(size_t)p * mio.B + at] = mio.b;
    }
    LANES_END
}

// robot b of the batch arrays of mmpc_mission_prepare_device (include/mmpc.h); a null array stays null
MMPC_DEV void mmpc_mission_robot(const MmpcParams &P, int b, int B, double *x, long long *tick, int *phase, const double *U_prev,
                                 const double *glob, int nglob, const double *obs0, const double *vel, double *x_in, double *traj_ref,
                                 int *start, double *obs, int *lists, int *counts, double *lds MMPC_EMU_ARG) {
    const size_t N = (size_t)P.N, M = (size_t)P.M, r = (size_t)b;
    MmpcMissionIO mio;
    MmpcTickIO &io = mio.t;
    io.x = x + r * 9;
    io.tick = tick ? tick + r : nullptr;
    io.U_prev = U_prev ? U_prev + r * N * 5 : nullptr;
    io.glob = glob + r * (size_t)nglob * 9;
    io.nglob = nglob;
    io.obs0 = obs0 ? obs0 + r * M * 3 : nullptr;
    io.vel = vel ? vel + r * M * 2 : nullptr;
    io.x_in = x_in ? x_in + r * 9 : nullptr;
    io.traj_ref = traj_ref ? traj_ref + r * (N + 1) * 9 : nullptr;
    io.start = start ? start + r : nullptr;
    io.obs = (obs && M > 0) ? obs + r * (N + 1) * M * 3 : nullptr;
    io.u_guess = nullptr;
    io.x_guess = nullptr;
    mio.phase = phase + r;
    mio.lists = lists;
    mio.counts = counts;
    mio.b = b;
    mio.B = B;
#ifdef MMPC_EMU
    mmpc_mission_one(P, mio, lds, emu);
#else
    mmpc_mission_one(P, mio, lds);
#endif
}
