// mmpc_manipulate.h - the manipulate phase of a fleet mission, one 64-lane workgroup per robot: what the reference's state machine
// does from 'move finish' on (interface_wholebody_qref.py:204-226).
//
// The mission kernel (mmpc_mission.h) drives a robot up to MMPC_PHASE_DONE ('move finish') and freezes it there.  This kernel runs
// after it in every tick and takes the robot on: at the transition it forms the endpoint target in the arm frame (:205-209), solves
// the arm's inverse kinematics (mmpc_ik.h, on lane 0), writes the joint-space line to the answer (globalPlanManipulator, :269-295:
// np.linspace(state, (state[:6], q_goal), T + 1)) and moves the robot to MMPC_PHASE_MANIPULATE; from then on it advances the robot
// itself, tests the finish condition (:219-223: the endpoint within 1 cm of its pose target => MMPC_PHASE_MANIP_DONE) and writes the
// window of the plan behind its nearest row in the joint columns (calcLocalRefTraj([6, 7, 8])), and the list of the robots to
// solve on the manipulate handle (terminal equality, weights diag(500, 500, 500, 0, 0, 1, 1, 1, 1): fleet.py).
//
// Same shared-source style as mmpc_mission.h (hipcc for gfx950, g++ -DMMPC_EMU -ffp-contract=off for the host:
// tests/manipulate_emu), on the LDS slots of mmpc_tick.h, whose clip, plant step, stage time, obstacle centre and arg-min tree it
// uses unchanged.  MMPC_TICK_XC is free once the advance is done: at the transition it holds the plan's last row.  State in memory
// (x, tick, phase) is read in the first phases and written in the last one; the plan of a robot in transition is written from LDS
// and every later phase of the same call forms its rows from LDS again, so no phase reads memory that the call wrote.
//
// Arithmetic: every operation rounded on its own (`#pragma clang fp contract(off)`), in the order of the numpy expressions.  A plan
// row is (j / T) (target - start) + start, which is np.linspace whenever a column has zero difference (columns 0..5 always have),
// the last row the target itself.  The endpoint's sin / cos are mmpc_sincos; the inverse kinematics uses the library sin / cos, so
// its answer is the host build's to solver accuracy, not bit for bit.
#pragma once
#include "mmpc_tick.h"
#include "mmpc_ik.h"
#include "../../include/mmpc.h"

struct MmpcManipIO {
    MmpcTickIO t;            // x, tick, U_prev, obs0, vel, x_in, traj_ref, start, obs; no global plan, no warm-start outputs
    int *phase;              // [1]   in/out (MMPC_PHASE_*)
    const double *pose;      // [4]   pose target of the endpoint: x, y, z, psi
    double *plan;            // [nplan][9] joint-space plan: written at the transition, read afterwards
    int nplan;
    double *qgoal;           // [3]   the IK's answer (may be null)
    int *ik_status;          // [1]   MMPC_IK_* (may be null)
    int *list;               // [B]   rows to solve
    int *counts;             // [2]   robots in MANIPULATE, robots in MANIP_DONE (zeroed before the launch)
    int b, B;
};

#ifdef MMPC_EMU
inline int mmpc_manip_take(int *c) { return (*c)++; }
#else
__device__ __forceinline__ int mmpc_manip_take(int *c) { return atomicAdd(c, 1); }
#endif

// row j, column c of np.linspace(s, g, T + 1)
MMPC_DEV double mmpc_manip_row(int j, int c, int T, const double *s, const double *g) {
#pragma clang fp contract(off)
    if (j >= T) return g[c];
    return ((double)j / (double)T) * (g[c] - s[c]) + s[c];
}

// world position of the endpoint (robot_models/mobile_manipulator.py:forward_tranformation): the arm's reach r and height z from its
// three segments, lifted by the base pose
MMPC_DEV void mmpc_manip_endpoint(const double *x, double e[3]) {
#pragma clang fp contract(off)
    double dr[3], dz[3], sn, cs;
    mmpc_arm_segments(x[6], x[7], x[8], dr, dz);
    mmpc_sincos(x[2], &sn, &cs);
    const double r = dr[0] + dr[1] + dr[2], z = dz[0] + dz[1] + dz[2];
    e[0] = x[0] + (r + MMPC_BX) * cs;
    e[1] = x[1] + (r + MMPC_BX) * sn;
    e[2] = z + MMPC_BZ;
}

// the endpoint target in the arm frame (:205-209): range + the 0.007 base-link offset, height above joint 1
MMPC_DEV void mmpc_manip_target(const double *x, const double *g, double *tx, double *tz) {
#pragma clang fp contract(off)
    const double dx = g[0] - x[0], dy = g[1] - x[1];
    *tx = sqrt(dx * dx + dy * dy) + 0.007;
    *tz = g[2] - MMPC_BZ;
}

// |e - g| over three components, as np.linalg.norm: sqrt(d0 d0 + d1 d1 + d2 d2)
MMPC_DEV double mmpc_manip_dist3(double a0, double a1, double a2, double b0, double b1, double b2) {
#pragma clang fp contract(off)
    const double d0 = a0 - b0, d1 = a1 - b1, d2 = a2 - b2;
    return sqrt(d0 * d0 + d1 * d1 + d2 * d2);
}

MMPC_DEV void mmpc_manipulate_one(const MmpcParams &P, const MmpcManipIO mio, double *lds MMPC_EMU_ARG) {
#pragma clang fp contract(off)
    const MmpcTickIO &io = mio.t;
    const int N = P.N, M = P.M, nplan = mio.nplan, T = mio.nplan - 1;
    const double dt = P.dt;
    int p = mio.phase[0];
    // a robot that still drives (< 3) is the mission kernel's, a finished one (5) is frozen: nothing of either is read for output
    // or written
    if (p != MMPC_PHASE_DONE && p != MMPC_PHASE_MANIPULATE) {
        LANES_BEGIN
        if (lane == 0 && p == MMPC_PHASE_MANIP_DONE) mmpc_manip_take(mio.counts + 1);
        LANES_END
        return;
    }
    // a robot that comes in at 'move finish' was advanced by the mission kernel in this tick
    const bool fresh = p == MMPC_PHASE_DONE;
    const bool adv = io.U_prev != nullptr && !fresh;
    // ---- 1. advance: x <- f(clip(x), U_prev[0]), as mmpc_mission_one
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
    const double *xs = lds + MMPC_TICK_XS, *g = mio.pose;
    // ---- 2. the transition (:204-216, on the unclipped state): endpoint target in the arm frame, inverse kinematics, the plan.  A
    //         failed solve does not stop the robot: the plan goes to the point the solver returned, the status says so
    if (fresh) {
        LANES_BEGIN
        if (lane == 0) {
            double tx, tz;
            mmpc_manip_target(xs, g, &tx, &tz);
            const double q0[3] = {xs[6], xs[7], xs[8]};
            double q[3];
            const int st = mmpc_ik_solve(q0, tx, tz, q, nullptr);
            // the plan's last row, in the slots the advance no longer needs
            for (int i = 0; i < 6; i++) lds[MMPC_TICK_XC + i] = xs[i];
            for (int i = 0; i < 3; i++) lds[MMPC_TICK_XC + 6 + i] = q[i];
            if (mio.qgoal) for (int i = 0; i < 3; i++) mio.qgoal[i] = q[i];
            if (mio.ik_status) mio.ik_status[0] = st;
        }
        LANES_END
        LANES_BEGIN
        for (int i = lane; i < 9 * nplan; i += MMPC_WAVE) {
            const int j = i / 9, c = i - 9 * j;
            mio.plan[i] = mmpc_manip_row(j, c, T, xs, lds + MMPC_TICK_XC);
        }
        LANES_END
        p = MMPC_PHASE_MANIPULATE;
    }
    // ---- 3. finish test (:219-223; every lane the same: a comparison with a NaN is false, so a non-finite robot keeps its phase)
    double e[3];
    mmpc_manip_endpoint(xs, e);
    if (mmpc_manip_dist3(e[0], e[1], e[2], g[0], g[1], g[2]) <= 0.01) p = MMPC_PHASE_MANIP_DONE;
    const bool live = p == MMPC_PHASE_MANIPULATE;
    // ---- 4. x_in; nearest plan row in the joint columns (per-lane first minimum, then the wave arg-min of mmpc_tick_one)
    LANES_BEGIN
    if (live && io.x_in && lane < 9) io.x_in[lane] = lds[MMPC_TICK_XI + lane];
    if (live) {
        double bd = INFINITY, bj = MMPC_TICK_NOROW;
        for (int j = lane; j < nplan; j += MMPC_WAVE) {
            double r6, r7, r8;
            if (fresh) {
                r6 = mmpc_manip_row(j, 6, T, xs, lds + MMPC_TICK_XC);
                r7 = mmpc_manip_row(j, 7, T, xs, lds + MMPC_TICK_XC);
                r8 = mmpc_manip_row(j, 8, T, xs, lds + MMPC_TICK_XC);
            } else {
                const double *row = mio.plan + (size_t)j * 9;
                r6 = row[6]; r7 = row[7]; r8 = row[8];
            }
            const double dj = mmpc_manip_dist3(xs[6], xs[7], xs[8], r6, r7, r8);
            if (dj < bd) { bd = dj; bj = (double)j; }
        }
        lds[MMPC_TICK_RD + lane] = bd;
        lds[MMPC_TICK_RJ + lane] = bj;
    }
    LANES_END
    int start = 0;
    if (live) {
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
        start = jw < (double)nplan ? (int)jw : 0;
    }
    // ---- 5. reference: traj_ref[k] = plan[min(start + k, nplan - 1)]; 6. obstacle table
    const long long tick = io.tick ? io.tick[0] + (adv ? 1 : 0) : 0;
    LANES_BEGIN
    if (live) {
        if (io.start && lane == 0) io.start[0] = start;
        if (io.traj_ref)
            for (int i = lane; i < 9 * (N + 1); i += MMPC_WAVE) {
                const int k = i / 9, c = i - 9 * k;
                const int r = start + k < T ? start + k : T;
                io.traj_ref[i] = fresh ? mmpc_manip_row(r, c, T, xs, lds + MMPC_TICK_XC) : mio.plan[(size_t)r * 9 + c];
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
    // ---- the state, the tick counter and the phase in memory; the robot's entry in the list
    LANES_BEGIN
    if (adv) {
        if (lane < 9) io.x[lane] = lds[MMPC_TICK_XS + lane];
        if (lane == 0) io.tick[0] = tick;
    }
    if (lane == 0) {
        mio.phase[0] = p;
        if (live) {
            const int at = mmpc_manip_take(mio.counts);
            if (at < mio.B) mio.list[at] = mio.b;
        } else mmpc_manip_take(mio.counts + 1);
    }
    LANES_END
}

// robot b of the batch arrays of mmpc_manipulate_prepare_device (include/mmpc.h); a null array stays null
MMPC_DEV void mmpc_manipulate_robot(const MmpcParams &P, int b, int B, double *x, long long *tick, int *phase, const double *U_prev,
                                    const double *pose, int nplan, double *plan, double *qgoal, int *ik_status, const double *obs0,
                                    const double *vel, double *x_in, double *traj_ref, int *start, double *obs, int *list, int *counts,
                                    double *lds MMPC_EMU_ARG) {
    const size_t N = (size_t)P.N, M = (size_t)P.M, r = (size_t)b;
    MmpcManipIO mio;
    MmpcTickIO &io = mio.t;
    io.x = x + r * 9;
    io.tick = tick ? tick + r : nullptr;
    io.U_prev = U_prev ? U_prev + r * N * 5 : nullptr;
    io.glob = nullptr;
    io.nglob = 0;
    io.obs0 = obs0 ? obs0 + r * M * 3 : nullptr;
    io.vel = vel ? vel + r * M * 2 : nullptr;
    io.x_in = x_in ? x_in + r * 9 : nullptr;
    io.traj_ref = traj_ref ? traj_ref + r * (N + 1) * 9 : nullptr;
    io.start = start ? start + r : nullptr;
    io.obs = (obs && M > 0) ? obs + r * (N + 1) * M * 3 : nullptr;
    io.u_guess = nullptr;
    io.x_guess = nullptr;
    mio.phase = phase + r;
    mio.pose = pose + r * 4;
    mio.plan = plan + r * (size_t)nplan * 9;
    mio.nplan = nplan;
    mio.qgoal = qgoal ? qgoal + r * 3 : nullptr;
    mio.ik_status = ik_status ? ik_status + r : nullptr;
    mio.list = list;
    mio.counts = counts;
    mio.b = b;
    mio.B = B;
#ifdef MMPC_EMU
    mmpc_manipulate_one(P, mio, lds, emu);
#else
    mmpc_manipulate_one(P, mio, lds);
#endif
}
