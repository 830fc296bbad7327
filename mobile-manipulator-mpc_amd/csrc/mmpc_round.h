// mmpc_round.h - the glue of a fleet mission under iteration budgets, one 64-lane workgroup per robot: the mission and manipulate
// kernels per robot instead of per batch, and the commit of a round's solves.
//
// Under a budget a robot whose solve was suspended is continued on a side stream while the others go on (fleet.py:
// DeviceFleet.run_mission(budget=...)), so the robots of a fleet are at different ticks and only some of them take part in a round.
// A hold word per robot (MMPC_HOLD_*, include/mmpc.h) says which: the round kernels here run mmpc_mission_one / mmpc_manipulate_one
// - unchanged - with a per-robot MmpcMissionIO / MmpcManipIO for the robots that are NEW (no advance) or READY (advance with
// U_last[b][0]) and skip every other one; the commit kernel takes a round's solves into U_last and the per-tick histories, or
// marks a robot whose solve used up its budget as suspended on the round's handle set.  A READY robot that has taken tick_limit - 1
// ticks retires: it gets the lock step's output-less call after the last tick (plant step, state machine) and is never touched
// again.  A retiring call must enter no list and no count: it gets the workgroup's spare counters (zeroed here) and a list
// capacity of 0, which mmpc_mission_one / mmpc_manipulate_one compare their list position with.
// Under a resume budget (mmpc_set_resume_budget) a continuation may come back still suspended: the rejoin (mmpc_rejoin_robot) is the
// rejoining commit except that such a robot stays suspended on its set and nothing of it is written.
//
// Same shared-source style as mmpc_mission.h (hipcc for gfx950, g++ -DMMPC_EMU -ffp-contract=off for the host: tests/round_emu).
// No arithmetic of its own: every number is mmpc_mission_one's or mmpc_manipulate_one's, or a copy.
#pragma once
#include "mmpc_mission.h"
#include "mmpc_manipulate.h"

#define MMPC_ROUND_SPARE 4   // ints of per-workgroup spare counters (the counts of a retiring call)

MMPC_DEV bool mmpc_round_solved_phase(int p) {
    return p == MMPC_PHASE_MOVE || p == MMPC_PHASE_APPROACH || p == MMPC_PHASE_ROTATE || p == MMPC_PHASE_MANIPULATE;
}

// robot b of the batch arrays of mmpc_mission_round_device (include/mmpc.h); a null output array stays null
MMPC_DEV void mmpc_mission_round_robot(const MmpcParams &P, int b, int B, double *x, long long *tick, int *phase, const double *U_last,
                                       const double *glob, int nglob, const double *obs0, const double *vel, double *x_in,
                                       double *traj_ref, int *start, double *obs, int *lists, int *counts, int *hold, int *solve_phase,
                                       long long tick_limit, double *lds, int *spare MMPC_EMU_ARG) {
    const size_t N = (size_t)P.N, M = (size_t)P.M, r = (size_t)b;
    const int h = hold[b];
    if (h != MMPC_HOLD_NEW && h != MMPC_HOLD_READY) return;
    const bool ready = h == MMPC_HOLD_READY;
    // a frozen robot (mmpc_mission_one: a code outside 0..2) is counted and nothing else, whatever its tick
    const bool frozen = (unsigned)phase[b] >= (unsigned)MMPC_PHASE_DONE;
    const bool retire = ready && !frozen && tick[b] + 1 >= tick_limit;
    if (retire) {
        LANES_BEGIN
        if (lane < MMPC_ROUND_SPARE) spare[lane] = 0;
        LANES_END
    }
    MmpcMissionIO mio;
    MmpcTickIO &io = mio.t;
    io.x = x + r * 9;
    io.tick = tick + r;
    io.U_prev = ready ? U_last + r * N * 5 : nullptr;
    io.glob = glob + r * (size_t)nglob * 9;
    io.nglob = nglob;
    io.obs0 = obs0 ? obs0 + r * M * 3 : nullptr;
    io.vel = vel ? vel + r * M * 2 : nullptr;
    io.x_in = (x_in && !retire) ? x_in + r * 9 : nullptr;
    io.traj_ref = (traj_ref && !retire) ? traj_ref + r * (N + 1) * 9 : nullptr;
    io.start = (start && !retire) ? start + r : nullptr;
    io.obs = (obs && M > 0 && !retire) ? obs + r * (N + 1) * M * 3 : nullptr;
    io.u_guess = nullptr;
    io.x_guess = nullptr;
    mio.phase = phase + r;
    mio.lists = lists;
    mio.counts = retire ? spare : counts;
    mio.b = b;
    mio.B = retire ? 0 : B;
#ifdef MMPC_EMU
    mmpc_mission_one(P, mio, lds, emu);
#else
    mmpc_mission_one(P, mio, lds);
#endif
    if (frozen) return;
    LANES_BEGIN
    if (lane == 0) {
        const int p = phase[b];
        if (retire) {
            // at 'move finish' the lock step's output-less manipulate call would still make the transition: the manipulate round does
            hold[b] = p == MMPC_PHASE_DONE ? MMPC_HOLD_RETIRED_AT_DONE : MMPC_HOLD_RETIRED;
        } else if ((unsigned)p < (unsigned)MMPC_PHASE_DONE) {
            hold[b] = MMPC_HOLD_LISTED;
            solve_phase[b] = p;
        }
    }
    LANES_END
}

// robot b of the batch arrays of mmpc_manipulate_round_device (include/mmpc.h); a null output array stays null
MMPC_DEV void mmpc_manipulate_round_robot(const MmpcParams &P, int b, int B, double *x, long long *tick, int *phase, const double *U_last,
                                          const double *pose, int nplan, double *plan, double *qgoal, int *ik_status, const double *obs0,
                                          const double *vel, double *x_in, double *traj_ref, int *start, double *obs, int *list,
                                          int *counts, int *hold, int *solve_phase, long long tick_limit, double *lds,
                                          int *spare MMPC_EMU_ARG) {
    const size_t N = (size_t)P.N, M = (size_t)P.M, r = (size_t)b;
    const int h = hold[b];
    // the mission round retired this robot at 'move finish': the output-less transition of the lock step's last call, then RETIRED
    const bool at_done = h == MMPC_HOLD_RETIRED_AT_DONE;
    if (h != MMPC_HOLD_NEW && h != MMPC_HOLD_READY && !at_done) return;
    const bool ready = h == MMPC_HOLD_READY;
    const int p0 = phase[b];
    // (a READY robot at 'move finish' was advanced by the mission round in this round; only one in 'manipulate' advances here)
    const bool mine = p0 == MMPC_PHASE_DONE || p0 == MMPC_PHASE_MANIPULATE;
    const bool retire = at_done || (ready && p0 == MMPC_PHASE_MANIPULATE && tick[b] + 1 >= tick_limit);
    if (retire) {
        LANES_BEGIN
        if (lane < MMPC_ROUND_SPARE) spare[lane] = 0;
        LANES_END
    }
    MmpcManipIO mio;
    MmpcTickIO &io = mio.t;
    io.x = x + r * 9;
    io.tick = tick + r;
    io.U_prev = ready ? U_last + r * N * 5 : nullptr;
    io.glob = nullptr;
    io.nglob = 0;
    io.obs0 = obs0 ? obs0 + r * M * 3 : nullptr;
    io.vel = vel ? vel + r * M * 2 : nullptr;
    io.x_in = (x_in && !retire) ? x_in + r * 9 : nullptr;
    io.traj_ref = (traj_ref && !retire) ? traj_ref + r * (N + 1) * 9 : nullptr;
    io.start = (start && !retire) ? start + r : nullptr;
    io.obs = (obs && M > 0 && !retire) ? obs + r * (N + 1) * M * 3 : nullptr;
    io.u_guess = nullptr;
    io.x_guess = nullptr;
    mio.phase = phase + r;
    mio.pose = pose + r * 4;
    mio.plan = plan + r * (size_t)nplan * 9;
    mio.nplan = nplan;
    mio.qgoal = qgoal ? qgoal + r * 3 : nullptr;
    mio.ik_status = ik_status ? ik_status + r : nullptr;
    mio.list = list;
    mio.counts = retire ? spare : counts;
    mio.b = b;
    mio.B = retire ? 0 : B;
#ifdef MMPC_EMU
    mmpc_manipulate_one(P, mio, lds, emu);
#else
    mmpc_manipulate_one(P, mio, lds);
#endif
    if (!mine && !at_done) return;
    LANES_BEGIN
    if (lane == 0) {
        if (retire) hold[b] = MMPC_HOLD_RETIRED;
        else if (phase[b] == MMPC_PHASE_MANIPULATE) {
            hold[b] = MMPC_HOLD_LISTED;
            solve_phase[b] = MMPC_PHASE_MANIPULATE;
        }
    }
    LANES_END
}

// the body of the commit and of the rejoin of robot b.  `again` (a constant of the caller): a robot whose continuation was suspended
// again (status 3 under rejoin: mmpc_set_resume_budget) stays SUSPENDED + set and nothing of it is written - its hold word and its
// solve phase included - but counters[1]; without it a status 3 under rejoin is committed
MMPC_DEV void mmpc_commit_robot_body(int N, int b, int *hold, int *solve_phase, int set, int rejoin, bool again, const double *U,
                                     const int *status, const int *iters, const long long *tick, const int *phase, double *U_last, double *u0,
                                     int *iters_hist, int *status_hist, int *phase_hist, int T, int *counters MMPC_EMU_ARG) {
    const size_t r = (size_t)b, nu = (size_t)N * 5;
    const int h = hold[b];
    const bool mine = rejoin ? h == MMPC_HOLD_SUSPENDED + set : h == MMPC_HOLD_LISTED;
    const int st = mine ? status[b] : 0;
    if (again && mine && st == 3) {
        LANES_BEGIN
        if (lane == 0) { mmpc_mission_take(counters + 1); mmpc_mission_take(counters + 3); }
        LANES_END
        return;
    }
    const bool suspend = mine && st == 3 && !rejoin, commit = mine && !suspend;
    const int hn = suspend ? MMPC_HOLD_SUSPENDED + set : (commit ? MMPC_HOLD_READY : h);
    const long long t = tick[b];
    LANES_BEGIN
    if (commit) {
        for (size_t i = (size_t)lane; i < nu; i += MMPC_WAVE) U_last[r * nu + i] = U[r * nu + i];
        if (t >= 0 && t < (long long)T) {
            const size_t at = r * (size_t)T + (size_t)t;
            if (lane < 5) u0[at * 5 + lane] = U[r * nu + lane];
            if (lane == 0) {
                iters_hist[at] = iters[b];
                status_hist[at] = st;
                phase_hist[at] = phase[b];
            }
        }
    }
    if (lane == 0) {
        if (mine) {
            hold[b] = hn;
            solve_phase[b] = -1;
            if (suspend) mmpc_mission_take(counters + 1);
            else {
                mmpc_mission_take(counters);
                if (st != 0) mmpc_mission_take(counters + 2);
            }
        }
        // live: the run still has work for this robot
        if (hn == MMPC_HOLD_NEW || hn == MMPC_HOLD_LISTED || hn >= MMPC_HOLD_SUSPENDED ||
            (hn == MMPC_HOLD_READY && mmpc_round_solved_phase(phase[b])))
            mmpc_mission_take(counters + 3);
    }
    LANES_END
}

// robot b of the arrays of mmpc_mission_commit_device (include/mmpc.h)
MMPC_DEV void mmpc_commit_robot(int N, int b, int *hold, int *solve_phase, int set, int rejoin, const double *U, const int *status,
                                const int *iters, const long long *tick, const int *phase, double *U_last, double *u0, int *iters_hist,
                                int *status_hist, int *phase_hist, int T, int *counters MMPC_EMU_ARG) {
#ifdef MMPC_EMU
    mmpc_commit_robot_body(N, b, hold, solve_phase, set, rejoin, false, U, status, iters, tick, phase, U_last, u0, iters_hist, status_hist,
                           phase_hist, T, counters, emu);
#else
    mmpc_commit_robot_body(N, b, hold, solve_phase, set, rejoin, false, U, status, iters, tick, phase, U_last, u0, iters_hist, status_hist,
                           phase_hist, T, counters);
#endif
}

// robot b of the arrays of mmpc_mission_rejoin_device (include/mmpc.h): the rejoin of the commit, except that a robot whose
// continuation was suspended again stays suspended
MMPC_DEV void mmpc_rejoin_robot(int N, int b, int *hold, int *solve_phase, int set, const double *U, const int *status, const int *iters,
                                const long long *tick, const int *phase, double *U_last, double *u0, int *iters_hist, int *status_hist,
                                int *phase_hist, int T, int *counters MMPC_EMU_ARG) {
#ifdef MMPC_EMU
    mmpc_commit_robot_body(N, b, hold, solve_phase, set, 1, true, U, status, iters, tick, phase, U_last, u0, iters_hist, status_hist,
                           phase_hist, T, counters, emu);
#else
    mmpc_commit_robot_body(N, b, hold, solve_phase, set, 1, true, U, status, iters, tick, phase, U_last, u0, iters_hist, status_hist,
                           phase_hist, T, counters);
#endif
}
