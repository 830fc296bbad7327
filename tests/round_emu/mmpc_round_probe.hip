// The three kernels of a mission round alone, as mmpc_hip.hip wraps them (TEST ONLY): compiled for gfx950 by
// tests/test_fleet_round_cpu.py to read the compiler's resource usage of them without building the whole library.
#include <hip/hip_runtime.h>
#include "../../mobile-manipulator-mpc_amd/csrc/mmpc_round.h"

extern "C" __global__ __launch_bounds__(MMPC_WAVE) void mmpc_mission_round_probe_kernel(
    const MmpcParams *__restrict__ Pp, int B, double *__restrict__ x, long long *__restrict__ tick, int *__restrict__ phase,
    const double *__restrict__ U_last, const double *__restrict__ glob, int nglob, const double *__restrict__ obs0,
    const double *__restrict__ vel, double *__restrict__ x_in, double *__restrict__ traj_ref, int *__restrict__ start,
    double *__restrict__ obs, int *__restrict__ lists, int *__restrict__ counts, int *__restrict__ hold, int *__restrict__ solve_phase,
    long long tick_limit) {
    __shared__ double lds[MMPC_TICK_LDS];
    __shared__ int spare[MMPC_ROUND_SPARE];
    const int b = (int)blockIdx.x;
    if (b >= B) return;
    mmpc_mission_round_robot(*Pp, b, B, x, tick, phase, U_last, glob, nglob, obs0, vel, x_in, traj_ref, start, obs, lists, counts, hold,
                             solve_phase, tick_limit, lds, spare);
}

extern "C" __global__ __launch_bounds__(MMPC_WAVE) void mmpc_manipulate_round_probe_kernel(
    const MmpcParams *__restrict__ Pp, int B, double *__restrict__ x, long long *__restrict__ tick, int *__restrict__ phase,
    const double *__restrict__ U_last, const double *__restrict__ pose, int nplan, double *plan, double *__restrict__ qgoal,
    int *__restrict__ ik_status, const double *__restrict__ obs0, const double *__restrict__ vel, double *__restrict__ x_in,
    double *__restrict__ traj_ref, int *__restrict__ start, double *__restrict__ obs, int *__restrict__ list, int *__restrict__ counts,
    int *__restrict__ hold, int *__restrict__ solve_phase, long long tick_limit) {
    __shared__ double lds[MMPC_TICK_LDS];
    __shared__ int spare[MMPC_ROUND_SPARE];
    const int b = (int)blockIdx.x;
    if (b >= B) return;
    mmpc_manipulate_round_robot(*Pp, b, B, x, tick, phase, U_last, pose, nplan, plan, qgoal, ik_status, obs0, vel, x_in, traj_ref, start, obs,
                                list, counts, hold, solve_phase, tick_limit, lds, spare);
}

extern "C" __global__ __launch_bounds__(MMPC_WAVE) void mmpc_commit_probe_kernel(
    int N, int B, int *__restrict__ hold, int *__restrict__ solve_phase, int set, int rejoin, const double *__restrict__ U,
    const int *__restrict__ status, const int *__restrict__ iters, const long long *__restrict__ tick, const int *__restrict__ phase,
    double *__restrict__ U_last, double *__restrict__ u0, int *__restrict__ iters_hist, int *__restrict__ status_hist,
    int *__restrict__ phase_hist, int T, int *__restrict__ counters) {
    const int b = (int)blockIdx.x;
    if (b >= B) return;
    mmpc_commit_robot(N, b, hold, solve_phase, set, rejoin, U, status, iters, tick, phase, U_last, u0, iters_hist, status_hist, phase_hist,
                      T, counters);
}
