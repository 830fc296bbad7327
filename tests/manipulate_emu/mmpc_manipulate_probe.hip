// The fleet manipulate kernel alone, as mmpc_hip.hip wraps it (TEST ONLY): compiled for gfx950 by tests/test_fleet_manipulate_cpu.py
// to read the compiler's resource usage of it without building the whole library.
#include <hip/hip_runtime.h>
#include "../../mobile-manipulator-mpc_amd/csrc/mmpc_manipulate.h"

extern "C" __global__ __launch_bounds__(MMPC_WAVE) void mmpc_manipulate_probe_kernel(
    const MmpcParams *__restrict__ Pp, int B, double *__restrict__ x, long long *__restrict__ tick, int *__restrict__ phase,
    const double *__restrict__ U_prev, const double *__restrict__ pose, int nplan, double *plan, double *__restrict__ qgoal,
    int *__restrict__ ik_status, const double *__restrict__ obs0, const double *__restrict__ vel, double *__restrict__ x_in,
    double *__restrict__ traj_ref, int *__restrict__ start, double *__restrict__ obs, int *__restrict__ list, int *__restrict__ counts) {
    __shared__ double lds[MMPC_TICK_LDS];
    const int b = (int)blockIdx.x;
    if (b >= B) return;
    mmpc_manipulate_robot(*Pp, b, B, x, tick, phase, U_prev, pose, nplan, plan, qgoal, ik_status, obs0, vel, x_in, traj_ref, start, obs, list,
                          counts, lds);
}
