// The fleet mission kernel alone, as mmpc_hip.hip wraps it (TEST ONLY): compiled for gfx950 by tests/test_fleet_mission_cpu.py to
// read the compiler's resource usage of it without building the whole library.
#include <hip/hip_runtime.h>
#include "../../mobile-manipulator-mpc_amd/csrc/mmpc_mission.h"

extern "C" __global__ __launch_bounds__(MMPC_WAVE) void mmpc_mission_probe_kernel(
    const MmpcParams *__restrict__ Pp, int B, double *__restrict__ x, long long *__restrict__ tick, int *__restrict__ phase,
    const double *__restrict__ U_prev, const double *__restrict__ glob, int nglob, const double *__restrict__ obs0,
    const double *__restrict__ vel, double *__restrict__ x_in, double *__restrict__ traj_ref, int *__restrict__ start,
    double *__restrict__ obs, int *__restrict__ lists, int *__restrict__ counts) {
    __shared__ double lds[MMPC_TICK_LDS];
    const int b = (int)blockIdx.x;
    if (b >= B) return;
    mmpc_mission_robot(*Pp, b, B, x, tick, phase, U_prev, glob, nglob, obs0, vel, x_in, traj_ref, start, obs, lists, counts, lds);
}
