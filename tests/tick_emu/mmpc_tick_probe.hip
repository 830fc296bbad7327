// The fleet tick kernel alone, as mmpc_hip.hip wraps it (TEST ONLY): compiled for gfx950 by tests/test_fleet_tick_cpu.py to read
// the compiler's resource usage of it without building the whole library.
#include <hip/hip_runtime.h>
#include "../../mobile-manipulator-mpc_amd/csrc/mmpc_tick.h"

extern "C" __global__ __launch_bounds__(MMPC_WAVE) void mmpc_tick_probe_kernel(
    const MmpcParams *__restrict__ Pp, int B, double *__restrict__ x, long long *__restrict__ tick, const double *__restrict__ U_prev,
    const double *__restrict__ glob, int nglob, const double *__restrict__ obs0, const double *__restrict__ vel,
    double *__restrict__ x_in, double *__restrict__ traj_ref, int *__restrict__ start, double *__restrict__ obs,
    double *__restrict__ u_guess, double *__restrict__ x_guess) {
    __shared__ double lds[MMPC_TICK_LDS];
    const int b = (int)blockIdx.x;
    if (b >= B) return;
    mmpc_tick_robot(*Pp, b, x, tick, U_prev, glob, nglob, obs0, vel, x_in, traj_ref, start, obs, u_guess, x_guess, lds);
}
