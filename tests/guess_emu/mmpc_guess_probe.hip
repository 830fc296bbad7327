// The mission's warm-start kernel alone, as mmpc_hip.hip wraps it (TEST ONLY): compiled for gfx950 by tests/test_fleet_guess_cpu.py
// to read the compiler's resource usage of it without building the whole library.
#include <hip/hip_runtime.h>
#include "../../mobile-manipulator-mpc_amd/csrc/mmpc_guess.h"

extern "C" __global__ __launch_bounds__(MMPC_WAVE) void mmpc_guess_probe_kernel(
    const MmpcParams *__restrict__ Pp, int B, const int *__restrict__ phase, const double *__restrict__ U_prev,
    const double *__restrict__ x_in, double *__restrict__ u_guess, double *__restrict__ x_guess) {
    const int b = (int)blockIdx.x;
    if (b >= B) return;
    mmpc_guess_robot(*Pp, b, phase, U_prev, x_in, u_guess, x_guess);
}
