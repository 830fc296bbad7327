// Host build of the bookkeeping of re-suspendable continuations (TEST ONLY - never part of the product): the per-entry logic of the
// handle's list of suspended instances (mobile-manipulator-mpc_amd/csrc/mmpc_suspend.h) and the rejoin of a mission round
// (mmpc_rejoin_robot, csrc/mmpc_round.h), compiled with -DMMPC_EMU -ffp-contract=off.  Every kernel is a loop over its entries;
// `reverse` runs the entries (and, in the rejoin, the lanes) in the opposite order.  The counts are zeroed here, as the library does
// with a hipMemsetAsync before the kernel.
#define MMPC_EMU 1
#include "../emu_common/mmpc_emu_poison.h"
#include "../../mobile-manipulator-mpc_amd/csrc/mmpc_round.h"
#include "../../mobile-manipulator-mpc_amd/csrc/mmpc_suspend.h"

extern "C" int mmpc_suspend_emu_collect(int B, const int *status, int *list, int *count, int reverse) {
    *count = 0;
    for (int i = 0; i < B; i++) mmpc_suspend_collect(reverse ? B - 1 - i : i, status, list, count);
    return 0;
}

extern "C" int mmpc_suspend_emu_collect_listed(int B, const int *in_list, int n, const int *status, int *list, int *count, int reverse) {
    *count = 0;
    for (int i = 0; i < n; i++) mmpc_suspend_collect_listed(reverse ? n - 1 - i : i, B, in_list, status, list, count);
    return 0;
}

// the compaction after a continuation (stamp null), or the first half of a merge
extern "C" int mmpc_suspend_emu_compact(int B, const int *in_list, int n, const int *status, int *list, int *count, int *stamp, int gen,
                                        int reverse) {
    *count = 0;
    for (int i = 0; i < n; i++) mmpc_suspend_compact(reverse ? n - 1 - i : i, B, in_list, status, list, count, stamp, gen);
    return 0;
}

// the second half of a merge: *count goes on from where the compaction left it
extern "C" int mmpc_suspend_emu_append(int B, const int *in_list, int n, const int *status, int *list, int *count, int *stamp, int gen,
                                       int reverse) {
    for (int i = 0; i < n; i++) mmpc_suspend_append(reverse ? n - 1 - i : i, B, in_list, status, list, count, stamp, gen);
    return 0;
}

extern "C" int mmpc_suspend_emu_rejoin(int N, int B, int *hold, int *solve_phase, int set, const double *U, const int *status,
                                       const int *iters, const long long *tick, const int *phase, double *U_last, double *u0,
                                       int *iters_hist, int *status_hist, int *phase_hist, int T, int *counters, int reverse) {
    for (int i = 0; i < 4; i++) counters[i] = 0;
    for (int i = 0; i < B; i++) {
        const int b = reverse ? B - 1 - i : i;
        MmpcEmu emu = reverse ? MmpcEmu{63, -1, -1} : MmpcEmu{0, 64, 1};
        mmpc_rejoin_robot(N, b, hold, solve_phase, set, U, status, iters, tick, phase, U_last, u0, iters_hist, status_hist, phase_hist, T,
                          counters, emu);
    }
    return 0;
}
