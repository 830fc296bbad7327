// mmpc_suspend.h - who is suspended: the per-entry logic of the kernels that keep a handle's list of suspended instances
// (mmpc_hip.hip: mmpc_collect_suspended, mmpc_collect_suspended_list, mmpc_compact_suspended, mmpc_append_suspended).
//
// A budgeted launch leaves the instances that used up their iterations with status MMPC_STATUS_SUSPENDED; the handle keeps them
// in a compacted list (any order) for mmpc_resume_batch_device.  Without a resume budget (mmpc_set_resume_budget, the default) the
// list is collected once per budgeted launch and forgotten after the first continuation.  With one a continuation may park its
// instances again, and a budgeted list launch carries the instances that are still suspended: the list is then
//   - compacted after every continuation to the entries whose status is still 3 (mmpc_suspend_compact), and
//   - merged in a budgeted list launch: the carried entries compacted, then the listed rows that were suspended appended, each
//     row once (mmpc_suspend_append).  The duplicate guard is a stamp per row: the entry that finds another value than this
//     merge's number there (and leaves the number) is the one that appends.  The compaction stamps what it keeps, so a carried row
//     that the list names again is in the result once - or not at all when its new solve has ended.
// An index outside [0, B) is skipped everywhere (a caller's list is unchecked device memory).
//
// Same shared-source style as mmpc_round.h (hipcc for gfx950, g++ -DMMPC_EMU for the host: tests/suspend_emu).  No arithmetic.
#pragma once
#include "mmpc_core.h"
#include "../../include/mmpc.h"

#ifdef MMPC_EMU
inline int mmpc_suspend_take(int *c) { return (*c)++; }
inline int mmpc_suspend_swap(int *p, int v) { const int o = *p; *p = v; return o; }
#else
__device__ __forceinline__ int mmpc_suspend_take(int *c) { return atomicAdd(c, 1); }
__device__ __forceinline__ int mmpc_suspend_swap(int *p, int v) { return atomicExch(p, v); }
#endif

// instance b of a whole-batch launch: into the list when it was suspended
MMPC_DEV void mmpc_suspend_collect(int b, const int *status, int *list, int *count) {
    if (status[b] == MMPC_STATUS_SUSPENDED) list[mmpc_suspend_take(count)] = b;
}

// entry w of a caller's list (list launches): only the listed instances can have been suspended by the launch before
MMPC_DEV void mmpc_suspend_collect_listed(int w, int B, const int *in_list, const int *status, int *list, int *count) {
    const int b = in_list[w];
    if ((unsigned)b < (unsigned)B && status[b] == MMPC_STATUS_SUSPENDED) list[mmpc_suspend_take(count)] = b;
}

// entry w of the handle's list: kept when its instance is still suspended.  stamp != null (a merge): the kept row gets the
// merge's number, so that mmpc_suspend_append does not enter it again.  The entries of a handle's list are distinct.
MMPC_DEV void mmpc_suspend_compact(int w, int B, const int *in_list, const int *status, int *list, int *count, int *stamp, int gen) {
    const int b = in_list[w];
    if ((unsigned)b >= (unsigned)B || status[b] != MMPC_STATUS_SUSPENDED) return;
    if (stamp) stamp[b] = gen;
    list[mmpc_suspend_take(count)] = b;
}

// entry w of a caller's list: appended when its instance was suspended and no entry of this merge (number gen) has taken the row
MMPC_DEV void mmpc_suspend_append(int w, int B, const int *in_list, const int *status, int *list, int *count, int *stamp, int gen) {
    const int b = in_list[w];
    if ((unsigned)b >= (unsigned)B || status[b] != MMPC_STATUS_SUSPENDED) return;
    if (mmpc_suspend_swap(stamp + b, gen) != gen) list[mmpc_suspend_take(count)] = b;
}
