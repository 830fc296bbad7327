// mmpc_hip.hip - gfx950 kernels + the C ABI of include/mmpc.h (libmmpc.so).
// One 64-lane workgroup (= one wavefront) per problem instance; the solver core is
// mmpc_core.h.  No CPU fallback: every entry point needs a HIP device.
// From a config to a kernel: mmpc_create resolves the handle's kernels once (resolve_kernels: the generic one, and the specialised
// pair when MMPC_FAST_LIST has the shape, or - for a handle created with cfg.specialise - when a shape library with it has been
// loaded, mmpc_load_shape_library) and keeps them as typed pointers; launch() picks by runs_fast() and launches through them.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <dlfcn.h>
#include <mutex>
#include <new>
#include <utility>
#include <vector>

#include "../../include/mmpc.h"
#include "mmpc_core.h"
#include "mmpc_fast.h"
#include "mmpc_fast_kernel.h"
#include "mmpc_ik.h"
#include "mmpc_tick.h"
#include "mmpc_mission.h"
#include "mmpc_manipulate.h"
#include "mmpc_round.h"
#include "mmpc_suspend.h"
#include "mmpc_guess.h"

template <int KIND, int NC = 0, int MC = -1, int OPSC = -1, int LC = -1>
__global__ __launch_bounds__(MMPC_WAVE) void mmpc_solve_kernel(
    const MmpcParams *__restrict__ Pp, int B, const double *__restrict__ x_init, const double *__restrict__ traj_ref,
    const double *__restrict__ u_ref, const double *__restrict__ u_last, const double *__restrict__ x_guess,
    const double *__restrict__ obs, double *__restrict__ X, double *__restrict__ U, double *__restrict__ s,
    int *__restrict__ status, int *__restrict__ iters, double *__restrict__ cost, double *__restrict__ err,
    const int *__restrict__ order, double *__restrict__ soc, int soc_stride, const long long *__restrict__ tick,
    double scale_max_grad, double *__restrict__ scale_out, const int *__restrict__ list_count) {
    extern __shared__ double lds[];
    // (list launches, mmpc_solve_rows_device: `order` is the caller's list and *list_count its length, both read here)
    if ((int)blockIdx.x >= (list_count ? *list_count : B)) return;
    // longest-first schedule hint: workgroup i solves instance order[i] (a permutation; results do not depend on it)
    const int b = order ? order[blockIdx.x] : (int)blockIdx.x;
    if ((unsigned)b >= (unsigned)B) return;
    const MmpcParams &P = *Pp;
    const int N = NC ? NC : P.N, M = MC >= 0 ? MC : P.M;
    // (doubles of an instance's obstacles: the motion record of OPSC = 2 - a constant of the instantiation, see mmpc_solve_one - or the table)
    const size_t so = OPSC == 2 ? (size_t)M * 5 : (size_t)((OPSC >= 0 ? OPSC : P.obs_per_stage) ? N + 1 : 1) * M * 3;
    MmpcIO io;
    mmpc_instance_io<KIND>(io, P, b, N, so, x_init, traj_ref, u_ref, u_last, x_guess, obs, X, U, s, status, iters, cost, err,
                           soc, soc_stride);
    if (OPSC == 2 && tick) io.tick = tick + b;
    io.scale_max_grad = scale_max_grad; if (scale_out) io.scale_out = scale_out + b;   // (objective scaling, mmpc_set_objective_scaling; 0: off)
    mmpc_solve_one<KIND, NC, MC, OPSC, LC>(P, io, lds);
}

// The run-time-sized generic kernel with the iteration budget / continuation code (mmpc_solve_one<.., CONT = true>): what a handle
// created with cfg.generic_budget launches when a budget is set or suspended instances are continued.  The launch forms are those
// of mmpc_fast_kernel: a whole batch or a caller's list (`order`, *list_count) with one instance per workgroup, or - resume_count
// != null - a continuation, whose small grid strides over the compacted list of the suspended instances.
template <int KIND, int OPSC = -1>
__global__ __launch_bounds__(MMPC_WAVE) void mmpc_solve_kernel_cont(
    const MmpcParams *__restrict__ Pp, int B, const double *__restrict__ x_init, const double *__restrict__ traj_ref,
    const double *__restrict__ u_ref, const double *__restrict__ u_last, const double *__restrict__ x_guess,
    const double *__restrict__ obs, double *__restrict__ X, double *__restrict__ U, double *__restrict__ s,
    int *__restrict__ status, int *__restrict__ iters, double *__restrict__ cost, double *__restrict__ err,
    const int *__restrict__ order, double *__restrict__ soc, int soc_stride, const long long *__restrict__ tick,
    double scale_max_grad, double *__restrict__ scale_out, const int *__restrict__ list_count, int budget,
    double *__restrict__ state, int state_stride, const int *__restrict__ resume_count) {
    extern __shared__ double lds[];
    const int limit = resume_count ? *resume_count : (list_count ? *list_count : B);
    for (int w = (int)blockIdx.x; w < limit; w += (int)gridDim.x) {
        const int b = order ? order[w] : w;
        // (an index outside the batch - a caller's list is unchecked device memory - is skipped: it would address the save areas too)
        if ((unsigned)b >= (unsigned)B) { if (!resume_count) break; continue; }
        const MmpcParams &P = *Pp;
        const int N = P.N, M = P.M;
        const size_t so = OPSC == 2 ? (size_t)M * 5 : (size_t)(P.obs_per_stage ? N + 1 : 1) * M * 3;
        MmpcIO io;
        mmpc_instance_io<KIND>(io, P, b, N, so, x_init, traj_ref, u_ref, u_last, x_guess, obs, X, U, s, status, iters, cost, err,
                               soc, soc_stride);
        if (OPSC == 2 && tick) io.tick = tick + b;
        io.scale_max_grad = scale_max_grad; if (scale_out) io.scale_out = scale_out + b;
        io.state = state ? state + (size_t)b * state_stride : nullptr;
        io.budget = budget;
        io.resume = (resume_count && state) ? 1 : 0;
        mmpc_solve_one<KIND, 0, -1, OPSC, -1, -1, true>(P, io, lds);
        if (!resume_count) break;               // (one instance per workgroup except in a continuation launch)
        __builtin_amdgcn_s_barrier();           // the next instance reuses the LDS block
    }
}

// WPE = waves per SIMD the register allocation is sized for (2: <= 256 registers, only pays when LDS allows >4 problems/CU)
// The generic kernel for a shape that is a constant of the instantiation (the demo's shapes, MMPC_STATIC_LIST): static LDS block
// and compile-time layout, as for the specialised kernels below; same code, same results as mmpc_solve_kernel<KIND>.
template <int KIND, int NC, int MC, int OPSC, int LC, int AWC>
__global__ __launch_bounds__(MMPC_WAVE) void mmpc_solve_kernel_static(
    const MmpcParams *__restrict__ Pp, int B, const double *__restrict__ x_init, const double *__restrict__ traj_ref,
    const double *__restrict__ u_ref, const double *__restrict__ u_last, const double *__restrict__ x_guess,
    const double *__restrict__ obs, double *__restrict__ X, double *__restrict__ U, double *__restrict__ s,
    int *__restrict__ status, int *__restrict__ iters, double *__restrict__ cost, double *__restrict__ err,
    const int *__restrict__ order, double *__restrict__ soc, int soc_stride, const long long *__restrict__ tick,
    double scale_max_grad, double *__restrict__ scale_out, const int *__restrict__ list_count) {
    constexpr int NHS = (KIND == 0 && LC > 0) ? 6 : 0, NQ = (KIND == 0 && AWC && LC >= 2) ? 6 * (LC - 1) : 0;
    __shared__ double lds[mmpc_layout<KIND>(NC, MC, OPSC, NHS, NQ).total];
    if ((int)blockIdx.x >= (list_count ? *list_count : B)) return;
    const int b = order ? order[blockIdx.x] : (int)blockIdx.x;
    if ((unsigned)b >= (unsigned)B) return;
    const MmpcParams &P = *Pp;
    constexpr int N = NC, M = MC;
    constexpr size_t so = OPSC == 2 ? (size_t)M * 5 : (size_t)(OPSC ? N + 1 : 1) * M * 3;
    MmpcIO io;
    mmpc_instance_io<KIND>(io, P, b, N, so, x_init, traj_ref, u_ref, u_last, x_guess, obs, X, U, s, status, iters, cost, err,
                           soc, soc_stride);
    if (OPSC == 2 && tick) io.tick = tick + b;
    io.scale_max_grad = scale_max_grad; if (scale_out) io.scale_out = scale_out + b;   // (objective scaling, mmpc_set_objective_scaling; 0: off)
    mmpc_solve_one<KIND, NC, MC, OPSC, LC, AWC>(P, io, lds);
}
// (kind, N, M, obs_per_stage, L, as_written): demo_wholebody_qref.py scenario 2 (two planes) as written and with the intended
// rows, scenario 1 (three planes) as written, the plane-free shape (the terminal-xy 'approach' phase of scenario 0), and the
// shape of BASELINE configs C3 / C4 for the cases the specialised kernel refuses (dense weights, terminal equality): 38 -> 32 ms
// per 8192 against the run-time-sized kernel (no scalar spills: every LDS offset an immediate)
#ifndef MMPC_STATIC_LIST   // (experiments build shorter lists: tools/build_variant.sh)
#define MMPC_STATIC_LIST(X) X(0, 20, 3, 0, 2, 1) X(0, 20, 3, 0, 2, 0) X(0, 20, 3, 0, 3, 1) X(0, 20, 3, 0, 0, 0) X(0, 20, 5, 0, 0, 0)
#endif

// (kind, N, M) triples with a specialised kernel; everything else runs the generic kernel.
// BASELINE configs C3/C4 (0,20,5), C5 (0,30,8), C2 (1,15,3); the reference demo (0,20,3).
// The base-only kernel needs 16 KB of LDS per problem (9 problems/CU): it is built for 2 waves/SIMD (+21 % measured).
#define MMPC_RESUME_GRID 256   // workgroups of a continuation launch (they stride over the list of suspended instances)
#ifndef MMPC_FAST_LIST   // (experiments build other lists: -D'MMPC_FAST_LIST(X)=X(0, 10, 5, 2)', tools/occupancy_probe.sh)
#define MMPC_FAST_LIST(X) X(0, 20, 5, 1) X(0, 30, 8, 1) X(0, 20, 3, 1) X(1, 15, 3, 2)
#endif

// Longest-processing-time-first order for the NEXT launch: instances sorted by descending iteration count of
// this one (counting sort, 256 bins, one workgroup).  Kernel time is bounded by the slowest instance; starting
// the slow ones first removes the tail.  In receding-horizon use consecutive ticks have correlated difficulty.
// (One workgroup of MMPC_LPT_THREADS = 256 threads: while another stream's solve launch fills the chip - groups of robots out of
//  phase, fleet.py:run_groups - a workgroup only gets a CU slot where a solver wave has just ended, and four waves fit the one
//  SIMD that frees; the 1024-thread form of round 2 needed two free SIMDs of one CU at once and waited up to 7 ms for them.)
#define MMPC_LPT_THREADS 256
__global__ __launch_bounds__(MMPC_LPT_THREADS) void mmpc_lpt_order(int B, const int *__restrict__ iters, int *__restrict__ order) {
    __shared__ int hist[256], start[256];
    const int t = (int)threadIdx.x;
    for (int v = t; v < 256; v += MMPC_LPT_THREADS) hist[v] = 0;
    __syncthreads();
    for (int i = t; i < B; i += MMPC_LPT_THREADS) { int v = iters[i]; v = v < 0 ? 0 : (v > 255 ? 255 : v); atomicAdd(&hist[v], 1); }
    __syncthreads();
    if (t == 0) { int acc = 0; for (int v = 255; v >= 0; v--) { start[v] = acc; acc += hist[v]; } }
    __syncthreads();
    for (int i = t; i < B; i += MMPC_LPT_THREADS) { int v = iters[i]; v = v < 0 ? 0 : (v > 255 ? 255 : v); order[atomicAdd(&start[v], 1)] = i; }
}

// list of the instances a budgeted launch left suspended (any order), and their number (the per-entry logic: mmpc_suspend.h)
__global__ __launch_bounds__(256) void mmpc_collect_suspended(int B, const int *__restrict__ status, int *__restrict__ list,
                                                             int *__restrict__ count) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < B) mmpc_suspend_collect(b, status, list, count);
}

// the same over a list of instances (list launches): only the listed ones can have been suspended by the launch before
__global__ __launch_bounds__(256) void mmpc_collect_suspended_list(int B, const int *__restrict__ in_list, const int *__restrict__ in_count,
                                                                  const int *__restrict__ status, int *__restrict__ list, int *__restrict__ count) {
    const int w = blockIdx.x * 256 + threadIdx.x;
    if (w < *in_count) mmpc_suspend_collect_listed(w, B, in_list, status, list, count);
}

// resume budget (mmpc_set_resume_budget): the handle's list compacted to the instances that are still suspended, into the handle's
// other list buffer (a grid-stride loop: the length is on the device).  stamp != null: the first half of a merge
__global__ __launch_bounds__(256) void mmpc_compact_suspended(int B, const int *__restrict__ in_list, const int *__restrict__ in_count,
                                                             const int *__restrict__ status, int *__restrict__ list, int *__restrict__ count,
                                                             int *__restrict__ stamp, int gen) {
    const int n = *in_count < B ? *in_count : B;
    for (int w = blockIdx.x * 256 + threadIdx.x; w < n; w += gridDim.x * 256) mmpc_suspend_compact(w, B, in_list, status, list, count, stamp, gen);
}

// ... and the second half: the rows of a list launch that were suspended, each appended once unless the list holds it already
__global__ __launch_bounds__(256) void mmpc_append_suspended(int B, const int *__restrict__ in_list, const int *__restrict__ in_count,
                                                            const int *__restrict__ status, int *__restrict__ list, int *__restrict__ count,
                                                            int *__restrict__ stamp, int gen) {
    const int w = blockIdx.x * 256 + threadIdx.x;
    if (w < *in_count) mmpc_suspend_append(w, B, in_list, status, list, count, stamp, gen);
}

// A-priori difficulty of an instance, from its data alone: how close the reference path comes to (or how deep it cuts
// into) an inflated obstacle disc - key = max over stages and obstacles of (r + base radius) - |ref_k - centre|.  The
// iteration count of the interior-point solve correlates with it (0.26 on the C4 generator; the instances that need 40+
// iterations are almost all among the deep cuts), and starting the workgroups in descending key order recovers about
// three quarters of what the exact longest-first order gains over batch order (list-scheduling the measured counts on
// 1024 slots: 192 iterations of wall time in batch order, 168 by this key, 160 exact).  Written as a pseudo iteration
// count 0..255 so that mmpc_lpt_order sorts it.
// With half-space obstacles (whole-body kind, L > 0) a second term: how far the arm's sample points of the START state reach
// into the planes (the largest half-space row value at x_init; [-0.5 m clear .. 0.4 m inside] -> 0..255), the larger of the two
// is the key.  On the demo's shape (2048 starts around the two planes, list-scheduled on 256 slots: 372 iterations of wall time
// in batch order, 250 exact) it gives 258 for the rows as written and 256 for the intended rows (exact there: 219) - the
// circles of that scenario are far away and their key alone is batch order.
// MOTION: `obs` is the motion record of obs_per_stage = 2 and `tick` its clock (null: 0) - the centres are those of the table twin,
// formed by the same helpers (mmpc_core.h), and so is the key.
template <bool MOTION>
__device__ __forceinline__ void mmpc_difficulty_key_body(int B, int N, int M, int nref, int obs_per_stage,
                                                          const double *__restrict__ traj_ref, const double *__restrict__ obs,
                                                          int *__restrict__ key, const MmpcParams *__restrict__ Pp,
                                                          const double *__restrict__ x_init, int planes, const long long *__restrict__ tick) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    int key_hs = 0;
    if (planes > 0) {
        const MmpcParams &P = *Pp;
        const double *x0 = x_init + (size_t)b * 9;
        double sn, cs, dr[3], dz[3], worst_hs = -1.0e9;
        mmpc_sincos(x0[2], &sn, &cs);
        mmpc_arm_segments(x0[6], x0[7], x0[8], dr, dz);
        for (int i = 0; i < 6; i++) worst_hs = fmax(worst_hs, mmpc_hs_row(P, i, x0[0], x0[1], cs, sn, dr, dz, nullptr));
        const double q2 = (worst_hs + 0.5) * (255.0 / 0.9);
        key_hs = (int)fmin(fmax(q2, 0.0), 255.0);   // (a NaN start: 0 - the solve reports it)
    }
    const double *tr = traj_ref + (size_t)b * (N + 1) * nref;
    double worst = -1.0e9;
    if constexpr (MOTION) {
        const double *rec = obs + (size_t)b * M * 5;
        const double tickd = tick ? (double)tick[b] : 0.0, dt = Pp->dt;
        for (int k = 0; k <= N; k++) {
            const double x = tr[k * nref], y = tr[k * nref + 1], t = mmpc_tick_time_d(tickd, k, dt);
            for (int m = 0; m < M; m++) {
                const double dx = x - mmpc_tick_centre(rec[5 * m], rec[5 * m + 3], t), dy = y - mmpc_tick_centre(rec[5 * m + 1], rec[5 * m + 4], t);
                worst = fmax(worst, (rec[5 * m + 2] + MMPC_BASE_R) - sqrt(dx * dx + dy * dy));
            }
        }
    } else {
    const double *ob = obs + (size_t)b * (obs_per_stage ? N + 1 : 1) * M * 3;
    for (int k = 0; k <= N; k++) {
        const double x = tr[k * nref], y = tr[k * nref + 1];
        const double *o = ob + (obs_per_stage ? (size_t)k * M * 3 : 0);
        for (int m = 0; m < M; m++) {
            const double dx = x - o[3 * m], dy = y - o[3 * m + 1];
            worst = fmax(worst, (o[3 * m + 2] + MMPC_BASE_R) - sqrt(dx * dx + dy * dy));
        }
    }
    }
    // [-1.5 m clearance .. 1.0 m penetration] -> 0..255
    const double q = (worst + 1.5) * (255.0 / 2.5);
    const int key_c = M > 0 ? (int)fmin(fmax(q, 0.0), 255.0) : 0;
    key[b] = key_c > key_hs ? key_c : key_hs;
}
__global__ __launch_bounds__(64) void mmpc_difficulty_key(int B, int N, int M, int nref, int obs_per_stage,
                                                          const double *__restrict__ traj_ref, const double *__restrict__ obs,
                                                          int *__restrict__ key, const MmpcParams *__restrict__ Pp,
                                                          const double *__restrict__ x_init, int planes) {
    mmpc_difficulty_key_body<false>(B, N, M, nref, obs_per_stage, traj_ref, obs, key, Pp, x_init, planes, nullptr);
}
__global__ __launch_bounds__(64) void mmpc_difficulty_key_motion(int B, int N, int M, int nref, const double *__restrict__ traj_ref,
                                                                 const double *__restrict__ rec, int *__restrict__ key,
                                                                 const MmpcParams *__restrict__ Pp, const double *__restrict__ x_init,
                                                                 int planes, const long long *__restrict__ tick) {
    mmpc_difficulty_key_body<true>(B, N, M, nref, 2, traj_ref, rec, key, Pp, x_init, planes, tick);
}

// out_u0[b][a] = U[b][0][a]
__global__ void mmpc_gather_u0(int B, int NU, int stride, const double *__restrict__ U, double *__restrict__ u0) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B * NU) u0[i] = U[(size_t)(i / NU) * stride + (i % NU)];
}

// Warm-start bookkeeping of the host-pointer entry point.  The reference assigns u_latest / x_guess only after a
// successful solve (mpc_wholebody_qref.py:329-330 come after the exception of :315): a failed instance keeps its
// previous warm start.  warm[b] = 1 once instance b has a converged solution in its rows.
__global__ void mmpc_keep_converged(int B, int nU, int nX, const int *__restrict__ status, const double *__restrict__ U,
                                    const double *__restrict__ X, double *__restrict__ u_latest, double *__restrict__ x_guess,
                                    int *__restrict__ warm) {
    const int b = blockIdx.x;
    if (b >= B || status[b] != MMPC_STATUS_CONVERGED) return;
    for (int i = threadIdx.x; i < nU; i += blockDim.x) u_latest[(size_t)b * nU + i] = U[(size_t)b * nU + i];
    for (int i = threadIdx.x; i < nX; i += blockDim.x) x_guess[(size_t)b * nX + i] = X[(size_t)b * nX + i];
    if (threadIdx.x == 0) warm[b] = 1;
}
// X guess of the instances that have no converged solution yet = what a null guess means: tile(x_init), clipped to xlim
// for the whole-body kinds (:290-291,:302; mpc_base.py:191-207 does not clip)
__global__ void mmpc_cold_xguess(int B, int NS, int NX, int clip, const MmpcParams *__restrict__ P, const int *__restrict__ warm,
                                 const double *__restrict__ x_init, double *__restrict__ x_guess) {
    const int b = blockIdx.x;
    if (b >= B || warm[b]) return;
    for (int i = threadIdx.x; i < NS * NX; i += blockDim.x) {
        const int j = i % NX;
        double v = x_init[(size_t)b * NX + j];
        if (clip) v = fmax(fmin(v, P->xlim[1][j]), P->xlim[0][j]);
        x_guess[(size_t)b * NS * NX + i] = v;
    }
}

// the signature of mmpc_solve_kernel<> and mmpc_solve_kernel_static<> (that of mmpc_fast_kernel<>: mmpc_fast_fn, mmpc_fast_kernel.h)
typedef void (*mmpc_gen_fn)(const MmpcParams *, int, const double *, const double *, const double *, const double *, const double *,
                            const double *, double *, double *, double *, int *, int *, double *, double *, const int *, double *, int,
                            const long long *, double, double *, const int *);

// the signature of mmpc_solve_kernel_cont<>
typedef void (*mmpc_gen_cont_fn)(const MmpcParams *, int, const double *, const double *, const double *, const double *, const double *,
                                 const double *, double *, double *, double *, int *, int *, double *, double *, const int *, double *, int,
                                 const long long *, double, double *, const int *, int, double *, int, const int *);

struct mmpc_handle_s {
    mmpc_config cfg;
    MmpcParams hp;          // host copy
    MmpcParams *dp;         // device copy
    int nx, nu, nref, lds_bytes;
    // the handle's kernels, resolved once by mmpc_create (resolve_kernels)
    mmpc_gen_fn gen_fn;     // generic: mmpc_solve_kernel<kind>, or the shape's static-LDS instantiation (MMPC_STATIC_LIST)
    int gen_dyn_lds;        // dynamic LDS of a gen_fn launch: lds_bytes, or 0 for a static-LDS instantiation
    mmpc_gen_cont_fn gen_cont_fn;   // cfg.generic_budget: the CONT twin of the run-time-sized generic kernel (gen_fn is then that kernel); else null
    int gen_state_doubles;  // ... and the save area of an instance it suspends (mmpc_gen_state)
    const long long *d_tick;   // obs_per_stage = 2: the registered clock [max_batch] (mmpc_set_obstacle_clock; null: tick 0)
    double scale_max_grad;     // objective scaling (mmpc_set_objective_scaling): nlp_scaling_max_gradient, 0 = off (the default)
    double *d_scale_out;       // ... and the registered array of the instances' factors [max_batch] (null: not wanted)
    mmpc_fast_fn fast_fn[2];   // specialised [CONT] for the handle's obs_per_stage; null: (kind, N, M) has none (MMPC_FAST_LIST) or L > 0
    int fast_lds_bytes;
    int per_cu, fast_per_cu;   // resident workgroups (= problems) per CU the runtime reports for the two kernels
    int diag;               // weights are diagonal (required by the specialised kernel)
    // one stream at a time: launches of a handle share device state (params, schedule hint, warm start), so work on a
    // new stream is ordered after the handle's previous launch through `ev` (recorded after every launch)
    hipEvent_t ev;
    hipStream_t last_stream;
    int ev_valid;
    int hint_on;            // mmpc_set_schedule_hint: 0 batch order, 1 history when there is one / data-derived otherwise, 2 data-derived
    int *d_key;             // a-priori difficulty keys of the launch being prepared
    // iteration budget / continuation (mmpc_set_iteration_budget, mmpc_resume_batch_device)
    int budget;             // iterations a launch may spend on an instance before it is suspended (0: no budget)
    int state_doubles;      // save area per instance
    double *d_state;        // [max_batch][state_doubles], allocated when a budget is first set
    double *d_gscr;         // [max_batch][gscr_doubles]: gain blocks of the specialised kernels of long horizons (MmpcGainBlock), else null
    int gscr_doubles;
    double *d_soc;          // [max_batch][soc_doubles]: scratch of the second-order correction (mmpc_soc_doubles), every kernel
    int soc_doubles;
    int *d_list, *d_count;  // compacted list of the suspended instances of the last launch
    int resume_B;           // batch size of the budgeted launch whose suspended instances can still be continued (0: nothing to resume)
    int resume_fast;        // ... and the family that launch ran (1 specialised, 0 generic): its continuation runs the same one
    // resume budget (mmpc_set_resume_budget): a continuation may suspend again, a budgeted list launch carries the suspended
    int resume_budget;      // iterations a continuation may spend on an instance (0, the default: to the end)
    int *d_list2, *d_count2;   // the other list buffer: a compaction or a merge writes it, then the two pairs change places
    int *d_stamp;           // [max_batch] duplicate guard of a merge (mmpc_suspend.h): the number of the merge that took the row
    int merge_gen;          // number of the last merge (the stamps start at 0, the numbers at 1)
    int no_lpt_env, force_generic_env;   // MMPC_NO_LPT / MMPC_FORCE_GENERIC, read once at create (diagnostics)
    int *d_warm;            // per instance: 1 once a CONVERGED solve has filled its u_latest / x_guess rows
    // device-side state and staging (capacity max_batch)
    double *d_x_init, *d_traj, *d_uref, *d_obs, *d_ulatest, *d_xguess, *d_X, *d_U, *d_s, *d_cost, *d_err, *d_u0;
    int *d_status, *d_iters;
    int *d_order;           // LPT schedule hint from the previous launch (valid for order_B instances)
    int order_B;
    // persistent plain launch of the specialised kernels (mmpc_set_persistent_grid; the kernel: mmpc_fast_kernel.h)
    int persistent_grid;    // 0: automatic (fast_per_cu x n_cu workgroups), > 0: that many, < 0: one workgroup per instance
    int n_cu;               // compute units of the handle's device
    int *d_ticket;          // the launch-position counter the workgroups draw from: 0 between launches (the kernel puts it back)
    char err[512];
};

static int fail(mmpc_handle h, int code, const char *fmt, const char *a = "", const char *b = "") {
    if (h) snprintf(h->err, sizeof(h->err), fmt, a, b);
    return code;
}
#define HIPCHK(h, call)                                                                   \
    do {                                                                                  \
        hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess) return fail(h, MMPC_E_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)

// doubles of an instance's obstacles, as every solve entry point takes them: static record, table per stage, or motion record
static size_t obs_doubles(mmpc_handle h) {
    const size_t M = (size_t)h->cfg.M;
    return h->hp.obs_per_stage == 2 ? M * 5 : (size_t)(h->hp.obs_per_stage ? h->cfg.N + 1 : 1) * M * 3;
}

static void default_weights(mmpc_handle h) {
    // mpc_wholebody_qref.py:12-16 / mpc_base.py:11-14
    MmpcParams &p = h->hp;
    memset(p.Q2, 0, sizeof(p.Q2)); memset(p.P2, 0, sizeof(p.P2)); memset(p.RW2, 0, sizeof(p.RW2));
    memset(p.R2, 0, sizeof(p.R2)); memset(p.W2, 0, sizeof(p.W2));
    const int nx = h->nx, nu = h->nu;
    if (h->cfg.kind == MMPC_KIND_WHOLEBODY_POSE) {
        // controllers/mpc_wholebody.py:11-15: Q = 5 I4, P = 50 I4 (4x4, leading dimension 4), R, W as the qref controller
        const double r[5] = {0.1, 0.1, 0, 0, 0}, w[5] = {0, 0, 0.1, 0.1, 0.1};
        for (int i = 0; i < 4; i++) { p.Q2[i * 4 + i] = 2 * 5.0; p.P2[i * 4 + i] = 2 * 50.0; }
        for (int i = 0; i < nu; i++) { p.R2[i * nu + i] = 2 * r[i]; p.W2[i * nu + i] = 2 * w[i]; }
    } else if (h->cfg.kind == MMPC_KIND_WHOLEBODY) {
        const double q[9] = {25, 25, 0, 0, 0, 5, 5, 5, 5}, r[5] = {0.1, 0.1, 0, 0, 0}, w[5] = {0, 0, 0.1, 0.1, 0.1};
        for (int i = 0; i < nx; i++) p.Q2[i * nx + i] = p.P2[i * nx + i] = 2 * q[i];
        for (int i = 0; i < nu; i++) { p.R2[i * nu + i] = 2 * r[i]; p.W2[i * nu + i] = 2 * w[i]; }
    } else {
        const double q[6] = {5, 5, 0, 0, 0, 1};
        for (int i = 0; i < nx; i++) p.Q2[i * nx + i] = p.P2[i * nx + i] = 2 * q[i];
        for (int i = 0; i < nu; i++) p.R2[i * nu + i] = 2.0;
    }
    for (int i = 0; i < nu * nu; i++) p.RW2[i] = p.R2[i] + p.W2[i];
    p.S = 1e5;
}

static void update_diag(mmpc_handle h) {
    const MmpcParams &p = h->hp;
    const int nx = h->nx, nu = h->nu;
    int d = 1;
    for (int i = 0; i < nx; i++) for (int j = 0; j < nx; j++) if (i != j && (p.Q2[i * nx + j] != 0.0 || p.P2[i * nx + j] != 0.0)) d = 0;
    for (int i = 0; i < nu; i++) for (int j = 0; j < nu; j++) if (i != j && (p.R2[i * nu + j] != 0.0 || p.W2[i * nu + j] != 0.0)) d = 0;
    h->diag = d;
}

// (waits for the handle's launches in flight - on whatever stream they were made - before the parameter block changes)
static int upload_params(mmpc_handle h) {
    update_diag(h);
    if (h->ev_valid) HIPCHK(h, hipEventSynchronize(h->ev));
    HIPCHK(h, hipMemcpy(h->dp, &h->hp, sizeof(MmpcParams), hipMemcpyHostToDevice));
    return MMPC_OK;
}

#ifdef MMPC_STAMP
// diagnostic build only: read and clear the per-phase cycle accumulators (not part of include/mmpc.h)
extern "C" int mmpc_debug_read_stamps(unsigned long long *out16) {
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(mmpc_stamp_acc), 16 * sizeof(unsigned long long)) != hipSuccess) return -1;
    unsigned long long z[16] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(mmpc_stamp_acc), z, sizeof(z)) != hipSuccess) return -1;
    return 0;
}
#endif
#ifdef MMPC_STAMP_GEN
extern "C" int mmpc_debug_read_gstamps(unsigned long long *out16) {
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(mmpc_gstamp_acc), 16 * sizeof(unsigned long long)) != hipSuccess) return -1;
    unsigned long long z[16] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(mmpc_gstamp_acc), z, sizeof(z)) != hipSuccess) return -1;
    return 0;
}
#endif
#ifdef MMPC_STAMP_INST
// diagnostic build only: the per-instance stamps of the last launch of a specialised kernel, rows 0 .. n - 1 (not part of include/mmpc.h)
extern "C" int mmpc_debug_read_inst_stamps(unsigned long long *out, int n) {
    if (!out || n < 0 || n > MMPC_INST_STAMP_ROWS) return -1;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(mmpc_inst_stamp), (size_t)n * 6 * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
#endif
extern "C" const char *mmpc_version(void) { return "mmpc 0.1 (gfx950)"; }
static thread_local char g_err[512] = "";   // errors of the handle-less entry points (mmpc_ik_*)
extern "C" const char *mmpc_last_error(mmpc_handle h) { return h ? h->err : g_err; }
// this launch uses the specialised kernel (decided per call: weights and the terminal equality change after create)
static bool runs_fast(mmpc_handle h) { return h->fast_fn[0] && h->diag && !h->hp.terminal_xy_eq && !h->force_generic_env; }
extern "C" int mmpc_runs_specialised(mmpc_handle h) { return h ? (runs_fast(h) ? 1 : 0) : MMPC_E_ARG; }
extern "C" int mmpc_problems_per_cu(mmpc_handle h) { return h ? (runs_fast(h) ? h->fast_per_cu : h->per_cu) : MMPC_E_ARG; }
extern "C" int mmpc_lds_bytes(mmpc_handle h) { return h ? (runs_fast(h) ? h->fast_lds_bytes : h->lds_bytes) : MMPC_E_ARG; }

// ---- shape libraries (mmpc_shape.hip): the specialised kernels of one (kind, N, M) each, loaded into the process on request.
// The registry is process-wide, filled under a mutex, and only grows: a library is never unloaded (handles keep pointers into it).
static std::mutex g_shape_mutex;
static std::vector<MmpcShapeDesc> &shape_registry() { static std::vector<MmpcShapeDesc> r; return r; }
static bool find_shape(int kind, int N, int M, MmpcShapeDesc *out) {
    std::lock_guard<std::mutex> lock(g_shape_mutex);
    for (const MmpcShapeDesc &d : shape_registry())
        if (d.kind == kind && d.N == N && d.M == M) { *out = d; return true; }
    return false;
}
static bool listed_shape(int kind, int N, int M) {
#define MMPC_X(K, NN, MM, WW) if (kind == K && N == NN && M == MM) return true;
    MMPC_FAST_LIST(MMPC_X)
#undef MMPC_X
    return false;
}

extern "C" int mmpc_shape_supported(int kind, int N, int M) { return mmpc_fast_shape_ok(kind, N, M) ? 1 : 0; }

extern "C" int mmpc_load_shape_library(const char *path) {
    if (!path || !*path) { snprintf(g_err, sizeof(g_err), "mmpc_load_shape_library: no path"); return MMPC_E_ARG; }
    // (a descriptor is read before anything of the library is trusted; a refused library stays mapped - its kernels are
    //  registered with the HIP runtime at load time - but nothing points into it)
    void *so = dlopen(path, RTLD_NOW | RTLD_LOCAL);
    if (!so) { snprintf(g_err, sizeof(g_err), "mmpc_load_shape_library: cannot open %.200s: %.200s", path, dlerror()); return MMPC_E_ARG; }
    typedef void (*describe_fn)(MmpcShapeDesc *, unsigned long long);
    describe_fn describe = (describe_fn)dlsym(so, MMPC_SHAPE_ENTRY);
    if (!describe) {
        snprintf(g_err, sizeof(g_err), "mmpc_load_shape_library: %.300s is not a shape library (no symbol %s)", path, MMPC_SHAPE_ENTRY);
        return MMPC_E_ARG;
    }
    // the head first (the part of the descriptor that is the same in every version of the sources), the whole descriptor only
    // when the library's magic, tag and descriptor size are this library's own: nothing is written behind `d` by a refused library
    MmpcShapeDesc d;
    memset(&d, 0, sizeof(d));
    describe(&d, sizeof(MmpcShapeHead));
    if (d.head.magic != MMPC_SHAPE_MAGIC) {
        snprintf(g_err, sizeof(g_err), "mmpc_load_shape_library: %.300s is not a shape library (bad descriptor)", path);
        return MMPC_E_ARG;
    }
    if (d.head.source_tag != (unsigned long long)MMPC_SOURCE_TAG) {
        snprintf(g_err, sizeof(g_err), "mmpc_load_shape_library: %.250s was built from other kernel sources (source tag %016llx, this library has %016llx): rebuild it",
                 path, d.head.source_tag, (unsigned long long)MMPC_SOURCE_TAG);
        return MMPC_E_ARG;
    }
    if (d.head.desc_bytes != sizeof(MmpcShapeDesc)) {
        snprintf(g_err, sizeof(g_err), "mmpc_load_shape_library: %.300s is not a shape library (bad descriptor size)", path);
        return MMPC_E_ARG;
    }
    describe(&d, sizeof(d));
    if (!mmpc_fast_shape_ok(d.kind, d.N, d.M)) {
        snprintf(g_err, sizeof(g_err), "mmpc_load_shape_library: %.250s holds shape (%d, %d, %d), outside the specialised envelope (mmpc_shape_supported)",
                 path, d.kind, d.N, d.M);
        return MMPC_E_ARG;
    }
    for (int o = 0; o < 3; o++) for (int c = 0; c < 2; c++) if (!d.fn[o][c]) {
        snprintf(g_err, sizeof(g_err), "mmpc_load_shape_library: %.300s is not a shape library (a kernel is missing)", path);
        return MMPC_E_ARG;
    }
    std::lock_guard<std::mutex> lock(g_shape_mutex);
    for (const MmpcShapeDesc &e : shape_registry())
        if (e.kind == d.kind && e.N == d.N && e.M == d.M) { g_err[0] = 0; return MMPC_OK; }   // the shape is there already: a no-op
    shape_registry().push_back(d);
    g_err[0] = 0;
    return MMPC_OK;
}

// A config becomes its kernels here and nowhere else (cfg, hp and lds_bytes are set): each list is expanded once, the launches
// go through the pointers.  The static-LDS generic instantiation of a listed shape replaces mmpc_solve_kernel<kind>.
static void resolve_kernels(mmpc_handle h) {
    const mmpc_config &c = h->cfg;
    const MmpcParams &p = h->hp;
    h->fast_fn[0] = h->fast_fn[1] = nullptr;   // (no list entry for the shape: no specialised kernel, nothing of its sizes)
    h->fast_lds_bytes = h->state_doubles = h->gscr_doubles = 0;
    h->gen_state_doubles = 0;
    // (the motion mode has run-time-sized instantiations of its own: the mode is a compile-time constant of every kernel)
    const mmpc_gen_fn by_kind[2][3] = {{mmpc_solve_kernel<0>, mmpc_solve_kernel<1>, mmpc_solve_kernel<2>},
                                       {mmpc_solve_kernel<0, 0, -1, 2>, mmpc_solve_kernel<1, 0, -1, 2>, mmpc_solve_kernel<2, 0, -1, 2>}};
    h->gen_fn = by_kind[p.obs_per_stage == 2][c.kind];
    h->gen_dyn_lds = h->lds_bytes;
    h->gen_cont_fn = nullptr;
    // cfg.generic_budget: budgets and continuation on the generic kernel.  The CONT twins exist for the run-time-sized kernels, and
    // the handle runs the run-time-sized one without a budget too: a continued solve and the uninterrupted one are then two
    // instantiations of one template with the same constants (the static-LDS kernels of MMPC_STATIC_LIST are not used)
    if (c.generic_budget) {
        const mmpc_gen_cont_fn cont_by_kind[2][3] = {{mmpc_solve_kernel_cont<0>, mmpc_solve_kernel_cont<1>, mmpc_solve_kernel_cont<2>},
                                                     {mmpc_solve_kernel_cont<0, 2>, mmpc_solve_kernel_cont<1, 2>, mmpc_solve_kernel_cont<2, 2>}};
        h->gen_cont_fn = cont_by_kind[p.obs_per_stage == 2][c.kind];
    }
    if (!c.generic_budget && !getenv("MMPC_NO_STATIC_GENERIC")) {
#define MMPC_X(K, NN, MM, OO, LL, AA)                                                                                      \
        if (c.kind == K && c.N == NN && c.M == MM && p.obs_per_stage == OO && c.L == LL && p.as_written == AA) {             \
            h->gen_fn = mmpc_solve_kernel_static<K, NN, MM, OO, LL, AA>;                                                     \
            h->gen_dyn_lds = 0;                                                                                              \
        }
        MMPC_STATIC_LIST(MMPC_X)
#undef MMPC_X
    }
#define MMPC_X(K, NN, MM, WW)                                                                                              \
    if (c.kind == K && c.N == NN && c.M == MM && c.L == 0) {                                                                 \
        const mmpc_fast_fn by_ops[3][2] = {{mmpc_fast_kernel<K, NN, MM, WW, false, 0>, mmpc_fast_kernel<K, NN, MM, WW, true, 0>},  \
                                           {mmpc_fast_kernel<K, NN, MM, WW, false, 1>, mmpc_fast_kernel<K, NN, MM, WW, true, 1>},  \
                                           {mmpc_fast_kernel<K, NN, MM, WW, false, 2>, mmpc_fast_kernel<K, NN, MM, WW, true, 2>}}; \
        h->fast_fn[0] = by_ops[p.obs_per_stage][0];                                                                          \
        h->fast_fn[1] = by_ops[p.obs_per_stage][1];                                                                          \
        h->state_doubles = mmpc_fast_state_doubles<K, NN>(MM);                                                               \
        h->gscr_doubles = MmpcGainBlock<K, NN>::total;                                                                       \
        h->fast_lds_bytes = mmpc_fast_layout<K, NN>(MM, p.obs_per_stage).total * (int)sizeof(double);                        \
    }
    MMPC_FAST_LIST(MMPC_X)
#undef MMPC_X
    // ... then the loaded shape libraries, for a handle that asked (cfg.specialise): a listed shape always runs its built-in kernels
    MmpcShapeDesc d;
    if (!h->fast_fn[0] && c.specialise && c.L == 0 && c.kind != MMPC_KIND_WHOLEBODY_POSE && !listed_shape(c.kind, c.N, c.M) &&
        find_shape(c.kind, c.N, c.M, &d)) {
        h->fast_fn[0] = d.fn[p.obs_per_stage][0];
        h->fast_fn[1] = d.fn[p.obs_per_stage][1];
        h->state_doubles = d.state_doubles;
        h->gscr_doubles = d.gscr_doubles;
        h->fast_lds_bytes = d.lds_bytes[p.obs_per_stage];
    }
}

extern "C" int mmpc_create(const mmpc_config *cfg, mmpc_handle *out) {
    if (!cfg || !out) return MMPC_E_ARG;
    *out = nullptr;
    if (cfg->kind != MMPC_KIND_WHOLEBODY && cfg->kind != MMPC_KIND_BASE && cfg->kind != MMPC_KIND_WHOLEBODY_POSE) return MMPC_E_ARG;
    if (cfg->N < 1 || cfg->N > 63 || cfg->M < 0 || cfg->M > 16 || cfg->max_batch < 1) return MMPC_E_ARG;
    if (cfg->L < 0 || cfg->L > 8 || (cfg->L > 0 && cfg->kind != MMPC_KIND_WHOLEBODY)) return MMPC_E_ARG;
    if (cfg->obs_per_stage < 0 || cfg->obs_per_stage > 2) return MMPC_E_ARG;
    if (cfg->generic_budget != 0 && cfg->generic_budget != 1) return MMPC_E_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device < 0 || cfg->device >= ndev) return MMPC_E_NODEVICE;
    mmpc_handle h = new (std::nothrow) mmpc_handle_s();
    if (!h) return MMPC_E_ARG;
    memset(h, 0, sizeof(*h));
    h->cfg = *cfg;
    h->nx = cfg->kind != MMPC_KIND_BASE ? 9 : 6;
    h->nu = cfg->kind != MMPC_KIND_BASE ? 5 : 2;
    h->nref = cfg->kind == MMPC_KIND_WHOLEBODY_POSE ? 4 : h->nx;   // reference row: endpoint pose (x,y,z,psi) or the state
    *out = h;  // returned even on failure below so that the caller can read the error text
    HIPCHK(h, hipSetDevice(cfg->device));
    MmpcParams &p = h->hp;
    p.N = cfg->N; p.M = cfg->M; p.obs_per_stage = cfg->obs_per_stage;
    p.max_iter = cfg->max_iter > 0 ? cfg->max_iter : 2000;   // the reference passes ipopt.max_iter 2000 (mpc_wholebody_qref.py:280)
    p.use_xguess = 0; p.terminal_xy_eq = 0; p.u_guess = nullptr;
    p.dt = cfg->dt; p.tol = cfg->tol > 0 ? cfg->tol : 1e-8; p.mu_init = cfg->mu_init > 0 ? cfg->mu_init : 1.0;
    for (int r = 0; r < 2; r++) {
        for (int j = 0; j < 5; j++) { p.ulim[r][j] = cfg->ulim[r][j]; p.dulim[r][j] = cfg->dulim[r][j]; }
        for (int j = 0; j < 9; j++) p.xlim[r][j] = cfg->xlim[r][j];
    }
    p.L = cfg->L;
    for (int j = 0; j < 8; j++) for (int a = 0; a < 6; a++) p.hs[j][a] = j < cfg->L ? cfg->halfspace[j][a] : 0.0;
    const int nhs = (cfg->kind == MMPC_KIND_WHOLEBODY && cfg->L > 0) ? 6 : 0;
    p.as_written = (cfg->kind == MMPC_KIND_WHOLEBODY && cfg->L >= 2 && cfg->as_written) ? 1 : 0;
    const int nq8 = p.as_written ? 6 * (cfg->L - 1) : 0;
    default_weights(h);
    const MmpcLayout L = cfg->kind == MMPC_KIND_WHOLEBODY ? mmpc_layout<0>(cfg->N, cfg->M, p.obs_per_stage, nhs, nq8)
                       : cfg->kind == MMPC_KIND_BASE    ? mmpc_layout<1>(cfg->N, cfg->M, p.obs_per_stage, 0)
                                                        : mmpc_layout<2>(cfg->N, cfg->M, p.obs_per_stage, 0);
    h->lds_bytes = L.total * (int)sizeof(double);
    if (h->lds_bytes > 160 * 1024) return fail(h, MMPC_E_ARG, "problem needs %s bytes of LDS%s", "more than 163840");
    resolve_kernels(h);
    if (h->gen_cont_fn) {
        // (one save area per instance serves both families: the larger of the two states)
        h->gen_state_doubles = mmpc_gen_state(h->nx, h->nu, cfg->N, L.R).total;
        if (h->state_doubles < h->gen_state_doubles) h->state_doubles = h->gen_state_doubles;
        HIPCHK(h, hipFuncSetAttribute((const void *)h->gen_cont_fn, hipFuncAttributeMaxDynamicSharedMemorySize, h->lds_bytes));
    }
    h->per_cu = h->fast_per_cu = 0;
    if (h->gen_dyn_lds) HIPCHK(h, hipFuncSetAttribute((const void *)h->gen_fn, hipFuncAttributeMaxDynamicSharedMemorySize, h->gen_dyn_lds));
    HIPCHK(h, hipOccupancyMaxActiveBlocksPerMultiprocessor(&h->per_cu, h->gen_fn, MMPC_WAVE, h->gen_dyn_lds));
    if (h->fast_fn[0]) HIPCHK(h, hipOccupancyMaxActiveBlocksPerMultiprocessor(&h->fast_per_cu, h->fast_fn[0], MMPC_WAVE, 0));
    const size_t B = (size_t)cfg->max_batch, N = (size_t)cfg->N, nx = (size_t)h->nx, nu = (size_t)h->nu;
    const size_t nobs = obs_doubles(h);
    HIPCHK(h, hipMalloc(&h->dp, sizeof(MmpcParams)));
    HIPCHK(h, hipMalloc(&h->d_x_init, B * nx * 8));
    HIPCHK(h, hipMalloc(&h->d_traj, B * (N + 1) * nx * 8));
    HIPCHK(h, hipMalloc(&h->d_uref, B * N * nu * 8));
    HIPCHK(h, hipMalloc(&h->d_obs, (B * nobs + 1) * 8));
    HIPCHK(h, hipMalloc(&h->d_ulatest, B * N * nu * 8));
    HIPCHK(h, hipMalloc(&h->d_xguess, B * (N + 1) * nx * 8));
    HIPCHK(h, hipMalloc(&h->d_X, B * (N + 1) * nx * 8));
    HIPCHK(h, hipMalloc(&h->d_U, B * N * nu * 8));
    HIPCHK(h, hipMalloc(&h->d_s, B * (N + 1) * 8));
    HIPCHK(h, hipMalloc(&h->d_cost, B * 8));
    HIPCHK(h, hipMalloc(&h->d_err, B * 8));
    HIPCHK(h, hipMalloc(&h->d_u0, B * nu * 8));
    HIPCHK(h, hipMalloc(&h->d_status, B * 4));
    HIPCHK(h, hipMalloc(&h->d_iters, B * 4));
    HIPCHK(h, hipMalloc(&h->d_order, B * 4));
    HIPCHK(h, hipMalloc(&h->d_warm, B * 4));
    HIPCHK(h, hipMalloc(&h->d_key, B * 4));
    HIPCHK(h, hipMalloc(&h->d_ticket, 4));
    HIPCHK(h, hipMemset(h->d_ticket, 0, 4));
    HIPCHK(h, hipDeviceGetAttribute(&h->n_cu, hipDeviceAttributeMultiprocessorCount, cfg->device));
    if (h->fast_fn[0] && h->gscr_doubles) HIPCHK(h, hipMalloc(&h->d_gscr, B * (size_t)h->gscr_doubles * 8));
    h->soc_doubles = mmpc_soc_doubles(cfg->N, h->nx, h->nu, L.NR);
    HIPCHK(h, hipMalloc(&h->d_soc, B * (size_t)h->soc_doubles * 8));
    h->order_B = 0;
    h->hint_on = 1;
    h->no_lpt_env = getenv("MMPC_NO_LPT") != nullptr;
    h->force_generic_env = getenv("MMPC_FORCE_GENERIC") != nullptr;
    HIPCHK(h, hipEventCreateWithFlags(&h->ev, hipEventDisableTiming));
    h->ev_valid = 0; h->last_stream = nullptr;
    HIPCHK(h, hipMemset(h->d_ulatest, 0, B * N * nu * 8));
    HIPCHK(h, hipMemset(h->d_xguess, 0, B * (N + 1) * nx * 8));
    HIPCHK(h, hipMemset(h->d_warm, 0, B * 4));
    int rc = upload_params(h);
    if (rc) return rc;
    h->err[0] = 0;
    return MMPC_OK;
}

extern "C" int mmpc_destroy(mmpc_handle h) {
    if (!h) return MMPC_E_ARG;
    void *ptrs[] = {h->dp, h->d_x_init, h->d_traj, h->d_uref, h->d_obs, h->d_ulatest, h->d_xguess, h->d_X, h->d_U,
                    h->d_s, h->d_cost, h->d_err, h->d_u0, h->d_status, h->d_iters, h->d_order, h->d_warm, h->d_key, h->d_state,
                    h->d_list, h->d_count, h->d_gscr, h->d_soc, h->d_ticket, h->d_list2, h->d_count2, h->d_stamp};
    (void)hipSetDevice(h->cfg.device);
    if (h->ev_valid) (void)hipEventSynchronize(h->ev);
    if (h->ev) (void)hipEventDestroy(h->ev);
    for (void *p : ptrs) if (p) (void)hipFree(p);
    delete h;
    return MMPC_OK;
}

extern "C" int mmpc_set_weights(mmpc_handle h, const double *Q, const double *R, const double *P, double S, const double *W) {
    if (!h) return MMPC_E_ARG;
    const int nx = h->nx, nu = h->nu;
    MmpcParams &p = h->hp;
    const int nq = h->nref;   // Q, P weigh the reference error: nx x nx, or 4 x 4 for the endpoint-pose reference
    if (Q) for (int i = 0; i < nq; i++) for (int j = 0; j < nq; j++) p.Q2[i * nq + j] = Q[i * nq + j] + Q[j * nq + i];
    if (P) for (int i = 0; i < nq; i++) for (int j = 0; j < nq; j++) p.P2[i * nq + j] = P[i * nq + j] + P[j * nq + i];
    if (R) for (int i = 0; i < nu; i++) for (int j = 0; j < nu; j++) p.R2[i * nu + j] = R[i * nu + j] + R[j * nu + i];
    if (W) for (int i = 0; i < nu; i++) for (int j = 0; j < nu; j++) p.W2[i * nu + j] = W[i * nu + j] + W[j * nu + i];
    if (S >= 0) p.S = S;
    for (int i = 0; i < nu * nu; i++) p.RW2[i] = p.R2[i] + p.W2[i];
    if (h->gen_cont_fn) h->resume_B = 0;   // (a continuation re-derives the weights: the save areas belong to the old ones)
    HIPCHK(h, hipSetDevice(h->cfg.device));
    return upload_params(h);
}

extern "C" int mmpc_set_terminal_xy_equality(mmpc_handle h, int on) {
    if (!h) return MMPC_E_ARG;
    if (on && h->cfg.kind == MMPC_KIND_WHOLEBODY_POSE)
        return fail(h, MMPC_E_UNSUPPORTED, "terminal-xy equality%s%s", " is defined on the joint-space reference only (mpc_wholebody_qref.py)");
    h->hp.terminal_xy_eq = on ? 1 : 0;   // handled by the generic kernel (the specialised kernels do not carry it)
    if (h->gen_cont_fn) h->resume_B = 0;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    return upload_params(h);
}

extern "C" int mmpc_reset(mmpc_handle h) {
    if (!h) return MMPC_E_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const size_t n = (size_t)h->cfg.max_batch * h->cfg.N * h->nu * 8;
    if (h->ev_valid) HIPCHK(h, hipEventSynchronize(h->ev));
    HIPCHK(h, hipMemset(h->d_ulatest, 0, n));
    HIPCHK(h, hipMemset(h->d_warm, 0, (size_t)h->cfg.max_batch * 4));
    h->order_B = 0;
    h->resume_B = 0;
    return MMPC_OK;
}

// the device pointers of a batch, as the *_device entry points take them
struct MmpcBatch {
    const double *x_init, *traj, *uref, *ulast, *xguess, *obs;
    double *X, *U, *s;
    int *status, *iters;
    double *cost, *err;
};
// what a launch covers: the whole batch, the instances the budgeted launch before it left suspended (a continuation), or the
// rows of a caller's device list (list launches only: `count` on the device, the grid is `capacity`; `either_family`: the list may
// go to the generic kernel as well - mmpc_solve_rows_device)
enum MmpcCover { MMPC_WHOLE_BATCH, MMPC_CONTINUATION, MMPC_LIST };
struct MmpcMode {
    MmpcCover cover;
    const int *list, *count;
    int capacity;
    bool either_family;
    bool to_end;   // a continuation that ignores the handle's resume budget (the one inside mmpc_solve_batch)
};
static const MmpcMode whole_batch = {MMPC_WHOLE_BATCH, nullptr, nullptr, 0, false, false}, continuation = {MMPC_CONTINUATION, nullptr, nullptr, 0, false, false},
                      continuation_to_end = {MMPC_CONTINUATION, nullptr, nullptr, 0, false, true};

static int launch(mmpc_handle h, int B, const MmpcBatch &a, hipStream_t st, const MmpcMode &mode) {
    const bool resume = mode.cover == MMPC_CONTINUATION;
    const int *ulist = mode.cover == MMPC_LIST ? mode.list : nullptr, *ucount = ulist ? mode.count : nullptr;
    // (the X guess is a launch argument: null = tile(x_init); nothing in the device parameter block changes per launch)
    // a launch on another stream than the previous one waits for it: both touch the handle's schedule hint
    if (h->ev_valid && st != h->last_stream) HIPCHK(h, hipStreamWaitEvent(st, h->ev, 0));
    const bool use_fast = runs_fast(h);
    // a continuation belongs to the budgeted launch right before it (same B, same buffers): anything in between - another
    // launch, a reset, a change of the budget, a first continuation - leaves the save areas and the list stale
    const bool gen_cont = !use_fast && h->gen_cont_fn;   // (cfg.generic_budget: the generic kernel of this launch has a CONT twin)
    if (resume && !((use_fast || gen_cont) && h->d_state && h->resume_B == B && h->resume_fast == (use_fast ? 1 : 0)))
        return fail(h, MMPC_E_UNSUPPORTED, "%s%s", h->gen_cont_fn ? "nothing to resume: the handle's last launch was not a budgeted launch of this batch size on the kernel family this one would run, or the weights / the terminal equality have changed since"
                                                                  : "nothing to resume: the handle's last launch was not a budgeted launch of this batch size on a specialised kernel");
    // resume budget: a continuation gives every suspended instance at most that many iterations and stays valid; a budgeted list
    // launch that could have been a continuation (same B, same family, nothing stale-making since) carries the suspended
    const int rbudget = (resume && !mode.to_end) ? h->resume_budget : 0;
    const bool carry = !resume && ulist && h->resume_budget > 0 && h->budget > 0 && (use_fast || gen_cont) && h->d_state && h->resume_B == B &&
                       h->resume_fast == (use_fast ? 1 : 0);
    h->resume_B = 0;
    // launch order of the workgroups (results do not depend on it): the iteration counts of the handle's previous launch of
    // this batch size when there are any and the mode allows them, else the a-priori difficulty key of THIS batch's data
    if (ulist && !use_fast && !mode.either_family && !gen_cont) return fail(h, MMPC_E_UNSUPPORTED, "%s%s", "list launches need a specialised kernel (this (kind, N, M, weights) runs the generic one)");
    const bool lpt = !resume && !ulist && h->hint_on && !h->no_lpt_env && B <= h->cfg.max_batch && B > 256;
    const bool history = lpt && h->hint_on == 1 && h->order_B == B;
    const int key_planes = (h->cfg.kind == MMPC_KIND_WHOLEBODY && h->hp.L > 0) ? h->hp.L : 0;
    if (lpt && !history && (h->cfg.M > 0 || key_planes)) {
        if (h->hp.obs_per_stage == 2)
            hipLaunchKernelGGL(mmpc_difficulty_key_motion, dim3((B + 63) / 64), dim3(64), 0, st, B, h->cfg.N, h->cfg.M, h->nref, a.traj,
                               a.obs, h->d_key, h->dp, a.x_init, key_planes, h->d_tick);
        else
        hipLaunchKernelGGL(mmpc_difficulty_key, dim3((B + 63) / 64), dim3(64), 0, st, B, h->cfg.N, h->cfg.M, h->nref,
                           h->hp.obs_per_stage, a.traj, a.obs, h->d_key, h->dp, a.x_init, key_planes);
        hipLaunchKernelGGL(mmpc_lpt_order, dim3(1), dim3(MMPC_LPT_THREADS), 0, st, B, h->d_key, h->d_order);
    }
    const int *order = ulist ? ulist : ((history || (lpt && (h->cfg.M > 0 || key_planes))) ? h->d_order : nullptr);
    const int grid = ulist ? mode.capacity : B;
    if (use_fast) {
        // CONT instantiation: the launch may suspend (a budget is set) or continues suspended instances; only it gets the save areas
        const bool cont = resume || h->budget > 0;
        // the plain launch (whole batch, no budget) is persistent: as many workgroups as the chip holds at once, which draw their
        // launch positions from the handle's ticket (mmpc_set_persistent_grid)
        const bool pers = !cont && !ulist && h->persistent_grid >= 0 && h->fast_per_cu > 0 && h->n_cu > 0;
        int pgrid = grid;
        if (pers) {
            const long long room = h->persistent_grid > 0 ? (long long)h->persistent_grid : (long long)h->fast_per_cu * h->n_cu;
            pgrid = room < B ? (int)room : B;
        }
        hipLaunchKernelGGL(h->fast_fn[cont], dim3(resume ? (B < MMPC_RESUME_GRID ? B : MMPC_RESUME_GRID) : pgrid), dim3(MMPC_WAVE), 0, st,
                           h->dp, B, a.x_init, a.traj, a.uref, a.ulast, a.xguess, a.obs, a.X, a.U, a.s, a.status, a.iters, a.cost, a.err,
                           resume ? h->d_list : order, resume ? rbudget : h->budget, cont ? h->d_state : (double *)nullptr,
                           cont ? h->state_doubles : 0, resume ? h->d_count : (const int *)nullptr,
                           resume ? (const int *)nullptr : ucount, h->d_gscr, h->d_soc, h->soc_doubles, h->d_tick,
                           h->scale_max_grad, h->d_scale_out, pers ? h->d_ticket : (int *)nullptr);
    } else if (gen_cont && (resume || h->budget > 0)) {
        hipLaunchKernelGGL(h->gen_cont_fn, dim3(resume ? (B < MMPC_RESUME_GRID ? B : MMPC_RESUME_GRID) : grid), dim3(MMPC_WAVE), h->lds_bytes, st,
                           h->dp, B, a.x_init, a.traj, a.uref, a.ulast, a.xguess, a.obs, a.X, a.U, a.s, a.status, a.iters, a.cost, a.err,
                           resume ? h->d_list : order, h->d_soc, h->soc_doubles, h->d_tick, h->scale_max_grad, h->d_scale_out,
                           resume ? (const int *)nullptr : ucount, resume ? rbudget : h->budget, h->d_state, h->state_doubles,
                           resume ? h->d_count : (const int *)nullptr);
    } else
        hipLaunchKernelGGL(h->gen_fn, dim3(grid), dim3(MMPC_WAVE), h->gen_dyn_lds, st, h->dp, B, a.x_init, a.traj, a.uref, a.ulast,
                           a.xguess, a.obs, a.X, a.U, a.s, a.status, a.iters, a.cost, a.err, order, h->d_soc, h->soc_doubles, h->d_tick,
                           h->scale_max_grad, h->d_scale_out, ucount);
    HIPCHK(h, hipGetLastError());
    if ((use_fast || gen_cont) && h->budget > 0 && !resume) {
        // who is suspended: compacted list for mmpc_resume_batch_device
        if (ulist && h->resume_budget > 0) {
            // resume budget: the carried instances that are still suspended, then the listed ones, every row once (mmpc_suspend.h)
            const int gen = h->merge_gen = h->merge_gen == 0x7fffffff ? 1 : h->merge_gen + 1;
            HIPCHK(h, hipMemsetAsync(h->d_count2, 0, 4, st));
            if (carry) hipLaunchKernelGGL(mmpc_compact_suspended, dim3((B + 255) / 256), dim3(256), 0, st, B, h->d_list, h->d_count, a.status, h->d_list2, h->d_count2, h->d_stamp, gen);
            hipLaunchKernelGGL(mmpc_append_suspended, dim3((mode.capacity + 255) / 256), dim3(256), 0, st, B, ulist, ucount, a.status, h->d_list2, h->d_count2, h->d_stamp, gen);
            std::swap(h->d_list, h->d_list2); std::swap(h->d_count, h->d_count2);
        } else {
            HIPCHK(h, hipMemsetAsync(h->d_count, 0, 4, st));
            if (ulist) hipLaunchKernelGGL(mmpc_collect_suspended_list, dim3((mode.capacity + 255) / 256), dim3(256), 0, st, B, ulist, ucount, a.status, h->d_list, h->d_count);
            else hipLaunchKernelGGL(mmpc_collect_suspended, dim3((B + 255) / 256), dim3(256), 0, st, B, a.status, h->d_list, h->d_count);
        }
        h->resume_B = B;
        h->resume_fast = use_fast ? 1 : 0;
    }
    if (resume && rbudget > 0) {
        // the continuation may have suspended its instances again: the list of those, for the next continuation (same B, same arguments)
        HIPCHK(h, hipMemsetAsync(h->d_count2, 0, 4, st));
        hipLaunchKernelGGL(mmpc_compact_suspended, dim3((B + 255) / 256), dim3(256), 0, st, B, h->d_list, h->d_count, a.status, h->d_list2, h->d_count2, (int *)nullptr, 0);
        std::swap(h->d_list, h->d_list2); std::swap(h->d_count, h->d_count2);
        h->resume_B = B;
        h->resume_fast = use_fast ? 1 : 0;
    }
    if (lpt && h->hint_on == 1) {
        hipLaunchKernelGGL(mmpc_lpt_order, dim3(1), dim3(MMPC_LPT_THREADS), 0, st, B, a.iters, h->d_order);
        h->order_B = B;
    }
    HIPCHK(h, hipEventRecord(h->ev, st));
    h->ev_valid = 1; h->last_stream = st;
    return MMPC_OK;
}

// the argument check the three *_device entry points share (the obstacle table may be null when there are no obstacles)
static bool bad_batch(mmpc_handle h, int B, const MmpcBatch &a) {
    return !h || B < 1 || B > h->cfg.max_batch || !a.x_init || !a.traj || !a.uref || !a.ulast || !a.X || !a.U || !a.s || !a.status ||
           !a.iters || !a.cost || !a.err || (h->cfg.M > 0 && !a.obs);
}
// ... and their launch: on the handle's device, with the handle's (unread) table in place of a null one
static int launch_device(mmpc_handle h, int B, MmpcBatch a, void *stream, const MmpcMode &mode) {
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (!a.obs) a.obs = h->d_obs;
    return launch(h, B, a, (hipStream_t)stream, mode);
}

extern "C" int mmpc_set_iteration_budget(mmpc_handle h, int budget) {
    if (!h || budget < 0) return fail(h, MMPC_E_ARG, "mmpc_set_iteration_budget: %s%s", "budget must be >= 0");
    if (budget > 0 && !h->fast_fn[0] && !h->gen_cont_fn) return fail(h, MMPC_E_UNSUPPORTED, "mmpc_set_iteration_budget: %s%s", "this (kind, N, M) runs the generic kernel, which has no continuation");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (budget > 0 && !h->d_state) {
        const size_t B = (size_t)h->cfg.max_batch;
        if (h->cfg.max_batch > (1 << 20)) return fail(h, MMPC_E_ARG, "%s%s", "iteration budgets need max_batch <= 2^20");
        HIPCHK(h, hipMalloc(&h->d_state, B * (size_t)h->state_doubles * 8));
        HIPCHK(h, hipMalloc(&h->d_list, B * 4));
        HIPCHK(h, hipMalloc(&h->d_count, 4));
        HIPCHK(h, hipMemset(h->d_count, 0, 4));
        // (the second list buffer and the duplicate guard of mmpc_set_resume_budget)
        HIPCHK(h, hipMalloc(&h->d_list2, B * 4));
        HIPCHK(h, hipMalloc(&h->d_count2, 4));
        HIPCHK(h, hipMemset(h->d_count2, 0, 4));
        HIPCHK(h, hipMalloc(&h->d_stamp, B * 4));
        HIPCHK(h, hipMemset(h->d_stamp, 0, B * 4));
    }
    if (h->ev_valid) HIPCHK(h, hipEventSynchronize(h->ev));
    h->budget = budget;
    h->resume_B = 0;
    return MMPC_OK;
}

extern "C" int mmpc_set_resume_budget(mmpc_handle h, int budget) {
    if (!h || budget < 0) return fail(h, MMPC_E_ARG, "mmpc_set_resume_budget: %s%s", "budget must be >= 0");
    if (budget > 0 && !h->fast_fn[0] && !h->gen_cont_fn) return fail(h, MMPC_E_UNSUPPORTED, "mmpc_set_resume_budget: %s%s", "this (kind, N, M) runs the generic kernel, which has no continuation");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (h->ev_valid) HIPCHK(h, hipEventSynchronize(h->ev));
    h->resume_budget = budget;   // (a pending continuation stays valid: a solve is the same bits wherever it is cut)
    return MMPC_OK;
}

extern "C" int mmpc_resume_batch_device(mmpc_handle h, int B, const double *d_x_init, const double *d_traj_ref,
                                        const double *d_u_ref, const double *d_u_last, const double *d_x_guess,
                                        const double *d_obs, double *d_X, double *d_U, double *d_s, int *d_status,
                                        int *d_iters, double *d_cost, double *d_err, void *stream) {
    if (h && B == 0) return MMPC_OK;   // an empty batch (e.g. the shard of a rank beyond the batch) is a no-op
    const MmpcBatch a = {d_x_init, d_traj_ref, d_u_ref, d_u_last, d_x_guess, d_obs, d_X, d_U, d_s, d_status, d_iters, d_cost, d_err};
    if (bad_batch(h, B, a)) return fail(h, MMPC_E_ARG, "mmpc_resume_batch_device: %s%s", "bad argument");
    return launch_device(h, B, a, stream, continuation);
}

extern "C" int mmpc_suspended_count(mmpc_handle h, int *count) {
    if (!h || !count) return MMPC_E_ARG;
    *count = 0;
    if (!h->d_count) return MMPC_OK;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (h->ev_valid) HIPCHK(h, hipEventSynchronize(h->ev));
    HIPCHK(h, hipMemcpy(count, h->d_count, 4, hipMemcpyDeviceToHost));
    return MMPC_OK;
}

extern "C" int mmpc_set_schedule_hint(mmpc_handle h, int on) {
    if (!h) return MMPC_E_ARG;
    if (on < 0 || on > 2) return fail(h, MMPC_E_ARG, "mmpc_set_schedule_hint: %s%s", "mode must be 0, 1 or 2");
    h->hint_on = on;
    h->order_B = 0;
    return MMPC_OK;
}

extern "C" int mmpc_set_persistent_grid(mmpc_handle h, int n) {
    if (!h) return MMPC_E_ARG;
    h->persistent_grid = n;   // (read by the next launch; launches in flight have their grid already)
    return MMPC_OK;
}

extern "C" int mmpc_set_warm_start(mmpc_handle h, const double *d_u_guess, double mu_init) {
    if (!h || !(mu_init > 0.0)) return fail(h, MMPC_E_ARG, "mmpc_set_warm_start: %s%s", "mu_init must be positive");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    h->hp.u_guess = d_u_guess;
    h->hp.mu_init = mu_init;
    return upload_params(h);
}

extern "C" int mmpc_set_obstacle_clock(mmpc_handle h, const long long *d_tick) {
    if (!h) return MMPC_E_ARG;
    if (h->hp.obs_per_stage != 2)
        return fail(h, MMPC_E_UNSUPPORTED, "mmpc_set_obstacle_clock: %s%s", "needs a handle created with obs_per_stage = 2 (motion record)");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    // (the kernels read the array at launch time: wait for the handle's launches in flight before the pointer they were given goes)
    if (h->ev_valid) HIPCHK(h, hipEventSynchronize(h->ev));
    h->d_tick = d_tick;
    return MMPC_OK;
}

extern "C" int mmpc_set_objective_scaling(mmpc_handle h, double max_gradient, double *d_scale_out) {
    if (!h) return MMPC_E_ARG;
    if (!(max_gradient >= 0.0) || !(max_gradient <= 1.79769313486231570815e308))   // (negative, NaN, infinite)
        return fail(h, MMPC_E_ARG, "mmpc_set_objective_scaling: %s%s", "max_gradient must be 0 (off) or a positive finite number");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    // (the kernels write d_scale_out: wait for the handle's launches in flight before the pointer they were given goes)
    if (h->ev_valid) HIPCHK(h, hipEventSynchronize(h->ev));
    h->scale_max_grad = max_gradient;
    h->d_scale_out = max_gradient > 0.0 ? d_scale_out : nullptr;
    return MMPC_OK;
}

extern "C" int mmpc_solve_batch_device(mmpc_handle h, int B, const double *d_x_init, const double *d_traj_ref,
                                       const double *d_u_ref, const double *d_u_last, const double *d_x_guess,
                                       const double *d_obs, double *d_X, double *d_U, double *d_s, int *d_status,
                                       int *d_iters, double *d_cost, double *d_err, void *stream) {
    if (h && B == 0) return MMPC_OK;   // an empty batch (e.g. the shard of a rank beyond the batch) is a no-op
    // B > max_batch: the handle's per-instance buffers (launch order, difficulty keys, save areas of suspended solves, list of
    // the suspended, the opt-in U guess) are sized for max_batch instances
    const MmpcBatch a = {d_x_init, d_traj_ref, d_u_ref, d_u_last, d_x_guess, d_obs, d_X, d_U, d_s, d_status, d_iters, d_cost, d_err};
    if (bad_batch(h, B, a)) return fail(h, MMPC_E_ARG, "mmpc_solve_batch_device: %s%s", "bad argument (B must be in 1..max_batch)");
    return launch_device(h, B, a, stream, whole_batch);
}

extern "C" int mmpc_solve_list_device(mmpc_handle h, int B, const int *d_list, const int *d_count, int capacity, const double *d_x_init,
                                      const double *d_traj_ref, const double *d_u_ref, const double *d_u_last, const double *d_x_guess,
                                      const double *d_obs, double *d_X, double *d_U, double *d_s, int *d_status, int *d_iters,
                                      double *d_cost, double *d_err, void *stream) {
    const MmpcBatch a = {d_x_init, d_traj_ref, d_u_ref, d_u_last, d_x_guess, d_obs, d_X, d_U, d_s, d_status, d_iters, d_cost, d_err};
    if (bad_batch(h, B, a) || !d_list || !d_count || capacity < 1 || capacity > B)
        return fail(h, MMPC_E_ARG, "mmpc_solve_list_device: %s%s", "bad argument (B in 1..max_batch, 1 <= capacity <= B)");
    return launch_device(h, B, a, stream, MmpcMode{MMPC_LIST, d_list, d_count, capacity, false});
}

extern "C" int mmpc_solve_rows_device(mmpc_handle h, int B, const int *d_list, const int *d_count, int capacity, const double *d_x_init,
                                      const double *d_traj_ref, const double *d_u_ref, const double *d_u_last, const double *d_x_guess,
                                      const double *d_obs, double *d_X, double *d_U, double *d_s, int *d_status, int *d_iters,
                                      double *d_cost, double *d_err, void *stream) {
    const MmpcBatch a = {d_x_init, d_traj_ref, d_u_ref, d_u_last, d_x_guess, d_obs, d_X, d_U, d_s, d_status, d_iters, d_cost, d_err};
    if (bad_batch(h, B, a) || !d_list || !d_count || capacity < 1 || capacity > B)
        return fail(h, MMPC_E_ARG, "mmpc_solve_rows_device: %s%s", "bad argument (B in 1..max_batch, 1 <= capacity <= B)");
    if (h->budget > 0 && !h->gen_cont_fn)
        return fail(h, MMPC_E_UNSUPPORTED, "mmpc_solve_rows_device: %s%s", "the handle has an iteration budget set (continuations belong to mmpc_solve_list_device)");
    return launch_device(h, B, a, stream, MmpcMode{MMPC_LIST, d_list, d_count, capacity, true});
}

extern "C" int mmpc_solve_batch(mmpc_handle h, int B, const double *x_init, const double *traj_ref, const double *u_ref,
                                const double *obs, double *out_u0, double *out_X, double *out_U, double *out_s,
                                int *out_status, int *out_iters, double *out_cost) {
    if (h && B == 0) return MMPC_OK;   // an empty batch (e.g. the shard of a rank beyond the batch) is a no-op
    if (!h || B < 1 || B > h->cfg.max_batch || !x_init || !traj_ref || !u_ref || !out_u0 || (h->cfg.M > 0 && !obs))
        return fail(h, MMPC_E_ARG, "mmpc_solve_batch: %s%s", "bad argument (B must be in 1..max_batch)");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const size_t N = (size_t)h->cfg.N, nx = (size_t)h->nx, nu = (size_t)h->nu, b = (size_t)B;
    const size_t nobs = obs_doubles(h);
    hipStream_t st = 0;
    HIPCHK(h, hipMemcpyAsync(h->d_x_init, x_init, b * nx * 8, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(h->d_traj, traj_ref, b * (N + 1) * (size_t)h->nref * 8, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(h->d_uref, u_ref, b * N * nu * 8, hipMemcpyHostToDevice, st));
    if (nobs) HIPCHK(h, hipMemcpyAsync(h->d_obs, obs, b * nobs * 8, hipMemcpyHostToDevice, st));
    // the base kind and the pose-reference kind warm-start X as well (mpc_base.py:194-201, mpc_wholebody.py:134-139); the
    // joint-reference whole-body controller never does (mpc_wholebody_qref.py:301-302)
    const double *xg = nullptr;
    if (h->cfg.kind != MMPC_KIND_WHOLEBODY) {
        if (h->ev_valid && st != h->last_stream) HIPCHK(h, hipStreamWaitEvent(st, h->ev, 0));
        hipLaunchKernelGGL(mmpc_cold_xguess, dim3(B), dim3(64), 0, st, B, (int)N + 1, (int)nx, h->cfg.kind != MMPC_KIND_BASE ? 1 : 0,
                           h->dp, h->d_warm, h->d_x_init, h->d_xguess);
        xg = h->d_xguess;
    }
    const MmpcBatch a = {h->d_x_init, h->d_traj, h->d_uref, h->d_ulatest, xg, h->d_obs, h->d_X, h->d_U, h->d_s,
                         h->d_status, h->d_iters, h->d_cost, h->d_err};
    int rc = launch(h, B, a, st, whole_batch);
    if (rc) return rc;
    if (h->budget > 0 && (h->fast_fn[0] || h->gen_cont_fn) && h->d_state) {   // the host-pointer call returns finished solves: continue the suspended ones at once
        rc = launch(h, B, a, st, continuation_to_end);   // (to the end whatever the resume budget is)
        if (rc && rc != MMPC_E_UNSUPPORTED) return rc;
    }
    // u_latest <- U*, x_guess <- X*  (:329-330), for the instances that converged
    hipLaunchKernelGGL(mmpc_keep_converged, dim3(B), dim3(64), 0, st, B, (int)(N * nu), (int)((N + 1) * nx), h->d_status, h->d_U,
                       h->d_X, h->d_ulatest, h->d_xguess, h->d_warm);
    hipLaunchKernelGGL(mmpc_gather_u0, dim3((B * (int)nu + 255) / 256), dim3(256), 0, st, B, (int)nu, (int)(N * nu), h->d_U, h->d_u0);
    HIPCHK(h, hipMemcpyAsync(out_u0, h->d_u0, b * nu * 8, hipMemcpyDeviceToHost, st));
    if (out_X) HIPCHK(h, hipMemcpyAsync(out_X, h->d_X, b * (N + 1) * nx * 8, hipMemcpyDeviceToHost, st));
    if (out_U) HIPCHK(h, hipMemcpyAsync(out_U, h->d_U, b * N * nu * 8, hipMemcpyDeviceToHost, st));
    if (out_s) HIPCHK(h, hipMemcpyAsync(out_s, h->d_s, b * (N + 1) * 8, hipMemcpyDeviceToHost, st));
    if (out_status) HIPCHK(h, hipMemcpyAsync(out_status, h->d_status, b * 4, hipMemcpyDeviceToHost, st));
    if (out_iters) HIPCHK(h, hipMemcpyAsync(out_iters, h->d_iters, b * 4, hipMemcpyDeviceToHost, st));
    if (out_cost) HIPCHK(h, hipMemcpyAsync(out_cost, h->d_cost, b * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipEventRecord(h->ev, st));
    HIPCHK(h, hipStreamSynchronize(st));
    return MMPC_OK;
}

extern "C" int mmpc_get_u_latest(mmpc_handle h, int B, double *u_latest) {
    if (!h || !u_latest || B < 1 || B > h->cfg.max_batch) return MMPC_E_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (h->ev_valid) HIPCHK(h, hipEventSynchronize(h->ev));
    HIPCHK(h, hipMemcpy(u_latest, h->d_ulatest, (size_t)B * h->cfg.N * h->nu * 8, hipMemcpyDeviceToHost));
    return MMPC_OK;
}
extern "C" int mmpc_set_u_latest(mmpc_handle h, int B, const double *u_latest) {
    if (!h || !u_latest || B < 1 || B > h->cfg.max_batch) return MMPC_E_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (h->ev_valid) HIPCHK(h, hipEventSynchronize(h->ev));
    HIPCHK(h, hipMemcpy(h->d_ulatest, u_latest, (size_t)B * h->cfg.N * h->nu * 8, hipMemcpyHostToDevice));
    return MMPC_OK;
}

// ---- batched inverse kinematics of the arm (manipulator_3DoF.py:79-133): one lane per instance, stateless
__global__ __launch_bounds__(256) void mmpc_ik_kernel(int B, const double *__restrict__ q0, const double *__restrict__ target,
                                                      double *__restrict__ q, int *__restrict__ status, int *__restrict__ iters) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double qi[3] = {q0[3 * b], q0[3 * b + 1], q0[3 * b + 2]};
    double qo[3];
    int it = 0;
    const int st = mmpc_ik_solve(qi, target[2 * b], target[2 * b + 1], qo, &it);
    q[3 * b] = qo[0]; q[3 * b + 1] = qo[1]; q[3 * b + 2] = qo[2];
    if (status) status[b] = st;
    if (iters) iters[b] = it;
}

#define IKCHK(call)                                                                                              \
    do {                                                                                                         \
        hipError_t e_ = (call);                                                                                  \
        if (e_ != hipSuccess) { snprintf(g_err, sizeof(g_err), "%s: %s", #call, hipGetErrorString(e_)); return MMPC_E_HIP; } \
    } while (0)

extern "C" int mmpc_ik_batch_device(int device, int B, const double *d_q0, const double *d_target_xz, double *d_q,
                                    int *d_status, int *d_iters, void *stream) {
    if (B < 0 || !d_q0 || !d_target_xz || !d_q) { snprintf(g_err, sizeof(g_err), "mmpc_ik_batch_device: bad argument"); return MMPC_E_ARG; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        snprintf(g_err, sizeof(g_err), "no HIP device %d (this library has no CPU fallback)", device);
        return MMPC_E_NODEVICE;
    }
    if (B == 0) return MMPC_OK;
    IKCHK(hipSetDevice(device));
    hipLaunchKernelGGL(mmpc_ik_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, B, d_q0, d_target_xz, d_q, d_status, d_iters);
    IKCHK(hipGetLastError());
    return MMPC_OK;
}

extern "C" int mmpc_ik_batch(int device, int B, const double *q0, const double *target_xz, double *out_q, int *out_status,
                             int *out_iters) {
    if (B < 0 || !q0 || !target_xz || !out_q) { snprintf(g_err, sizeof(g_err), "mmpc_ik_batch: bad argument"); return MMPC_E_ARG; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        snprintf(g_err, sizeof(g_err), "no HIP device %d (this library has no CPU fallback)", device);
        return MMPC_E_NODEVICE;
    }
    if (B == 0) return MMPC_OK;
    IKCHK(hipSetDevice(device));
    double *d_q0 = nullptr, *d_t = nullptr, *d_q = nullptr;
    int *d_st = nullptr, *d_it = nullptr;
    int rc = MMPC_OK;
    hipError_t e = hipSuccess;
    if ((e = hipMalloc(&d_q0, (size_t)B * 24)) == hipSuccess && (e = hipMalloc(&d_t, (size_t)B * 16)) == hipSuccess &&
        (e = hipMalloc(&d_q, (size_t)B * 24)) == hipSuccess && (e = hipMalloc(&d_st, (size_t)B * 4)) == hipSuccess &&
        (e = hipMalloc(&d_it, (size_t)B * 4)) == hipSuccess &&
        (e = hipMemcpy(d_q0, q0, (size_t)B * 24, hipMemcpyHostToDevice)) == hipSuccess &&
        (e = hipMemcpy(d_t, target_xz, (size_t)B * 16, hipMemcpyHostToDevice)) == hipSuccess) {
        rc = mmpc_ik_batch_device(device, B, d_q0, d_t, d_q, d_st, d_it, nullptr);
        if (rc == MMPC_OK && (e = hipDeviceSynchronize()) == hipSuccess && (e = hipMemcpy(out_q, d_q, (size_t)B * 24, hipMemcpyDeviceToHost)) == hipSuccess) {
            if (out_status) e = hipMemcpy(out_status, d_st, (size_t)B * 4, hipMemcpyDeviceToHost);
            if (e == hipSuccess && out_iters) e = hipMemcpy(out_iters, d_it, (size_t)B * 4, hipMemcpyDeviceToHost);
        }
    }
    if (e != hipSuccess) { snprintf(g_err, sizeof(g_err), "mmpc_ik_batch: %s", hipGetErrorString(e)); rc = MMPC_E_HIP; }
    (void)hipFree(d_q0); (void)hipFree(d_t); (void)hipFree(d_q); (void)hipFree(d_st); (void)hipFree(d_it);
    return rc;
}

// ---- the glue of a receding-horizon tick (mmpc_tick.h): one workgroup per robot, whole-body kind with a per-stage obstacle table
__global__ __launch_bounds__(MMPC_WAVE) void mmpc_tick_kernel(
    const MmpcParams *__restrict__ Pp, int B, double *__restrict__ x, long long *__restrict__ tick, const double *__restrict__ U_prev,
    const double *__restrict__ glob, int nglob, const double *__restrict__ obs0, const double *__restrict__ vel,
    double *__restrict__ x_in, double *__restrict__ traj_ref, int *__restrict__ start, double *__restrict__ obs,
    double *__restrict__ u_guess, double *__restrict__ x_guess) {
    __shared__ double lds[MMPC_TICK_LDS];
    const int b = (int)blockIdx.x;
    if (b >= B) return;
    mmpc_tick_robot(*Pp, b, x, tick, U_prev, glob, nglob, obs0, vel, x_in, traj_ref, start, obs, u_guess, x_guess, lds);
}

extern "C" int mmpc_tick_prepare_device(mmpc_handle h, int B, double *d_x, long long *d_tick, const double *d_U_prev,
                                        const double *d_glob, int nglob, const double *d_obs0, const double *d_vel, double *d_x_in,
                                        double *d_traj_ref, int *d_start, double *d_obs, double *d_u_guess, double *d_x_guess,
                                        void *stream) {
    if (!h) return MMPC_E_ARG;
    if (h->cfg.kind != MMPC_KIND_WHOLEBODY || !h->hp.obs_per_stage)
        return fail(h, MMPC_E_UNSUPPORTED, "mmpc_tick_prepare_device: %s%s", "needs a whole-body handle (joint-space reference) created with obs_per_stage = 1 or 2");
    if (h->hp.obs_per_stage == 2 && d_obs)
        return fail(h, MMPC_E_ARG, "mmpc_tick_prepare_device: %s%s", "d_obs must be NULL on a motion handle (obs_per_stage = 2): the kernels form the centres from the record and the clock");
    if (B == 0) return MMPC_OK;
    if (B < 1 || B > h->cfg.max_batch) return fail(h, MMPC_E_ARG, "mmpc_tick_prepare_device: %s%s", "B must be in 0..max_batch");
    if (!d_x) return fail(h, MMPC_E_ARG, "mmpc_tick_prepare_device: %s%s", "d_x is required");
    if (!d_tick && (d_U_prev || d_obs)) return fail(h, MMPC_E_ARG, "mmpc_tick_prepare_device: %s%s", "the advance and the obstacle table need d_tick");
    if ((d_traj_ref || d_start) && !d_glob) return fail(h, MMPC_E_ARG, "mmpc_tick_prepare_device: %s%s", "the window and the start index need d_glob");
    if (d_glob && (nglob < 1 || nglob > (1 << 24))) return fail(h, MMPC_E_ARG, "mmpc_tick_prepare_device: %s%s", "nglob must be in 1..2^24");
    if (d_obs && h->cfg.M > 0 && (!d_obs0 || !d_vel)) return fail(h, MMPC_E_ARG, "mmpc_tick_prepare_device: %s%s", "the obstacle table needs d_obs0 and d_vel");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipStream_t st = (hipStream_t)stream;
    // ordered against the handle's launches as they are among themselves: the solve reads what this writes (and the registered
    // u_guess), the next call of this reads the solve's U
    if (h->ev_valid && st != h->last_stream) HIPCHK(h, hipStreamWaitEvent(st, h->ev, 0));
    hipLaunchKernelGGL(mmpc_tick_kernel, dim3(B), dim3(MMPC_WAVE), 0, st, h->dp, B, d_x, d_tick, d_U_prev, d_glob, nglob, d_obs0, d_vel, d_x_in,
                       d_traj_ref, d_start, d_obs, d_u_guess, d_x_guess);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(h->ev, st));
    h->ev_valid = 1; h->last_stream = st;
    return MMPC_OK;
}

// ---- the same with the reference's task state machine per robot (mmpc_mission.h): phases, and the per-phase lists of robots to solve
__global__ __launch_bounds__(MMPC_WAVE) void mmpc_mission_kernel(
    const MmpcParams *__restrict__ Pp, int B, double *__restrict__ x, long long *__restrict__ tick, int *__restrict__ phase,
    const double *__restrict__ U_prev, const double *__restrict__ glob, int nglob, const double *__restrict__ obs0,
    const double *__restrict__ vel, double *__restrict__ x_in, double *__restrict__ traj_ref, int *__restrict__ start,
    double *__restrict__ obs, int *__restrict__ lists, int *__restrict__ counts) {
    __shared__ double lds[MMPC_TICK_LDS];
    const int b = (int)blockIdx.x;
    if (b >= B) return;
    mmpc_mission_robot(*Pp, b, B, x, tick, phase, U_prev, glob, nglob, obs0, vel, x_in, traj_ref, start, obs, lists, counts, lds);
}

extern "C" int mmpc_mission_prepare_device(mmpc_handle h, int B, double *d_x, long long *d_tick, int *d_phase, const double *d_U_prev,
                                           const double *d_glob, int nglob, const double *d_obs0, const double *d_vel, double *d_x_in,
                                           double *d_traj_ref, int *d_start, double *d_obs, int *d_lists, int *d_counts, void *stream) {
    if (!h) return MMPC_E_ARG;
    if (h->cfg.kind != MMPC_KIND_WHOLEBODY || !h->hp.obs_per_stage)
        return fail(h, MMPC_E_UNSUPPORTED, "mmpc_mission_prepare_device: %s%s", "needs a whole-body handle (joint-space reference) created with obs_per_stage = 1 or 2");
    if (h->hp.obs_per_stage == 2 && d_obs)
        return fail(h, MMPC_E_ARG, "mmpc_mission_prepare_device: %s%s", "d_obs must be NULL on a motion handle (obs_per_stage = 2): the kernels form the centres from the record and the clock");
    if (B == 0) return MMPC_OK;
    if (B < 1 || B > h->cfg.max_batch) return fail(h, MMPC_E_ARG, "mmpc_mission_prepare_device: %s%s", "B must be in 0..max_batch");
    if (!d_x) return fail(h, MMPC_E_ARG, "mmpc_mission_prepare_device: %s%s", "d_x is required");
    if (!d_phase || !d_lists || !d_counts) return fail(h, MMPC_E_ARG, "mmpc_mission_prepare_device: %s%s", "d_phase, d_lists and d_counts are required");
    if (!d_tick && (d_U_prev || d_obs)) return fail(h, MMPC_E_ARG, "mmpc_mission_prepare_device: %s%s", "the advance and the obstacle table need d_tick");
    if (!d_glob || nglob < 1 || nglob > (1 << 24)) return fail(h, MMPC_E_ARG, "mmpc_mission_prepare_device: %s%s", "d_glob is required, nglob must be in 1..2^24");
    if (d_obs && h->cfg.M > 0 && (!d_obs0 || !d_vel)) return fail(h, MMPC_E_ARG, "mmpc_mission_prepare_device: %s%s", "the obstacle table needs d_obs0 and d_vel");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipStream_t st = (hipStream_t)stream;
    if (h->ev_valid && st != h->last_stream) HIPCHK(h, hipStreamWaitEvent(st, h->ev, 0));
    HIPCHK(h, hipMemsetAsync(d_counts, 0, 4 * sizeof(int), st));
    hipLaunchKernelGGL(mmpc_mission_kernel, dim3(B), dim3(MMPC_WAVE), 0, st, h->dp, B, d_x, d_tick, d_phase, d_U_prev, d_glob, nglob, d_obs0,
                       d_vel, d_x_in, d_traj_ref, d_start, d_obs, d_lists, d_counts);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(h->ev, st));
    h->ev_valid = 1; h->last_stream = st;
    return MMPC_OK;
}

// ---- the manipulate phase of a mission (mmpc_manipulate.h): the robots the mission kernel left at 'move finish', IK at the transition
__global__ __launch_bounds__(MMPC_WAVE) void mmpc_manipulate_kernel(
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

extern "C" int mmpc_manipulate_prepare_device(mmpc_handle h, int B, double *d_x, long long *d_tick, int *d_phase, const double *d_U_prev,
                                              const double *d_pose, int nplan, double *d_plan, double *d_qgoal, int *d_ik_status,
                                              const double *d_obs0, const double *d_vel, double *d_x_in, double *d_traj_ref, int *d_start,
                                              double *d_obs, int *d_list, int *d_counts, void *stream) {
    if (!h) return MMPC_E_ARG;
    if (h->cfg.kind != MMPC_KIND_WHOLEBODY || !h->hp.obs_per_stage)
        return fail(h, MMPC_E_UNSUPPORTED, "mmpc_manipulate_prepare_device: %s%s", "needs a whole-body handle (joint-space reference) created with obs_per_stage = 1 or 2");
    if (h->hp.obs_per_stage == 2 && d_obs)
        return fail(h, MMPC_E_ARG, "mmpc_manipulate_prepare_device: %s%s", "d_obs must be NULL on a motion handle (obs_per_stage = 2): the kernels form the centres from the record and the clock");
    if (B == 0) return MMPC_OK;
    if (B < 1 || B > h->cfg.max_batch) return fail(h, MMPC_E_ARG, "mmpc_manipulate_prepare_device: %s%s", "B must be in 0..max_batch");
    if (!d_x) return fail(h, MMPC_E_ARG, "mmpc_manipulate_prepare_device: %s%s", "d_x is required");
    if (!d_phase || !d_pose || !d_plan || !d_list || !d_counts)
        return fail(h, MMPC_E_ARG, "mmpc_manipulate_prepare_device: %s%s", "d_phase, d_pose, d_plan, d_list and d_counts are required");
    if (nplan < 2 || nplan > (1 << 16)) return fail(h, MMPC_E_ARG, "mmpc_manipulate_prepare_device: %s%s", "nplan must be in 2..2^16");
    if (!d_tick && (d_U_prev || d_obs)) return fail(h, MMPC_E_ARG, "mmpc_manipulate_prepare_device: %s%s", "the advance and the obstacle table need d_tick");
    if (d_obs && h->cfg.M > 0 && (!d_obs0 || !d_vel)) return fail(h, MMPC_E_ARG, "mmpc_manipulate_prepare_device: %s%s", "the obstacle table needs d_obs0 and d_vel");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipStream_t st = (hipStream_t)stream;
    if (h->ev_valid && st != h->last_stream) HIPCHK(h, hipStreamWaitEvent(st, h->ev, 0));
    HIPCHK(h, hipMemsetAsync(d_counts, 0, 2 * sizeof(int), st));
    hipLaunchKernelGGL(mmpc_manipulate_kernel, dim3(B), dim3(MMPC_WAVE), 0, st, h->dp, B, d_x, d_tick, d_phase, d_U_prev, d_pose, nplan, d_plan,
                       d_qgoal, d_ik_status, d_obs0, d_vel, d_x_in, d_traj_ref, d_start, d_obs, d_list, d_counts);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(h->ev, st));
    h->ev_valid = 1; h->last_stream = st;
    return MMPC_OK;
}

// ---- the shifted warm start of a mission tick (mmpc_guess.h): step 6 of the tick kernel for the robots the tick solves
__global__ __launch_bounds__(MMPC_WAVE) void mmpc_guess_kernel(
    const MmpcParams *__restrict__ Pp, int B, const int *__restrict__ phase, const double *__restrict__ U_prev,
    const double *__restrict__ x_in, double *__restrict__ u_guess, double *__restrict__ x_guess) {
    const int b = (int)blockIdx.x;
    if (b >= B) return;
    mmpc_guess_robot(*Pp, b, phase, U_prev, x_in, u_guess, x_guess);
}

extern "C" int mmpc_shift_guess_device(mmpc_handle h, int B, const int *d_phase, const double *d_U_prev, const double *d_x_in,
                                       double *d_u_guess, double *d_x_guess, void *stream) {
    if (!h) return MMPC_E_ARG;
    if (h->cfg.kind != MMPC_KIND_WHOLEBODY)
        return fail(h, MMPC_E_UNSUPPORTED, "mmpc_shift_guess_device: %s%s", "needs a whole-body handle (joint-space reference)");
    if (B == 0) return MMPC_OK;
    if (B < 1 || B > h->cfg.max_batch) return fail(h, MMPC_E_ARG, "mmpc_shift_guess_device: %s%s", "B must be in 0..max_batch");
    if (!d_U_prev || !d_x_in || !d_u_guess || !d_x_guess)
        return fail(h, MMPC_E_ARG, "mmpc_shift_guess_device: %s%s", "d_U_prev, d_x_in, d_u_guess and d_x_guess are required");
    if (d_u_guess == d_U_prev) return fail(h, MMPC_E_ARG, "mmpc_shift_guess_device: %s%s", "d_u_guess must not be d_U_prev");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipStream_t st = (hipStream_t)stream;
    if (h->ev_valid && st != h->last_stream) HIPCHK(h, hipStreamWaitEvent(st, h->ev, 0));
    hipLaunchKernelGGL(mmpc_guess_kernel, dim3(B), dim3(MMPC_WAVE), 0, st, h->dp, B, d_phase, d_U_prev, d_x_in, d_u_guess, d_x_guess);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(h->ev, st));
    h->ev_valid = 1; h->last_stream = st;
    return MMPC_OK;
}

// ---- missions under iteration budgets (mmpc_round.h): the mission and manipulate kernels per robot under a hold word, and the commit
__global__ __launch_bounds__(MMPC_WAVE) void mmpc_mission_round_kernel(
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

// the checks mmpc_mission_round_device and mmpc_manipulate_round_device share with the prepare calls (nullptr: fine)
static const char *round_bad(mmpc_handle h, int B, const double *d_x, const long long *d_tick, const int *d_phase, const double *d_U_last,
                             const double *d_obs0, const double *d_vel, const double *d_obs, const int *d_hold, const int *d_solve_phase,
                             long long tick_limit) {
    if (B < 1 || B > h->cfg.max_batch) return "B must be in 0..max_batch";
    if (!d_x || !d_tick || !d_phase) return "d_x, d_tick and d_phase are required";
    if (!d_U_last || !d_hold || !d_solve_phase) return "d_U_last, d_hold and d_solve_phase are required";
    if (tick_limit < 1) return "tick_limit must be at least 1";
    if (d_obs && h->cfg.M > 0 && (!d_obs0 || !d_vel)) return "the obstacle table needs d_obs0 and d_vel";
    return nullptr;
}

extern "C" int mmpc_mission_round_device(mmpc_handle h, int B, double *d_x, long long *d_tick, int *d_phase, const double *d_U_last,
                                         const double *d_glob, int nglob, const double *d_obs0, const double *d_vel, double *d_x_in,
                                         double *d_traj_ref, int *d_start, double *d_obs, int *d_lists, int *d_counts, int *d_hold,
                                         int *d_solve_phase, long long tick_limit, void *stream) {
    if (!h) return MMPC_E_ARG;
    if (h->cfg.kind != MMPC_KIND_WHOLEBODY || !h->hp.obs_per_stage)
        return fail(h, MMPC_E_UNSUPPORTED, "mmpc_mission_round_device: %s%s", "needs a whole-body handle (joint-space reference) created with obs_per_stage = 1 or 2");
    if (h->hp.obs_per_stage == 2 && d_obs)
        return fail(h, MMPC_E_ARG, "mmpc_mission_round_device: %s%s", "d_obs must be NULL on a motion handle (obs_per_stage = 2): the kernels form the centres from the record and the clock");
    if (B == 0) return MMPC_OK;
    if (const char *why = round_bad(h, B, d_x, d_tick, d_phase, d_U_last, d_obs0, d_vel, d_obs, d_hold, d_solve_phase, tick_limit))
        return fail(h, MMPC_E_ARG, "mmpc_mission_round_device: %s%s", why);
    if (!d_lists || !d_counts) return fail(h, MMPC_E_ARG, "mmpc_mission_round_device: %s%s", "d_lists and d_counts are required");
    if (!d_glob || nglob < 1 || nglob > (1 << 24)) return fail(h, MMPC_E_ARG, "mmpc_mission_round_device: %s%s", "d_glob is required, nglob must be in 1..2^24");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipStream_t st = (hipStream_t)stream;
    if (h->ev_valid && st != h->last_stream) HIPCHK(h, hipStreamWaitEvent(st, h->ev, 0));
    HIPCHK(h, hipMemsetAsync(d_counts, 0, 4 * sizeof(int), st));
    hipLaunchKernelGGL(mmpc_mission_round_kernel, dim3(B), dim3(MMPC_WAVE), 0, st, h->dp, B, d_x, d_tick, d_phase, d_U_last, d_glob, nglob,
                       d_obs0, d_vel, d_x_in, d_traj_ref, d_start, d_obs, d_lists, d_counts, d_hold, d_solve_phase, tick_limit);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(h->ev, st));
    h->ev_valid = 1; h->last_stream = st;
    return MMPC_OK;
}

__global__ __launch_bounds__(MMPC_WAVE) void mmpc_manipulate_round_kernel(
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

extern "C" int mmpc_manipulate_round_device(mmpc_handle h, int B, double *d_x, long long *d_tick, int *d_phase, const double *d_U_last,
                                            const double *d_pose, int nplan, double *d_plan, double *d_qgoal, int *d_ik_status,
                                            const double *d_obs0, const double *d_vel, double *d_x_in, double *d_traj_ref, int *d_start,
                                            double *d_obs, int *d_list, int *d_counts, int *d_hold, int *d_solve_phase,
                                            long long tick_limit, void *stream) {
    if (!h) return MMPC_E_ARG;
    if (h->cfg.kind != MMPC_KIND_WHOLEBODY || !h->hp.obs_per_stage)
        return fail(h, MMPC_E_UNSUPPORTED, "mmpc_manipulate_round_device: %s%s", "needs a whole-body handle (joint-space reference) created with obs_per_stage = 1 or 2");
    if (h->hp.obs_per_stage == 2 && d_obs)
        return fail(h, MMPC_E_ARG, "mmpc_manipulate_round_device: %s%s", "d_obs must be NULL on a motion handle (obs_per_stage = 2): the kernels form the centres from the record and the clock");
    if (B == 0) return MMPC_OK;
    if (const char *why = round_bad(h, B, d_x, d_tick, d_phase, d_U_last, d_obs0, d_vel, d_obs, d_hold, d_solve_phase, tick_limit))
        return fail(h, MMPC_E_ARG, "mmpc_manipulate_round_device: %s%s", why);
    if (!d_pose || !d_plan || !d_list || !d_counts)
        return fail(h, MMPC_E_ARG, "mmpc_manipulate_round_device: %s%s", "d_pose, d_plan, d_list and d_counts are required");
    if (nplan < 2 || nplan > (1 << 16)) return fail(h, MMPC_E_ARG, "mmpc_manipulate_round_device: %s%s", "nplan must be in 2..2^16");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipStream_t st = (hipStream_t)stream;
    if (h->ev_valid && st != h->last_stream) HIPCHK(h, hipStreamWaitEvent(st, h->ev, 0));
    HIPCHK(h, hipMemsetAsync(d_counts, 0, 2 * sizeof(int), st));
    hipLaunchKernelGGL(mmpc_manipulate_round_kernel, dim3(B), dim3(MMPC_WAVE), 0, st, h->dp, B, d_x, d_tick, d_phase, d_U_last, d_pose, nplan,
                       d_plan, d_qgoal, d_ik_status, d_obs0, d_vel, d_x_in, d_traj_ref, d_start, d_obs, d_list, d_counts, d_hold, d_solve_phase,
                       tick_limit);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(h->ev, st));
    h->ev_valid = 1; h->last_stream = st;
    return MMPC_OK;
}

__global__ __launch_bounds__(MMPC_WAVE) void mmpc_commit_kernel(
    int N, int B, int *__restrict__ hold, int *__restrict__ solve_phase, int set, int rejoin, const double *__restrict__ U,
    const int *__restrict__ status, const int *__restrict__ iters, const long long *__restrict__ tick, const int *__restrict__ phase,
    double *__restrict__ U_last, double *__restrict__ u0, int *__restrict__ iters_hist, int *__restrict__ status_hist,
    int *__restrict__ phase_hist, int T, int *__restrict__ counters) {
    const int b = (int)blockIdx.x;
    if (b >= B) return;
    mmpc_commit_robot(N, b, hold, solve_phase, set, rejoin, U, status, iters, tick, phase, U_last, u0, iters_hist, status_hist, phase_hist,
                      T, counters);
}

extern "C" int mmpc_mission_commit_device(mmpc_handle h, int B, int *d_hold, int *d_solve_phase, int set, int rejoin, const double *d_U,
                                          const int *d_status, const int *d_iters, const long long *d_tick, const int *d_phase,
                                          double *d_U_last, double *d_u0, int *d_iters_hist, int *d_status_hist, int *d_phase_hist, int T,
                                          int *d_counters, void *stream) {
    if (!h) return MMPC_E_ARG;
    if (h->cfg.kind != MMPC_KIND_WHOLEBODY)
        return fail(h, MMPC_E_UNSUPPORTED, "mmpc_mission_commit_device: %s%s", "needs a whole-body handle (joint-space reference)");
    if (B == 0) return MMPC_OK;
    if (B < 1 || B > h->cfg.max_batch) return fail(h, MMPC_E_ARG, "mmpc_mission_commit_device: %s%s", "B must be in 0..max_batch");
    if (!d_hold || !d_solve_phase || !d_U || !d_status || !d_iters || !d_tick || !d_phase || !d_U_last || !d_u0 || !d_iters_hist ||
        !d_status_hist || !d_phase_hist || !d_counters)
        return fail(h, MMPC_E_ARG, "mmpc_mission_commit_device: %s%s", "every array is required");
    if (d_U_last == d_U) return fail(h, MMPC_E_ARG, "mmpc_mission_commit_device: %s%s", "d_U_last must not be d_U");
    if (set < 0 || set > 15 || (rejoin != 0 && rejoin != 1) || T < 1)
        return fail(h, MMPC_E_ARG, "mmpc_mission_commit_device: %s%s", "set must be in 0..15, rejoin 0 or 1, T at least 1");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipStream_t st = (hipStream_t)stream;
    if (h->ev_valid && st != h->last_stream) HIPCHK(h, hipStreamWaitEvent(st, h->ev, 0));
    HIPCHK(h, hipMemsetAsync(d_counters, 0, 4 * sizeof(int), st));
    hipLaunchKernelGGL(mmpc_commit_kernel, dim3(B), dim3(MMPC_WAVE), 0, st, h->cfg.N, B, d_hold, d_solve_phase, set, rejoin, d_U, d_status,
                       d_iters, d_tick, d_phase, d_U_last, d_u0, d_iters_hist, d_status_hist, d_phase_hist, T, d_counters);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(h->ev, st));
    h->ev_valid = 1; h->last_stream = st;
    return MMPC_OK;
}

// the rejoin of a run with a resume budget (mmpc_set_resume_budget): a robot whose continuation was suspended again stays suspended
__global__ __launch_bounds__(MMPC_WAVE) void mmpc_rejoin_kernel(
    int N, int B, int *__restrict__ hold, int *__restrict__ solve_phase, int set, const double *__restrict__ U,
    const int *__restrict__ status, const int *__restrict__ iters, const long long *__restrict__ tick, const int *__restrict__ phase,
    double *__restrict__ U_last, double *__restrict__ u0, int *__restrict__ iters_hist, int *__restrict__ status_hist,
    int *__restrict__ phase_hist, int T, int *__restrict__ counters) {
    const int b = (int)blockIdx.x;
    if (b >= B) return;
    mmpc_rejoin_robot(N, b, hold, solve_phase, set, U, status, iters, tick, phase, U_last, u0, iters_hist, status_hist, phase_hist, T, counters);
}

extern "C" int mmpc_mission_rejoin_device(mmpc_handle h, int B, int *d_hold, int *d_solve_phase, int set, const double *d_U,
                                          const int *d_status, const int *d_iters, const long long *d_tick, const int *d_phase,
                                          double *d_U_last, double *d_u0, int *d_iters_hist, int *d_status_hist, int *d_phase_hist, int T,
                                          int *d_counters, void *stream) {
    if (!h) return MMPC_E_ARG;
    if (h->cfg.kind != MMPC_KIND_WHOLEBODY)
        return fail(h, MMPC_E_UNSUPPORTED, "mmpc_mission_rejoin_device: %s%s", "needs a whole-body handle (joint-space reference)");
    if (B == 0) return MMPC_OK;
    if (B < 1 || B > h->cfg.max_batch) return fail(h, MMPC_E_ARG, "mmpc_mission_rejoin_device: %s%s", "B must be in 0..max_batch");
    if (!d_hold || !d_solve_phase || !d_U || !d_status || !d_iters || !d_tick || !d_phase || !d_U_last || !d_u0 || !d_iters_hist ||
        !d_status_hist || !d_phase_hist || !d_counters)
        return fail(h, MMPC_E_ARG, "mmpc_mission_rejoin_device: %s%s", "every array is required");
    if (d_U_last == d_U) return fail(h, MMPC_E_ARG, "mmpc_mission_rejoin_device: %s%s", "d_U_last must not be d_U");
    if (set < 0 || set > 15 || T < 1)
        return fail(h, MMPC_E_ARG, "mmpc_mission_rejoin_device: %s%s", "set must be in 0..15, T at least 1");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipStream_t st = (hipStream_t)stream;
    if (h->ev_valid && st != h->last_stream) HIPCHK(h, hipStreamWaitEvent(st, h->ev, 0));
    HIPCHK(h, hipMemsetAsync(d_counters, 0, 4 * sizeof(int), st));
    hipLaunchKernelGGL(mmpc_rejoin_kernel, dim3(B), dim3(MMPC_WAVE), 0, st, h->cfg.N, B, d_hold, d_solve_phase, set, d_U, d_status,
                       d_iters, d_tick, d_phase, d_U_last, d_u0, d_iters_hist, d_status_hist, d_phase_hist, T, d_counters);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(h->ev, st));
    h->ev_valid = 1; h->last_stream = st;
    return MMPC_OK;
}
