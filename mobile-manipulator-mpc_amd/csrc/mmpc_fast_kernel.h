// mmpc_fast_kernel.h - the launchable form of the specialised solver: the kernel wrapper around mmpc_solve_fast, the type of a
// pointer to it, and the descriptor through which a shape library (mmpc_shape.hip: the six kernels of one (kind, N, M), built on
// demand) hands its kernels to libmmpc.so (mmpc_load_shape_library in mmpc_hip.hip).  Both translation units include this file,
// so a listed shape and a loaded one run the same text.
#pragma once
#include "mmpc_fast.h"

// Diagnostic build only (-DMMPC_STAMP_INST, tools/persistent_launch_probe.py --stamps): per instance row the start and the end of its
// solve on the 100 MHz clock all XCDs share and on the wave's cycle counter, the XCD and the workgroup that solved it.  The shipped
// kernels contain no stamps.
#ifdef MMPC_STAMP_INST
#define MMPC_INST_STAMP_ROWS 8192
__device__ unsigned long long mmpc_inst_stamp[6 * MMPC_INST_STAMP_ROWS];
#define MMPC_INST_T0() const unsigned long long ir0_ = __builtin_amdgcn_s_memrealtime(), ic0_ = __builtin_readcyclecounter();
#define MMPC_INST_T1(b)                                                                                                        \
    if (threadIdx.x == 0 && (b) < MMPC_INST_STAMP_ROWS) {                                                                      \
        unsigned long long *q_ = mmpc_inst_stamp + 6 * (b);                                                                    \
        q_[0] = ir0_; q_[1] = __builtin_amdgcn_s_memrealtime(); q_[2] = ic0_; q_[3] = __builtin_readcyclecounter();             \
        q_[4] = __builtin_amdgcn_s_getreg(20 | (3 << 11)); q_[5] = blockIdx.x;   /* (HW_REG_XCC_ID, bits 3:0) */                 \
    }
#else
#define MMPC_INST_T0()
#define MMPC_INST_T1(b)
#endif

// OPS = the config's obs_per_stage (0 static record, 1 table per stage, 2 motion record + clock): part of the LDS layout.  The LDS block is STATIC (its size is a
// constant of the instantiation): with `extern __shared__` the base of the dynamic block is resolved after instruction
// selection and every lane-derived LDS address carries an add of that constant 0 (14 of the ~200 instructions of a Riccati stage).
template <int KIND, int N, int MC, int WPE, bool CONT, int OPS>
__global__ __launch_bounds__(MMPC_WAVE, WPE) void mmpc_fast_kernel(
    const MmpcParams *__restrict__ Pp, int B, const double *__restrict__ x_init, const double *__restrict__ traj_ref,
    const double *__restrict__ u_ref, const double *__restrict__ u_last, const double *__restrict__ x_guess,
    const double *__restrict__ obs, double *__restrict__ X, double *__restrict__ U, double *__restrict__ s,
    int *__restrict__ status, int *__restrict__ iters, double *__restrict__ cost, double *__restrict__ err,
    const int *__restrict__ order, int budget, double *__restrict__ state, int state_stride, const int *__restrict__ resume_count,
    const int *__restrict__ list_count, double *__restrict__ gscr, double *__restrict__ soc, int soc_stride,
    const long long *__restrict__ tick, double scale_max_grad, double *__restrict__ scale_out, int *__restrict__ ticket) {
    __shared__ double lds[mmpc_fast_layout<KIND, N>(MC, OPS).total];
    // A continuation launch (resume_count != null): `order` is the compacted list of the suspended instances, *resume_count its
    // length, and the grid is SMALL (MMPC_RESUME_GRID workgroups that stride over the list): a handful of instances is left,
    // and a grid of B workgroups that almost all exit at once would still have to be dispatched one by one - in a stream of
    // batches that competes with the next batch's launch.
    // A list launch (list_count != null, mmpc_solve_list_device): `order` is the caller's list of instances, *list_count its length
    // (read on the device: the caller need not know it), the grid is the list's capacity.
    const int limit = resume_count ? *resume_count : (list_count ? *list_count : B);
    // A persistent launch (ticket != null; the plain launch of the kernels without the continuation code, mmpc_set_persistent_grid): the
    // grid is what the chip holds at once, and a workgroup that has finished an instance draws the next launch position from *ticket
    // - a greedy queue in launch order, without the dispatch of a new workgroup (its LDS allocation, its wave launch) at every
    // turnover of a slot.  *ticket is 0 when the kernel starts and 0 again when it ends: the tickets drawn are 0 .. B + grid - 1,
    // each once, every workgroup draws exactly one that is >= B, and the one that draws the last has seen every other draw - it
    // puts the counter back, so no launch needs a memset or another kernel before it.
    const bool pers = !CONT && ticket != nullptr;
    auto take = [&]() -> int {
        int t = 0;
        if (threadIdx.x == 0) t = atomicAdd(ticket, 1);
        return __builtin_amdgcn_readfirstlane(t);
    };
    int w = pers ? take() : (int)blockIdx.x;
    for (; w < limit; w = pers ? take() : w + (int)gridDim.x) {
        // launch order: position w solves instance order[w] (a permutation / a list; results do not depend on it)
        const int b = order ? order[w] : w;
        // (a list launch takes its row indices from the caller's device memory, where nothing can have checked them: an index
        //  outside the batch is skipped - it would address the inputs, the outputs and the handle's own save areas)
        if ((unsigned)b >= (unsigned)B) { if (!pers && (!CONT || !resume_count)) break; continue; }
        const MmpcParams &P = *Pp;
        const int M = MC;
        const size_t so = OPS == 2 ? (size_t)M * 5 : (size_t)(P.obs_per_stage ? N + 1 : 1) * M * 3;
        MmpcIO io;
        mmpc_instance_io<KIND>(io, P, b, N, so, x_init, traj_ref, u_ref, u_last, x_guess, obs, X, U, s, status, iters, cost, err,
                               soc, soc_stride);
        io.state = state ? state + (size_t)b * state_stride : nullptr;
        io.budget = budget;
        io.resume = resume_count ? 1 : 0;
        io.gscr = MmpcGainBlock<KIND, N>::ON ? gscr + (size_t)b * MmpcGainBlock<KIND, N>::total : nullptr;
        if (OPS == 2 && tick) io.tick = tick + b;   // the clock is indexed by instance row, like every per-instance array
        io.scale_max_grad = scale_max_grad; if (scale_out) io.scale_out = scale_out + b;   // (objective scaling; by instance row too)
        MMPC_INST_T0()
        mmpc_solve_fast<KIND, N, MC, CONT, OPS>(P, io, lds);
        MMPC_INST_T1(b)
        if (!pers && (!CONT || !resume_count)) break;      // (one instance per workgroup except in a continuation or a persistent launch)
        __builtin_amdgcn_s_barrier();           // the next instance reuses the LDS block
    }
    if (pers && w == limit + (int)gridDim.x - 1 && threadIdx.x == 0) atomicExch(ticket, 0);
}

// the signature of mmpc_fast_kernel<>
typedef void (*mmpc_fast_fn)(const MmpcParams *, int, const double *, const double *, const double *, const double *, const double *,
                             const double *, double *, double *, double *, int *, int *, double *, double *, const int *, int, double *,
                             int, const int *, const int *, double *, double *, int, const long long *, double, double *, int *);

// Contents of the kernel sources as build.py hashes them (-DMMPC_SOURCE_TAG=0x...ULL, the same value for libmmpc.so and for every
// shape library): MmpcParams and the kernel argument list are no stable ABI, so a library from other sources is refused.
#ifndef MMPC_SOURCE_TAG
#define MMPC_SOURCE_TAG 0ULL   // (a build by hand, without build.py: matches only another such build)
#endif
#define MMPC_SHAPE_MAGIC 0x4d4d504353484150ULL   // "MMPCSHAP"
// The one C function a shape library exports: void (MmpcShapeDesc *d, unsigned long long bytes), `bytes` being the room behind d.
// The head of the descriptor - magic, source tag, the descriptor's own size - is the only part of it that never changes: with
// bytes >= sizeof(MmpcShapeHead) the head is written, the rest only when bytes >= sizeof(MmpcShapeDesc) of the LIBRARY's build.  The
// loader asks for the head first and for the whole descriptor once magic, tag and size are its own, so that a library from other
// sources - whose descriptor may be larger - writes nothing behind the loader's struct before it is refused.
#define MMPC_SHAPE_ENTRY "mmpc_shape_describe"
struct MmpcShapeHead {
    unsigned long long magic, source_tag, desc_bytes;
};
struct MmpcShapeDesc {
    MmpcShapeHead head;
    int kind, N, M, wpe;
    mmpc_fast_fn fn[3][2];          // [obs_per_stage][CONT]
    int state_doubles, gscr_doubles;   // mmpc_fast_state_doubles, MmpcGainBlock::total
    int lds_bytes[3];               // the fast layout's bytes per obs_per_stage
};
// the descriptor of mmpc_fast_kernel<K, NN, MM, WW, ., .>
template <int K, int NN, int MM, int WW>
inline void mmpc_shape_fill(MmpcShapeDesc *d, unsigned long long bytes) {
    static_assert(mmpc_fast_shape_ok(K, NN, MM), "(kind, N, M) is outside the specialised template's envelope (MmpcFastEnvelope)");
    if (!d || bytes < sizeof(MmpcShapeHead)) return;
    d->head.magic = MMPC_SHAPE_MAGIC; d->head.source_tag = MMPC_SOURCE_TAG; d->head.desc_bytes = sizeof(MmpcShapeDesc);
    if (bytes < sizeof(MmpcShapeDesc)) return;
    d->kind = K; d->N = NN; d->M = MM; d->wpe = WW;
    d->fn[0][0] = mmpc_fast_kernel<K, NN, MM, WW, false, 0>; d->fn[0][1] = mmpc_fast_kernel<K, NN, MM, WW, true, 0>;
    d->fn[1][0] = mmpc_fast_kernel<K, NN, MM, WW, false, 1>; d->fn[1][1] = mmpc_fast_kernel<K, NN, MM, WW, true, 1>;
    d->fn[2][0] = mmpc_fast_kernel<K, NN, MM, WW, false, 2>; d->fn[2][1] = mmpc_fast_kernel<K, NN, MM, WW, true, 2>;
    d->state_doubles = mmpc_fast_state_doubles<K, NN>(MM);
    d->gscr_doubles = MmpcGainBlock<K, NN>::total;
    for (int o = 0; o < 3; o++) d->lds_bytes[o] = mmpc_fast_layout<K, NN>(MM, o).total * (int)sizeof(double);
}
