// What a solve of a host lane-emulation build starts on (TEST ONLY - never part of the product): the LDS slab, the gain block, the
// scratch of the second-order correction, a save area and the per-lane register state, under the test's control.  Included by every
// harness under tests/ BEFORE the kernel headers (it defines MMPC_EMU_LANE_HOOK, which they expand behind their lane state).
//
// On the device a workgroup starts on whatever the previous one left in LDS, and under the persistent launch an instance starts on
// its predecessor's slab and registers: finite, plausible numbers.  A slab filled with NaN - the default here, and all the
// harnesses did before - shows a stale read that enters arithmetic, and is blind to one that is consumed by a comparison
// (`x > y ? x : y` of the max / min reductions, the guards of the line search and the filter): a NaN on one side is dropped there.
// So the fill is a mode, set per library with mmpc_emu_poison_set:
//   0 nan     every block filled with NaN for every instance (the default: a caller that never sets a mode sees no change)
//   1 keep    the blocks of the previous instance of this call, as it left them (the first instance of a call: NaN)
//   2 noise   seeded uniform values in +-1e3 (one stream per call of the setter, so a run is repeatable)
//   3 +1e300  4 -1e300  5 +inf  6 -inf  7 zero  8 1e-310 (a denormal)
// The blocks stay exact-size heap blocks, one malloc per instance (per call in mode keep), so a sanitized build sees any access
// outside them.  lane: -1 leaves the lane state alone (the default: it carries over from the previous solve of the thread),
// 0 ... 255 overwrites every byte of it with that value at the entry of every solve, continuations included.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum { MMPC_POISON_NAN = 0, MMPC_POISON_KEEP, MMPC_POISON_NOISE, MMPC_POISON_PBIG, MMPC_POISON_NBIG, MMPC_POISON_PINF, MMPC_POISON_NINF,
       MMPC_POISON_ZERO, MMPC_POISON_DENORMAL, MMPC_POISON_MODES };

static int mmpc_emu_poison_mode = MMPC_POISON_NAN, mmpc_emu_poison_lane = -1;
static uint64_t mmpc_emu_poison_rng = 0;

static inline double mmpc_emu_poison_noise() {   // splitmix64 -> uniform in [-1e3, 1e3)
    uint64_t z = (mmpc_emu_poison_rng += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    z ^= z >> 31;
    return ((double)(z >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0) * 1e3;
}

static inline void mmpc_emu_poison_fill_mode(double *p, size_t n, int mode) {
    for (size_t i = 0; i < n; i++)
        switch (mode) {
        case MMPC_POISON_NOISE: p[i] = mmpc_emu_poison_noise(); break;
        case MMPC_POISON_PBIG: p[i] = 1e300; break;
        case MMPC_POISON_NBIG: p[i] = -1e300; break;
        case MMPC_POISON_PINF: p[i] = INFINITY; break;
        case MMPC_POISON_NINF: p[i] = -INFINITY; break;
        case MMPC_POISON_ZERO: p[i] = 0.0; break;
        case MMPC_POISON_DENORMAL: p[i] = 1e-310; break;
        default: p[i] = NAN; break;   // (nan, and what keep starts a call on)
        }
}

extern "C" int mmpc_emu_poison_set(int mode, unsigned long long seed, int lane) {
    if (mode < 0 || mode >= MMPC_POISON_MODES || lane < -1 || lane > 255) return -1;
    mmpc_emu_poison_mode = mode; mmpc_emu_poison_rng = seed; mmpc_emu_poison_lane = lane;
    return 0;
}
// a block the caller owns (the save areas of a continuation chain live in the test's arrays) filled by the current mode
extern "C" void mmpc_emu_poison_fill(double *p, long long n) { mmpc_emu_poison_fill_mode(p, (size_t)(n > 0 ? n : 0), mmpc_emu_poison_mode); }

// One block of a harness call: next(n) is the block of the next instance - a fresh exact-size one filled by the mode, or in mode
// keep the previous instance's, untouched.  n = 0: no block (nullptr), as the harnesses had it for a gain block that is in LDS.
struct MmpcEmuBlock {
    double *p = nullptr;
    size_t n = 0;
    double *next(size_t n_) {
        if (mmpc_emu_poison_mode == MMPC_POISON_KEEP && p && n == n_) return p;
        free(p);
        n = n_;
        p = n ? (double *)malloc(sizeof(double) * n) : nullptr;
        mmpc_emu_poison_fill_mode(p, n, mmpc_emu_poison_mode);
        return p;
    }
    ~MmpcEmuBlock() { free(p); }
    MmpcEmuBlock() {}
    MmpcEmuBlock(const MmpcEmuBlock &) = delete;
    MmpcEmuBlock &operator=(const MmpcEmuBlock &) = delete;
};

// the kernels' lane state (static thread_local in the host builds: it outlives the solve) behind its declaration
static inline void mmpc_emu_lane_hook(void *p, size_t bytes) {
    if (mmpc_emu_poison_lane >= 0) memset(p, mmpc_emu_poison_lane, bytes);
}
#define MMPC_EMU_LANE_HOOK(ptr, bytes) mmpc_emu_lane_hook((void *)(ptr), (bytes));
