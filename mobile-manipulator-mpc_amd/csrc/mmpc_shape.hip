// mmpc_shape.hip - a shape library: the six specialised kernels ([one launch, budgeted / continuation] x obs_per_stage 0, 1, 2)
// of ONE (kind, N, M), libmmpc_shape_<kind>_<N>_<M>.so.  Built on demand by build.py:build_shape_library with
// -DMMPC_SHAPE_KIND= -DMMPC_SHAPE_N= -DMMPC_SHAPE_M= and the flags and source tag of libmmpc.so; loaded by
// mmpc_load_shape_library, after which mmpc_create picks the shape up as it picks up a shape of MMPC_FAST_LIST.
#include <hip/hip_runtime.h>
#include <math.h>
#include "mmpc_fast_kernel.h"

#if !defined(MMPC_SHAPE_KIND) || !defined(MMPC_SHAPE_N) || !defined(MMPC_SHAPE_M)
#error "mmpc_shape.hip: build with -DMMPC_SHAPE_KIND= -DMMPC_SHAPE_N= -DMMPC_SHAPE_M= (build.py:build_shape_library)"
#endif
// waves per SIMD the register allocation is sized for: 1 for the whole-body kind, 2 for the base kind, as MMPC_FAST_LIST has it
#define MMPC_SHAPE_WPE (MMPC_SHAPE_KIND == 1 ? 2 : 1)

extern "C" __attribute__((visibility("default"))) void mmpc_shape_describe(MmpcShapeDesc *d, unsigned long long bytes) {
    mmpc_shape_fill<MMPC_SHAPE_KIND, MMPC_SHAPE_N, MMPC_SHAPE_M, MMPC_SHAPE_WPE>(d, bytes);
}
