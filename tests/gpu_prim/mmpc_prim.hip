// mmpc_prim.hip - TEST ONLY (tests/prim_helper.py, tests/test_gpu_primitives.py).  Runs the device-only primitives of the
// kernels on the GPU, one at a time, so that each can be compared with an exact reference: the pieces that the host
// lane-emulation build (tests/emu/mmpc_emu.cpp) replaces by hand-written stand-ins and therefore never compiles.
// Every kernel here calls the product's functions and macros as they stand (mmpc_tile.h, mmpc_core.h, mmpc_fast.h); where a
// macro expects the solver's surroundings (ls_one, wr_one, lane) it gets a local of that name.
// One wavefront per block as in the product, straight-line code, no data-dependent loop; the launchers take host pointers
// and return the HIP error code (0 = success).
#include <hip/hip_runtime.h>
#include <utility>
#include "../../mobile-manipulator-mpc_amd/csrc/mmpc_fast.h"
#include "mmpc_prim_ops.h"

// ---- scalar functions: one thread per item
template <int OP>
__global__ void __launch_bounds__(MMPC_WAVE) mmpc_prim_map_kernel(int n, const double *in, double *out) {
    constexpr int NIN = mmpc_prim_nin(OP), NOUT = mmpc_prim_nout(OP);
    const int i = blockIdx.x * MMPC_WAVE + threadIdx.x;
    if (i >= n) return;
    double a[NIN], o[NOUT];
#pragma unroll
    for (int j = 0; j < NIN; j++) a[j] = in[(size_t)i * NIN + j];
#pragma unroll
    for (int j = 0; j < NOUT; j++) o[j] = 0.0;
    mmpc_prim_map_one(OP, a, o);
#pragma unroll
    for (int j = 0; j < NOUT; j++) out[(size_t)i * NOUT + j] = o[j];
}

// ---- cross-lane exchanges: one block per vector of 64 doubles, MMPC_PRIM_LANE_ROWS rows of 64 results
struct MmpcPrimLane { double v; };
template <int... J>
__device__ __forceinline__ void mmpc_prim_readlanes(const MmpcPrimLane &ls_one, double *o, int lane, std::integer_sequence<int, J...>) {
    ((o[MMPC_WAVE * (MMPC_PRIM_LANE_READLANE + J) + lane] = MMPC_LANE_GET(v, J)), ...);
}
template <int... J>
__device__ __forceinline__ void mmpc_prim_rowbcasts(double v, double *o, int lane, std::integer_sequence<int, J...>) {
    ((o[MMPC_WAVE * (MMPC_PRIM_LANE_ROWBCAST + J) + lane] = mmpc_rowbcast_f64<J>(v)), ...);
}
__global__ void __launch_bounds__(MMPC_WAVE) mmpc_prim_lanes_kernel(const double *in, double *out) {
    LANES_BEGIN
    MmpcPrimLane ls_one;
    ls_one.v = in[(size_t)blockIdx.x * MMPC_WAVE + lane];
    double *o = out + (size_t)blockIdx.x * MMPC_PRIM_LANE_ROWS * MMPC_WAVE;
    mmpc_prim_readlanes(ls_one, o, lane, std::make_integer_sequence<int, MMPC_WAVE>());
    mmpc_prim_rowbcasts(ls_one.v, o, lane, std::make_integer_sequence<int, 16>());
    double b9[9], b6[6];
    mmpc_rowbcast_all<0, 9>(ls_one.v, b9);
    mmpc_rowbcast_all<0, 6>(ls_one.v, b6);
#pragma unroll
    for (int j = 0; j < 9; j++) o[MMPC_WAVE * (MMPC_PRIM_LANE_RBALL9 + j) + lane] = b9[j];
#pragma unroll
    for (int j = 0; j < 6; j++) o[MMPC_WAVE * (MMPC_PRIM_LANE_RBALL6 + j) + lane] = b6[j];
    o[MMPC_WAVE * (MMPC_PRIM_LANE_DPP + 0) + lane] = mmpc_dpp_f64<0xB1>(ls_one.v);
    o[MMPC_WAVE * (MMPC_PRIM_LANE_DPP + 1) + lane] = mmpc_dpp_f64<0x4E>(ls_one.v);
    o[MMPC_WAVE * (MMPC_PRIM_LANE_DPP + 2) + lane] = mmpc_dpp_f64<0x141>(ls_one.v);
    o[MMPC_WAVE * (MMPC_PRIM_LANE_DPP + 3) + lane] = mmpc_dpp_f64<0x140>(ls_one.v);
    o[MMPC_WAVE * MMPC_PRIM_LANE_XOR16 + lane] = MMPC_LANE_XOR16(v);
    o[MMPC_WAVE * MMPC_PRIM_LANE_LOWER16 + lane] = MMPC_LANE_LOWER16(v);
    o[MMPC_WAVE * MMPC_PRIM_LANE_XOR32 + lane] = mmpc_xor32_f64(ls_one.v);
    LANES_END_REG
}

// ---- reductions: one block per vector, MMPC_PRIM_RED_ROWS rows of 64 results (every lane's)
__global__ void __launch_bounds__(MMPC_WAVE) mmpc_prim_red_kernel(const double *in, double *out) {
    __shared__ double RED[MMPC_WAVE];
    LANES_BEGIN
    RED[lane] = in[(size_t)blockIdx.x * MMPC_WAVE + lane];   // (as the generic kernel's phases leave their partials)
    LANES_END
    LANES_BEGIN
    const double wr_one[9] = {-7.0, -7.0, -7.0, in[(size_t)blockIdx.x * MMPC_WAVE + lane], -7.0, -7.0, -7.0, -7.0, -7.0};
    double *o = out + (size_t)blockIdx.x * MMPC_PRIM_RED_ROWS * MMPC_WAVE;
    o[0 * MMPC_WAVE + lane] = MMPC_RED_SUM(3);
    o[1 * MMPC_WAVE + lane] = MMPC_RED_MAX(3);
    o[2 * MMPC_WAVE + lane] = MMPC_RED_MIN(3);
    o[3 * MMPC_WAVE + lane] = MMPC_GRED_SUM(RED);
    o[4 * MMPC_WAVE + lane] = MMPC_GRED_MAX(RED);
    o[5 * MMPC_WAVE + lane] = MMPC_GRED_MIN(RED);
    o[6 * MMPC_WAVE + lane] = MMPC_GRED_MAXERR(RED);
    LANES_END_REG
}
// four at a time: in = a, b, c, d (4 rows of 64), out = the four sums then the four maxima (8 rows of 64)
__global__ void __launch_bounds__(MMPC_WAVE) mmpc_prim_red4_kernel(const double *in, double *out) {
    LANES_BEGIN
    const double *v = in + (size_t)blockIdx.x * 4 * MMPC_WAVE;
    const double wr_one[9] = {-7.0, v[lane], -7.0, -7.0, v[MMPC_WAVE + lane], -7.0, v[2 * MMPC_WAVE + lane], -7.0, v[3 * MMPC_WAVE + lane]};
    double s4[4], m4[4];
    MMPC_RED4_SUM(1, 4, 6, 8, s4);
    MMPC_RED4_MAX(1, 4, 6, 8, m4);
    double *o = out + (size_t)blockIdx.x * 8 * MMPC_WAVE;
#pragma unroll
    for (int j = 0; j < 4; j++) { o[j * MMPC_WAVE + lane] = s4[j]; o[(4 + j) * MMPC_WAVE + lane] = m4[j]; }
    LANES_END_REG
}

// ---- the matrix-core tile.  in = a, b, c[0..3] as the lanes hold them (6 rows of 64); out = MMPC_MFMA0(a, b) and
// MMPC_MFMA(c; a, b) as the lanes hold them (2 x 4 rows of 64)
struct MmpcPrimTile { MmpcAcc acc, s, d; double a, b; };
__global__ void __launch_bounds__(MMPC_WAVE) mmpc_prim_mfma_kernel(const double *in, double *out) {
    LANES_BEGIN
    const double *v = in + (size_t)blockIdx.x * 6 * MMPC_WAVE;
    double *o = out + (size_t)blockIdx.x * 8 * MMPC_WAVE;
    MmpcPrimTile ls_one;
    ls_one.a = v[lane]; ls_one.b = v[MMPC_WAVE + lane];
    MMPC_MFMA0(acc, ls.a, ls.b)
#pragma unroll
    for (int r = 0; r < 4; r++) o[r * MMPC_WAVE + lane] = ls_one.acc[r];
#pragma unroll
    for (int r = 0; r < 4; r++) ls_one.acc[r] = v[(2 + r) * MMPC_WAVE + lane];
    MMPC_MFMA(acc, ls.a, ls.b)
#pragma unroll
    for (int r = 0; r < 4; r++) o[(4 + r) * MMPC_WAVE + lane] = ls_one.acc[r];
    LANES_END_REG
}
// chained products without lane movement: in = the accumulator registers of S and of D (2 x 4 rows of 64); out = the
// accumulators of  sum_r MFMA(A = S[r], B = D[r])  and of  sum_r MFMA(A = D[r], B = S[r])
__global__ void __launch_bounds__(MMPC_WAVE) mmpc_prim_chain_kernel(const double *in, double *out) {
    LANES_BEGIN
    const double *v = in + (size_t)blockIdx.x * 8 * MMPC_WAVE;
    double *o = out + (size_t)blockIdx.x * 8 * MMPC_WAVE;
    MmpcPrimTile ls_one;
#pragma unroll
    for (int r = 0; r < 4; r++) { ls_one.s[r] = v[r * MMPC_WAVE + lane]; ls_one.d[r] = v[(4 + r) * MMPC_WAVE + lane]; }
    MMPC_MFMA0(acc, ls.s[0], ls.d[0])
    MMPC_MFMA(acc, ls.s[1], ls.d[1])
    MMPC_MFMA(acc, ls.s[2], ls.d[2])
    MMPC_MFMA(acc, ls.s[3], ls.d[3])
#pragma unroll
    for (int r = 0; r < 4; r++) o[r * MMPC_WAVE + lane] = ls_one.acc[r];
    MMPC_MFMA0(acc, ls.d[0], ls.s[0])
    MMPC_MFMA(acc, ls.d[1], ls.s[1])
    MMPC_MFMA(acc, ls.d[2], ls.s[2])
    MMPC_MFMA(acc, ls.d[3], ls.s[3])
#pragma unroll
    for (int r = 0; r < 4; r++) o[(4 + r) * MMPC_WAVE + lane] = ls_one.acc[r];
    LANES_END_REG
}

// ---- launchers
namespace {
// copies in, launches `launch(d_in, d_out)`, copies out; frees on every path
template <class L>
int mmpc_prim_run(const double *in, size_t n_in, double *out, size_t n_out, L launch) {
    double *d_in = nullptr, *d_out = nullptr;
    hipError_t e = hipMalloc(&d_in, n_in * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&d_out, n_out * sizeof(double));
    if (e == hipSuccess) e = hipMemcpy(d_in, in, n_in * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(d_out, 0, n_out * sizeof(double));
    if (e == hipSuccess) { launch(d_in, d_out); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, d_out, n_out * sizeof(double), hipMemcpyDeviceToHost);
    if (d_in) (void)hipFree(d_in);
    if (d_out) (void)hipFree(d_out);
    return (int)e;
}
}

extern "C" int mmpc_prim_op_shape(int op, int *nin, int *nout) {
    *nin = mmpc_prim_nin(op); *nout = mmpc_prim_nout(op);
    return *nin > 0 ? 0 : -1;
}
// n items: in [n][nin], out [n][nout]
extern "C" int mmpc_prim_map(int op, int n, const double *in, double *out) {
    if (n <= 0 || mmpc_prim_nin(op) <= 0) return -1;
    const unsigned grid = (unsigned)((n + MMPC_WAVE - 1) / MMPC_WAVE);
    return mmpc_prim_run(in, (size_t)n * mmpc_prim_nin(op), out, (size_t)n * mmpc_prim_nout(op), [&](const double *di, double *dout) {
        switch (op) {
#define X(name, id, nin, nout) case id: mmpc_prim_map_kernel<id><<<grid, MMPC_WAVE>>>(n, di, dout); break;
            MMPC_PRIM_OPS(X)
#undef X
        }
    });
}
// nvec vectors: in [nvec][64], out [nvec][MMPC_PRIM_LANE_ROWS][64]
extern "C" int mmpc_prim_lanes(int nvec, const double *in, double *out) {
    if (nvec <= 0) return -1;
    return mmpc_prim_run(in, (size_t)nvec * MMPC_WAVE, out, (size_t)nvec * MMPC_PRIM_LANE_ROWS * MMPC_WAVE,
                         [&](const double *di, double *dout) { mmpc_prim_lanes_kernel<<<(unsigned)nvec, MMPC_WAVE>>>(di, dout); });
}
// in [nvec][64], out [nvec][MMPC_PRIM_RED_ROWS][64]
extern "C" int mmpc_prim_red(int nvec, const double *in, double *out) {
    if (nvec <= 0) return -1;
    return mmpc_prim_run(in, (size_t)nvec * MMPC_WAVE, out, (size_t)nvec * MMPC_PRIM_RED_ROWS * MMPC_WAVE,
                         [&](const double *di, double *dout) { mmpc_prim_red_kernel<<<(unsigned)nvec, MMPC_WAVE>>>(di, dout); });
}
// in [nvec][4][64], out [nvec][8][64]
extern "C" int mmpc_prim_red4(int nvec, const double *in, double *out) {
    if (nvec <= 0) return -1;
    return mmpc_prim_run(in, (size_t)nvec * 4 * MMPC_WAVE, out, (size_t)nvec * 8 * MMPC_WAVE,
                         [&](const double *di, double *dout) { mmpc_prim_red4_kernel<<<(unsigned)nvec, MMPC_WAVE>>>(di, dout); });
}
// in [nvec][6][64], out [nvec][8][64]
extern "C" int mmpc_prim_mfma(int nvec, const double *in, double *out) {
    if (nvec <= 0) return -1;
    return mmpc_prim_run(in, (size_t)nvec * 6 * MMPC_WAVE, out, (size_t)nvec * 8 * MMPC_WAVE,
                         [&](const double *di, double *dout) { mmpc_prim_mfma_kernel<<<(unsigned)nvec, MMPC_WAVE>>>(di, dout); });
}
// in [nvec][8][64], out [nvec][8][64]
extern "C" int mmpc_prim_chain(int nvec, const double *in, double *out) {
    if (nvec <= 0) return -1;
    return mmpc_prim_run(in, (size_t)nvec * 8 * MMPC_WAVE, out, (size_t)nvec * 8 * MMPC_WAVE,
                         [&](const double *di, double *dout) { mmpc_prim_chain_kernel<<<(unsigned)nvec, MMPC_WAVE>>>(di, dout); });
}
// the A/B switches this library was built with (the tests check that they asked for the right one)
extern "C" int mmpc_prim_switches() { return (MMPC_RCP_NEWTON ? 1 : 0) | (MMPC_PIV_NEWTON ? 2 : 0); }
