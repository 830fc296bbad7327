"""What the kernels' instructions compute: the device-only primitives of mmpc_tile.h / mmpc_core.h / mmpc_fast.h, one per
launch on the GPU (tests/gpu_prim/mmpc_prim.hip calls the product's functions and macros as they stand), against exact
references - and against the stand-ins that replace them in the host lane-emulation build, on whose faithfulness the whole
CPU suite rests.  Needs neither torch nor libmmpc.so.

References are independent of both builds: fractions.Fraction for everything algebraic (a double is a rational, so
|r x - 1| and |y^2 x - 1| are exact), exact rational sums for reductions, numpy indexing for permutations, mpmath at 200 bits
for log / sin / cos (tests/test_primitives_cpu.py holds the checks both modules share).  Every bound is derived, none is
taken from what the code returns; the measured worst values are printed (pytest -s) and quoted in the comments of
mmpc_tile.h / mmpc_core.h.

Edge values, where the device and the emulation differ in class (table EDGE_DEVICE / EDGE_HOST of test_primitives_cpu.py),
and why no call site sees the difference:
  * mmpc_rcp / mmpc_rcp3 / mmpc_rcp_piv at +-0, +-inf, a subnormal: NaN on the device, +-inf / +-0 in the emulation.  Call sites:
    box slacks pass through mmpc_box_t first (>= 1e-15); row slacks are kept positive by the fraction-to-boundary rule and
    start at >= 1e-2; mmpc_log_mant divides by m + 1 in [1.7, 2.42]; the pivots of the legs are tested with `!(p > 0)`
    BEFORE their reciprocal is used, which catches 0, a negative value and NaN alike, and an inf pivot means an inf entry
    that turns the next update into NaN.  Either class (NaN, or inf times a finite number) ends in a non-finite evaluation,
    which both builds report as status 2.
  * mmpc_rsqrt(0) - a robot standing on an obstacle's centre: NaN on the device, +inf in the emulation, where the distance
    d = m2 * id = 0 * inf is NaN one line later: the row and the sum over the rows are NaN in both builds.
  * mmpc_sqrt_pair(0) - the end point on one of the four self-collision points: (NaN, NaN) on the device, (0, -inf) in the
    emulation: h = 0.05 there is the true value, the gradient (0 * -inf = NaN or +-inf) is not finite in either build.
  No edge input gives a finite non-zero wrong value in either build."""
from fractions import Fraction

import numpy as np
import pytest

import prim_helper as P
import test_primitives_cpu as cpu

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SEED = cpu.SEED + 100

# ---- bounds on the relative error (exact rational arithmetic), and where each comes from
B_RCP = U * (1 + 2.0 ** -7)          # 1.12e-16: one rounding of the final fma; the cubic step leaves e^3 <= 2^-60 for a seed good to 2^-20
B_RSQRT = 1.5 * U * (1 + 2.0 ** -7)  # 1.68e-16: the final fma's rounding + half of the 2^-53 the rounded product x y puts into e
B_PIV = 2.0 ** -48 + U               # 3.7e-15: e^2 of a seed good to 2^-24 (what mmpc_tile.h states) + one rounding: pins the seed
B_SQRT_N = 2                         # ulp of the result


@pytest.fixture(scope="module")
def dev():
    return P.device()


@pytest.fixture(scope="module")
def hst():
    return P.host()


def recip_inputs(rng, lo=1e-30, hi=1e30, named=()):
    """2^16 values log-uniform over [lo, hi] with the end points, 2^12 mantissa edges (1 + j 2^-52) 2^e and (2 - j 2^-52) 2^e with e
    over the same range, and the named cases.
    Reachable domains, from the call sites: mmpc_rcp - box slacks mmpc_box_t(d) in [1e-15, 2 x 9.9e18], row slacks (no floor)
    and m + 1 in [1.7, 2.42] (mmpc_log_mant); mmpc_rcp3 / mmpc_rcp_piv - the pivots of the elimination legs (positive, tested
    before use; DESIGN section 7 reports magnitudes to 1e10 under barrier weights); mmpc_rsqrt - squared distances to obstacle
    centres; mmpc_sqrt_pair - squared distances between arm points.  Where the code gives no tighter bound: [1e-30, 1e30]."""
    x = 10.0 ** rng.uniform(np.log10(lo), np.log10(hi), 1 << 16)
    j = np.arange(1024)
    e = rng.integers(int(np.ceil(np.log2(lo))), int(np.floor(np.log2(hi))) - 1, 1024).astype(float)
    edges = np.concatenate([(1 + j * 2.0 ** -52) * 2.0 ** e, (2 - j * 2.0 ** -52) * 2.0 ** e,
                            (1 + j * 2.0 ** -52), (2 - j * 2.0 ** -52)])
    return np.concatenate([x, [lo, hi, 1e-15, 2 * 9.9e18, 1.7, 2.42], edges, np.asarray(named, float)])


def worst_rcp_err(x, r):
    """max |r x - 1| exactly, and the x attaining it"""
    worst, at = Fraction(0), None
    for xi, ri in zip(x, r):
        e = abs(Fraction(float(ri)) * Fraction(float(xi)) - 1)
        if e > worst:
            worst, at = e, float(xi)
    return worst, at


def worst_rsqrt_err(x, y):
    """max relative error d of y against 1 / sqrt(x), exactly: (1 + d)^2 = y^2 x.  Returns the worst |y^2 x - 1| (= 2 d + d^2)"""
    worst, at = Fraction(0), None
    for xi, yi in zip(x, y):
        Y = Fraction(float(yi))
        e = abs(Y * Y * Fraction(float(xi)) - 1)
        if e > worst:
            worst, at = e, float(xi)
    return worst, at


def sq_bound(b):
    """|y^2 x - 1| that a relative error b of y allows"""
    b = Fraction(b)
    return 2 * b + b * b


# ------------------------------------------------------------------------------------------------- a. reciprocals and roots
# the inputs that attained the worst errors on the MI355X stay in the sample by name (shipped build, MMPC_PIV_NEWTON=0, MMPC_RCP_NEWTON=1,
# mmpc_rcp_piv; mmpc_rsqrt, inv of mmpc_sqrt_pair, n of mmpc_sqrt_pair)
NAMED_RCP = [1.009741958682895e-28, 2251799813685247.8, 15.998394031246612, 17587082115124.412]
NAMED_RSQRT = [1.242934199509302e-26, 5.7891661980951546e-11, 2.1175823681357513e-22]


@pytest.mark.parametrize("name", ["rcp", "rcp3"])
def test_rcp(dev, name):
    x = recip_inputs(np.random.default_rng(SEED), named=NAMED_RCP)
    worst, at = worst_rcp_err(x, dev.map(name, x))
    print("mmpc_%s: worst relative error %.4e at x = %r (bound %.4e)" % (name, float(worst), at, B_RCP))
    assert worst <= Fraction(B_RCP), (float(worst), at)


def test_rcp_piv(dev):
    x = recip_inputs(np.random.default_rng(SEED + 1), named=NAMED_RCP)
    worst, at = worst_rcp_err(x, dev.map("rcp_piv", x))
    print("mmpc_rcp_piv: worst relative error %.4e = 2^%.2f at x = %r (bound %.4e)" % (float(worst), np.log2(float(worst)), at, B_PIV))
    assert worst <= Fraction(B_PIV), (float(worst), at)


def test_rsqrt(dev):
    x = recip_inputs(np.random.default_rng(SEED + 2), named=NAMED_RSQRT)
    worst, at = worst_rsqrt_err(x, dev.map("rsqrt", x))
    print("mmpc_rsqrt: worst relative error %.4e at x = %r (bound %.4e)" % (float(worst) / 2, at, B_RSQRT))
    assert worst <= sq_bound(B_RSQRT), (float(worst) / 2, at)


def test_sqrt_pair(dev):
    """inv = -1 / (2 sqrt(m)) to the mmpc_rsqrt bound; n = sqrt(m) to 2 ulp: (n - 2 u)^2 <= m <= (n + 2 u)^2, u the spacing at n"""
    x = recip_inputs(np.random.default_rng(SEED + 3), named=NAMED_RSQRT)
    got = dev.map("sqrt_pair", x)
    worst, at = worst_rsqrt_err(x, -2 * got[:, 1])
    print("mmpc_sqrt_pair inv: worst relative error %.4e at m = %r (bound %.4e)" % (float(worst) / 2, at, B_RSQRT))
    assert worst <= sq_bound(B_RSQRT), (float(worst) / 2, at)
    wn, atn = 0.0, None
    for m, n in zip(x, got[:, 0]):
        Nf, M, u = Fraction(float(n)), Fraction(float(m)), Fraction(float(np.spacing(n)))
        assert (Nf - B_SQRT_N * u) ** 2 <= M <= (Nf + B_SQRT_N * u) ** 2, (m, n)
        e = abs(float((Nf * Nf - M) / (2 * Nf) / u))     # |n - sqrt(m)| / u to first order
        if e > wn:
            wn, atn = e, float(m)
    print("mmpc_sqrt_pair n: worst error %.3f ulp at m = %r (bound %d ulp)" % (wn, atn, B_SQRT_N))


def test_rcp_one_newton_step_is_resolved():
    """-DMMPC_RCP_NEWTON=1 takes one refinement step out of mmpc_rcp: its worst error must lie ABOVE the bound of the shipped
    function and below the Newton bound - standing proof that the test resolves one lost step"""
    d = P.device(("MMPC_RCP_NEWTON=1",))
    assert d.switches() == 3
    x = recip_inputs(np.random.default_rng(SEED), named=NAMED_RCP)
    worst, at = worst_rcp_err(x, d.map("rcp", x))
    print("mmpc_rcp with MMPC_RCP_NEWTON=1: worst relative error %.4e at x = %r (must lie in (%.4e, %.4e))" % (float(worst), at, B_RCP, B_PIV))
    assert Fraction(B_RCP) < worst < Fraction(B_PIV), (float(worst), at)


def test_rcp_piv_cubic_step_meets_the_rcp_bound():
    d = P.device(("MMPC_PIV_NEWTON=0",))
    assert d.switches() == 0
    x = recip_inputs(np.random.default_rng(SEED + 1), named=NAMED_RCP)
    worst, at = worst_rcp_err(x, d.map("rcp_piv", x))
    print("mmpc_rcp_piv with MMPC_PIV_NEWTON=0: worst relative error %.4e at x = %r (bound %.4e)" % (float(worst), at, B_RCP))
    assert worst <= Fraction(B_RCP), (float(worst), at)


def test_edge_values(dev, hst):
    """the committed class tables, on the device and in the emulation (see the module docstring for the call sites)"""
    print("device:")
    cpu.check_edges(dev, cpu.EDGE_DEVICE)
    print("emulation:")
    cpu.check_edges(hst, cpu.EDGE_HOST)


def test_vmax_vmin(dev):
    """mmpc_vmax / mmpc_vmin (v_max_f64 / v_min_f64) equal numpy.fmax / fmin bit for bit on 2^16 pairs, NaN on either side and
    +-inf among them (two NaNs give a NaN; a (+0, -0) pair is left out: IEEE leaves it open)"""
    rng = np.random.default_rng(SEED + 4)
    n = 1 << 16
    a = rng.standard_normal(n) * 10.0 ** rng.uniform(-300, 300, n); b = rng.standard_normal(n) * 10.0 ** rng.uniform(-300, 300, n)
    b[::5] = a[::5]
    for arr, off in ((a, 0), (b, 1)):
        arr[off + 2:4096:8] = np.nan; arr[off + 4:4096:16] = np.inf; arr[off + 12:4096:16] = -np.inf
    a[4096:4100] = [0.0, -0.0, np.nan, np.nan]; b[4096:4100] = [1.0, -1.0, 0.0, -0.0]
    a[5000:5200] = np.nan; b[5000:5200] = np.nan
    for name, ref in (("vmax", np.fmax), ("vmin", np.fmin)):
        got, want = dev.map(name, a, b), ref(a, b)
        both = np.isnan(a) & np.isnan(b)
        assert np.isnan(got[both]).all() and both.sum() > 100
        assert (got[~both].view(np.uint64) == want[~both].view(np.uint64)).all()
        assert (np.isnan(a) ^ np.isnan(b)).sum() > 500


def test_zsafe(dev, hst):
    """mmpc_z_safeguard_fast on the device against mmpc_z_safeguard on the host, and both device functions against the exact clamp"""
    cpu.check_zsafe(dev)
    z, t, mu = cpu.zsafe_inputs(np.random.default_rng(cpu.SEED + 10))
    f, s = dev.map("zsafe_fast", z, t, mu), hst.map("zsafe", z, t, mu)
    assert (np.abs(f - s) <= 4 * np.spacing(np.abs(s))).all()


def test_powf(dev):
    cpu.check_powf(dev)


def test_mul24(dev):
    cpu.check_mul24(dev)


# ------------------------------------------------------------------------------------------------- b. cross-lane exchanges
def test_lane_exchanges(dev):
    """every exchange, every lane, bit-exact: mmpc_readlane_f64 (j = 0..63), mmpc_rowbcast_f64<0..15>, mmpc_rowbcast_all<0, 9> and
    <0, 6>, mmpc_dpp_f64<0xB1 | 0x4E | 0x141 | 0x140>, mmpc_xor16_f64, mmpc_lower16_f64, mmpc_xor32_f64.  (The host stand-ins
    MMPC_LANE_GET / _XOR16 / _LOWER16 are held to the same expectation by tests/test_primitives_cpu.py.)"""
    cpu.check_lanes(dev, range(P.LANE_ROWS))


# ------------------------------------------------------------------------------------------------- c. reductions
def test_reductions(dev, hst):
    """all lanes the same bits; the bits of the host stand-in (mmpc_emu_red, mmpc_emu_red_arr) on every vector without a NaN -
    the sentence the CPU suite rests on; and, independently of both, exact maxima / minima and the pairwise bound of the sums"""
    d, h = cpu.check_reductions(dev), cpu.check_reductions(hst)
    for fam in d:
        assert (d[fam].view(np.uint64) == h[fam].view(np.uint64)).all(), fam


def test_red4(dev, hst):
    d, h = cpu.check_red4(dev), cpu.check_red4(hst)
    assert (d.view(np.uint64) == h.view(np.uint64)).all()


def test_reductions_nan(dev, hst):
    """A NaN in lane p, each p.  MAXERR returns NaN in every lane on both builds; the sums return NaN.  mmpc_wave_max / _min on
    the device return the maximum / minimum of the other 63 lanes in every lane (v_max_f64 drops a NaN), which the ternary of
    the host stand-in does NOT do for every p (test_primitives_cpu.py::test_reduction_nan_host_standin).  The source knows that
    ("NaNs are caught by the sums of the evaluation"): the catch it relies on is that the sum over the same vector is NaN."""
    rng = np.random.default_rng(cpu.SEED + 14)
    V = rng.standard_normal((64, 64))
    V[np.arange(64), np.arange(64)] = np.nan
    D, H = dev.red(V), hst.red(V)
    assert np.isnan(D[:, [0, 3, 6]]).all() and np.isnan(H[:, [0, 3, 6]]).all()
    assert (D[:, 1] == np.nanmax(V, axis=1)[:, None]).all()
    assert (D[:, 2] == np.nanmin(V, axis=1)[:, None]).all()
    R4 = dev.red4(np.stack([V, V[::-1], 2 * V, 3 * V], axis=1))
    assert np.isnan(R4[:, :4]).all()
    assert (R4[:, 4] == np.nanmax(V, axis=1)[:, None]).all() and (R4[:, 6] == 2 * np.nanmax(V, axis=1)[:, None]).all()


# ------------------------------------------------------------------------------------------------- d. the matrix-core tile
# Whether v_mfma_f64_16x16x4_f64 rounds like the host macro (an fma chain in ascending k) - found out by this test on the device
MFMA_BITWISE_LIKE_FMA_CHAIN = True


def test_mfma_tile(dev, hst):
    """the lane <-> element map (integer operands, each element of A and B alone: exact), the error bound on real entries, the
    chaining claim, and whether the device result on real entries is bitwise that of the host macro"""
    cpu.check_mfma_exact(dev)
    cpu.check_mfma_chain(dev)
    d, h = cpu.check_mfma_real(dev), cpu.check_mfma_real(hst)
    same = d.view(np.uint64) == h.view(np.uint64)
    print("MMPC_MFMA on real entries: %d of %d device results are bitwise those of the host macro (fma chain in ascending k)" % (same.sum(), same.size))
    assert same.all() == MFMA_BITWISE_LIKE_FMA_CHAIN


# ------------------------------------------------------------------------------------------------- e. shared-source functions
# (hipcc contracts a * b + c * d where g++ does not, frexp and rint are other routines: held to the same bounds, not bitwise)
def test_sincos_device(dev):
    cpu.check_sincos(dev)


def test_arm_segments_device(dev):
    cpu.check_arm_segments(dev)


def test_self_row_device(dev):
    cpu.check_self_row(dev)


def test_logacc_device(dev):
    cpu.check_logacc(dev)
