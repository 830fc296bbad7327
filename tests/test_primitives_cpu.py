"""The kernels' primitives one at a time, HOST side: the entry points mmpc_emu_prim_* of the lane-emulation build
(tests/emu/mmpc_emu.cpp) against references that are independent of both builds - fractions.Fraction for everything
algebraic (a double is a rational), math.fsum / numpy for reductions and permutations, mpmath at 200 bits for log / sin / cos.

Two kinds of functions pass through here:
  * functions whose source both builds share (mmpc_sincos, mmpc_arm_segments[_fast], mmpc_log_mant / MmpcLogAcc,
    mmpc_self_row, mmpc_z_safeguard): their accuracy bounds are established here, on a machine without a GPU, and
    tests/test_gpu_primitives.py runs the same checks (the check_* functions below) through the device library;
  * the stand-ins the emulation puts in place of gfx950 hardware (mmpc_emu_red, mmpc_emu_red4, mmpc_emu_red_arr, the fma
    loops of MMPC_MFMA, MMPC_LANE_*): checked against the references here so that a failure of "device == stand-in" on the
    GPU can be attributed to one side.
Also here: the cross-compile of the device library for gfx950 in its three variants (no GPU needed)."""
import math
from fractions import Fraction

import numpy as np
import pytest

import emu_helper
import prim_helper as P

try:
    import mpmath as mp
except ImportError:          # resolution of the fall-back: 2^-64 (numpy.longdouble); the bounds below are >= 2^-53
    mp = None

U = 2.0 ** -53               # unit roundoff
SEED = 20261016


def host():
    return P.host()


def ulp(x):
    """spacing of the doubles at |x| (x: a float or an array)"""
    return np.spacing(np.abs(np.asarray(x, float)))


# ---------------------------------------------------------------------------------------------------------------- references
def _hp(v):
    return mp.mpf(float(v)) if mp is not None else np.longdouble(v)


def _hpfun():
    return (mp.sin, mp.cos, mp.log, mp.sqrt) if mp is not None else (np.sin, np.cos, np.log, np.sqrt)


class _prec:
    """200 bits of working precision (mpmath), or nothing to set (numpy.longdouble)"""

    def __init__(self, dps=None):
        self.ctx = None if mp is None else (mp.workdps(dps) if dps else mp.workprec(200))

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *a):
        if self.ctx is not None:
            self.ctx.__exit__(*a)


def ref_arm_segments(q1, q2, q3):
    """oracle/nlp.py:arm_segments re-evaluated in high precision (arguments already high-precision numbers): (dr[3], dz[3])"""
    from oracle import nlp
    sin, cos = _hpfun()[:2]
    A2, A3, A5, A6, A7 = (_hp(v) for v in (nlp.A2, nlp.A3, nlp.A5, nlp.A6, nlp.A7))
    a, b = q1 - q2, q1 - q2 - q3
    s1, c1, sA, cA, sB, cB = sin(q1), cos(q1), sin(a), cos(a), sin(b), cos(b)
    return [A2 * s1 + A3 * c1, -A3 * cA + A5 * sA, A6 * cB - A7 * sB], [A2 * c1 - A3 * s1, A3 * sA + A5 * cA, -A6 * sB - A7 * cB]


def ref_self_row(i, x6):
    """oracle/nlp.py:selfcol_row_direct (world points of wholebody_fk) in high precision; x6 = x, y, psi, q1, q2, q3"""
    from oracle import nlp
    sin, cos, _, sqrt = _hpfun()
    px, py, psi = x6[0], x6[1], x6[2]
    dr, dz = ref_arm_segments(x6[3], x6[4], x6[5])
    c, s = cos(psi), sin(psi)
    bx, bz = _hp(nlp.BASELINK2JOINT1_X), _hp(nlp.BASELINK2JOINT1_Z)

    def lift(r, z):
        return (px + (r + bx) * c, py + (r + bx) * s, z + bz)
    j2 = lift(dr[0], dz[0]); j3 = lift(dr[0] + dr[1], dz[0] + dz[1]); e = lift(dr[0] + dr[1] + dr[2], dz[0] + dz[1] + dz[2])
    pts = [(0 * px,) * 3, tuple(v / 2 for v in j2), j2, tuple((u + v) / 2 for u, v in zip(j2, j3))]
    d = [u - v for u, v in zip(pts[i], e)]
    return _hp(nlp.SELF_COLLISION_RADIUS) - sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])


# ---------------------------------------------------------------------------------------------------------------- inputs
def sincos_inputs(rng):
    """log-uniform in +-[1e-8, 1e6]; uniform in +-[0, 8] (the joint and heading range); the doubles nearest to k pi/2 (k =
    1..2000 and 64 random k up to 6.3e5: |x| up to 1e6) with their two neighbours, both signs"""
    n = 8192
    a = 10.0 ** rng.uniform(-8, 6, n) * rng.choice([-1.0, 1.0], n)
    b = rng.uniform(-8, 8, n)
    ks = np.concatenate([np.arange(1, 2001), rng.integers(2001, 630001, 64)])
    with _prec():
        hpi = mp.pi / 2 if mp is not None else np.longdouble(math.pi) / 2 + np.longdouble(6.123233995736766e-17)
        c = np.array([float(int(k) * hpi) for k in ks])
    c = np.concatenate([np.nextafter(c, -np.inf), c, np.nextafter(c, np.inf)])
    c = np.concatenate([c, -c[::7]])
    return np.concatenate([a, b, c])


def red_families(rng):
    """vectors of 64 doubles without a NaN, by family"""
    f = {}
    f["normal"] = rng.standard_normal((256, 64))
    f["loguniform"] = 10.0 ** rng.uniform(-30, 30, (256, 64)) * rng.choice([-1.0, 1.0], (256, 64))
    f["onehot"] = 1.5 * np.eye(64)                                    # a dropped or doubled lane gives 0 or 3
    half = rng.standard_normal((64, 32)) * 10.0 ** rng.uniform(-3, 6, (64, 1))
    c = np.concatenate([half, -half], axis=1)
    c[:, 0] += 1e-9 * rng.standard_normal(64)                         # cancels to a small remainder
    f["cancel"] = rng.permuted(c, axis=1)
    f["equal"] = np.repeat(np.array([0.0, 1.0, -1.0, 0.1, 1e-300, -3e200, 2.0 ** -1040, 7.25])[:, None], 64, axis=1)
    inf = rng.standard_normal((128, 64))
    inf[np.arange(64), np.arange(64)] = np.inf
    inf[64 + np.arange(64), np.arange(64)] = -np.inf
    f["inf"] = inf
    return f


def red4_inputs(rng):
    """(n, 4, 64): a, b, c, d.  First 64: four different values at four different one-hot positions, over all positions (pins
    out[0..3] <-> (a, b, c, d)); then 64 random quadruples"""
    oh = np.zeros((64, 4, 64))
    for p in range(64):
        for j in range(4):
            oh[p, j, (p + 17 * j) % 64] = 1.5 + j
    return np.concatenate([oh, rng.standard_normal((64, 4, 64))])


def mfma_int_inputs(rng):
    """(A (16,4), B (4,16), C (16,16)) with integer entries |.| <= 64: 64 random triples, then each element of A set alone (B
    random), then each element of B set alone (A random): pins the lane <-> element map element by element"""
    out = []
    ri = lambda *s: rng.integers(-64, 65, s).astype(float)
    for _ in range(64):
        out.append((ri(16, 4), ri(4, 16), ri(16, 16)))
    for e in range(64):
        A = np.zeros((16, 4)); A[e // 4, e % 4] = 1 + e
        out.append((A, ri(4, 16), np.zeros((16, 16))))
    for e in range(64):
        B = np.zeros((4, 16)); B[e // 16, e % 16] = 1 + e
        out.append((ri(16, 4), B, np.zeros((16, 16))))
    return out


def mfma_real_inputs(rng):
    """normal entries; magnitudes 1e-8 .. 1e8 with random signs"""
    out = []
    m = lambda *s: 10.0 ** rng.uniform(-8, 8, s) * rng.choice([-1.0, 1.0], s)
    for _ in range(16):
        out.append((rng.standard_normal((16, 4)), rng.standard_normal((4, 16)), rng.standard_normal((16, 16))))
    for _ in range(16):
        out.append((m(16, 4), m(4, 16), m(16, 16)))
    return out


# ---------------------------------------------------------------------------------------------------------------- checks
# (each takes the library - host or device - and returns what it measured; the GPU module runs them on the device library)
def check_sincos(lib):
    """absolute error <= 2^-52 everywhere (|x| up to 1e6, the neighbours of k pi/2 included); <= 2 ulp of the result for |x| <= 8"""
    x = sincos_inputs(np.random.default_rng(SEED))
    got = lib.map("sincos", x)
    sin, cos = _hpfun()[:2]
    worst_abs, worst_ulp, at_abs, at_ulp = 0.0, 0.0, None, None
    with _prec():
        for xi, (s, c) in zip(x, got):
            for g, r in ((s, sin(_hp(xi))), (c, cos(_hp(xi)))):
                err = abs(float(_hp(g) - r))
                if err > worst_abs:
                    worst_abs, at_abs = err, xi
                if abs(xi) <= 8 and err / ulp(float(r)) > worst_ulp:
                    worst_ulp, at_ulp = err / ulp(float(r)), xi
    print("mmpc_sincos: worst absolute error %.3e (bound 2^-52 = %.3e) at x = %r; worst error for |x| <= 8: %.3f ulp (bound 2) at x = %r"
          % (worst_abs, 2.0 ** -52, at_abs, worst_ulp, at_ulp))
    assert worst_abs <= 2.0 ** -52, (worst_abs, at_abs)
    assert worst_ulp <= 2.0, (worst_ulp, at_ulp)
    return dict(abs=worst_abs, ulp=worst_ulp)


def check_arm_segments(lib):
    """mmpc_arm_segments / _fast against oracle/nlp.py:arm_segments in high precision: <= 4 ulp of the largest link length"""
    from oracle import nlp
    rng = np.random.default_rng(SEED + 1)
    q = np.concatenate([rng.uniform(-3.0, 3.0, (2048, 3)), [[0, 0, 0], [math.pi / 2, 0, 0], [math.pi / 2, math.pi / 2, math.pi / 2], [-2.9, 2.9, -2.9]]])
    bound = 4 * float(ulp(max(nlp.A2, nlp.A3, nlp.A5, nlp.A6, nlp.A7)))    # 2.2e-16
    res = {}
    for name in ("arm", "arm_fast"):
        got = lib.map(name, q[:, 0], q[:, 1], q[:, 2])
        worst = 0.0
        with _prec():
            for qi, g in zip(q, got):
                dr, dz = ref_arm_segments(*[_hp(v) for v in qi])
                worst = max(worst, max(abs(float(_hp(g[j]) - dr[j])) for j in range(3)), max(abs(float(_hp(g[3 + j]) - dz[j])) for j in range(3)))
        print("mmpc_%s_segments: worst absolute error %.3e (bound %.3e)" % (name, worst, bound))
        assert worst <= bound, (name, worst)
        res[name] = worst
    return res


def check_self_row(lib):
    """value against nlp.selfcol_row_direct (1e-14); gradient against a central difference of the high-precision value in
    60-digit arithmetic, h = 1e-20 (truncation and rounding ~1e-40): <= 1e-12"""
    from oracle import nlp
    rng = np.random.default_rng(SEED + 2)
    n = 96
    X = np.column_stack([rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), rng.uniform(-math.pi, math.pi, n), rng.uniform(-2.8, 2.8, n),
                         rng.uniform(-2.8, 2.8, n), rng.uniform(-2.8, 2.8, n)])
    wv, wg = 0.0, 0.0
    for i in range(4):
        got = lib.map("self_row", float(i), *[X[:, j] for j in range(6)])
        for x6, g in zip(X, got):
            x9 = np.zeros(9); x9[:3] = x6[:3]; x9[6:] = x6[3:]
            wv = max(wv, abs(g[0] - nlp.selfcol_row_direct(x9, i)))
            if mp is None:      # (no 60-digit arithmetic without mpmath: the value only)
                continue
            with _prec(60):
                h = mp.mpf(10) ** -20
                xm = [mp.mpf(float(v)) for v in x6]
                wv = max(wv, abs(float(ref_self_row(i, xm) - mp.mpf(float(g[0])))))
                for a in range(6):
                    xp = list(xm); xp[a] += h
                    xn = list(xm); xn[a] -= h
                    d = (ref_self_row(i, xp) - ref_self_row(i, xn)) / (2 * h)
                    wg = max(wg, abs(float(d - mp.mpf(float(g[1 + a])))))
    print("mmpc_self_row: worst value error %.3e (bound 1e-14), worst gradient error %.3e (bound 1e-12)" % (wv, wg))
    assert wv <= 1e-14 and wg <= 1e-12, (wv, wg)
    return dict(value=wv, grad=wg)


def logacc_cases(rng):
    """(factors (14, padded with the exact factor 1.0), ex, k), k in {1, 2, 9, 10, 14}: all 1e-15; all 9.9e18 (the underflow and
    overflow margins of the shipped shapes: box slacks lie in [1e-15 (mmpc_box_t), 2 x 9.9e18 (mmpc_bound_active)]); log-uniform
    over [1e-15, 9.9e18]; all in [0.5, 2]; each with ex = 0 and with a non-zero ex handed in"""
    out = []
    for k in (1, 2, 9, 10, 14):
        fam = [np.full(k, 1e-15), np.full(k, 9.9e18)]
        fam += [10.0 ** rng.uniform(-15, math.log10(9.9e18), k) for _ in range(32)]
        fam += [rng.uniform(0.5, 2.0, k) for _ in range(32)]
        for t in fam:
            for ex in (0, 37, -211):
                out.append((np.concatenate([t, np.ones(P.LOGACC_K - k)]), ex, k))
    return out


def check_logacc(lib):
    """|value - (sum log t_i + ex log 2)| <= (k + 2) 2^-53 + 2 x 2^-53 |value|  (k roundings of the product, the series, the
    final sum); the product stays finite and normal"""
    cases = logacc_cases(np.random.default_rng(SEED + 3))
    F = np.array([c[0] for c in cases]); ex = np.array([float(c[1]) for c in cases])
    got = lib.map("logacc", *[F[:, j] for j in range(P.LOGACC_K)], ex)
    log = _hpfun()[2]
    worst = 0.0
    with _prec():
        for (t, e, k), (val, mant) in zip(cases, got):
            assert np.isfinite(mant) and abs(mant) >= np.finfo(float).tiny, ("the product left the normal range", t[:k], mant)
            ref = sum(log(_hp(v)) for v in t[:k]) + e * log(_hp(2))
            err = float(abs(_hp(val) - ref))
            bound = (k + 2) * U + 2 * U * abs(val)
            worst = max(worst, err / bound)
            assert err <= bound, (t[:k], e, val, err, bound)
    print("MmpcLogAcc: worst error / bound = %.3f over %d cases" % (worst, len(cases)))
    return worst


def exact_sum_err(v, s):
    """|s - sum(v)| and sum(|v|) in rational arithmetic"""
    fr = [Fraction(float(a)) for a in v]
    return abs(Fraction(float(s)) - sum(fr)), sum(abs(a) for a in fr)


def check_reductions(lib):
    """all 64 lanes return the same bits; max / min equal numpy's exactly; a sum s satisfies |s - sum(v)| <= 6 x 2^-53 x sum(|v|)
    (six levels of pairwise addition; exact rational arithmetic, which is what math.fsum rounds).  Returns {family: (n, 7)}"""
    out = {}
    worst = 0.0
    for name, V in red_families(np.random.default_rng(SEED + 4)).items():
        R = lib.red(V)
        assert (R.view(np.uint64) == R.view(np.uint64)[:, :, :1]).all(), "%s: the lanes differ" % name
        R = R[:, :, 0]
        for v, r in zip(V, R):
            assert r[1] == r[4] == r[6] == v.max(), (name, v, r)
            assert r[2] == r[5] == v.min(), (name, v, r)
            for s in (r[0], r[3]):
                if not np.isfinite(v).all():
                    assert s == math.fsum(v), (name, s)
                    continue
                err, mag = exact_sum_err(v, s)
                assert err <= 6 * Fraction(U) * mag, (name, v, s, float(err))
                if mag:
                    worst = max(worst, float(err / mag) / U)
        if name == "onehot":
            assert (R[:, [0, 1, 3, 4, 6]] == 1.5).all() and (R[:, [2, 5]] == 0.0).all()
        out[name] = R
    print("wave sums: worst |s - sum(v)| / sum|v| = %.3f x 2^-53 (bound 6)" % worst)
    return out


def check_red4(lib):
    """the four-at-a-time reductions: lanes agree; out[0..3] <-> (a, b, c, d); maxima exact, sums within the pairwise bound"""
    V = red4_inputs(np.random.default_rng(SEED + 5))
    R = lib.red4(V)
    assert (R.view(np.uint64) == R.view(np.uint64)[:, :, :1]).all(), "the lanes differ"
    R = R[:, :, 0]
    for p in range(64):
        assert (R[p, :4] == [1.5, 2.5, 3.5, 4.5]).all() and (R[p, 4:] == [1.5, 2.5, 3.5, 4.5]).all(), (p, R[p])
    for v, r in zip(V, R):
        for j in range(4):
            assert r[4 + j] == v[j].max()
            err, mag = exact_sum_err(v[j], r[j])
            assert err <= 6 * Fraction(U) * mag
    return R


def check_mfma_exact(lib):
    """integer operands: D = A B (MMPC_MFMA0) and D = A B + C (MMPC_MFMA) exactly; every element of A and of B alone"""
    cases = mfma_int_inputs(np.random.default_rng(SEED + 6))
    R = lib.mfma(np.stack([P.tile_pack(*c) for c in cases]))
    for n, ((A, B, Cm), r) in enumerate(zip(cases, R)):
        Ai, Bi, Ci = A.astype(np.int64), B.astype(np.int64), Cm.astype(np.int64)
        assert (P.acc_unpack(r[:4]) == (Ai @ Bi).astype(float)).all(), ("MMPC_MFMA0", n)
        assert (P.acc_unpack(r[4:]) == (Ai @ Bi + Ci).astype(float)).all(), ("MMPC_MFMA", n)


def check_mfma_real(lib):
    """|D - exact| <= 4 x 2^-53 (|A| |B| + |C|) elementwise, exact in rational arithmetic.  Returns the raw results"""
    cases = mfma_real_inputs(np.random.default_rng(SEED + 7))
    R = lib.mfma(np.stack([P.tile_pack(*c) for c in cases]))
    worst = 0.0
    fr = np.vectorize(lambda v: Fraction(float(v)), otypes=[object])
    for (A, B, Cm), r in zip(cases, R):
        Af, Bf, Cf = fr(A), fr(B), fr(Cm)
        for acc, Cx in ((r[:4], None), (r[4:], Cf)):
            D = fr(P.acc_unpack(acc))
            ex = Af.dot(Bf) + (Cx if Cx is not None else 0)
            mag = np.abs(Af).dot(np.abs(Bf)) + (np.abs(Cx) if Cx is not None else 0)
            ratio = max(abs(d - e) / m for d, e, m in zip(D.ravel(), ex.ravel(), mag.ravel()))
            assert ratio <= 4 * Fraction(U), float(ratio)
            worst = max(worst, float(ratio) / U)
    print("MMPC_MFMA on real entries: worst |D - exact| / (|A| |B| + |C|) = %.3f x 2^-53 (bound 4)" % worst)
    return R


def check_mfma_chain(lib):
    """the chaining claim of mmpc_tile.h: the accumulator registers of D1 are the K-blocks of a B operand as they stand, those
    of a symmetric S the K-blocks of an A operand: sum_r MFMA(A = S[r], B = D1[r]) = S D1 without lane movement.  With the
    roles exchanged the registers of D1 stand for D1^T as an A operand: sum_r MFMA(A = D1[r], B = S[r]) = D1^T S, which is
    D1 S for a symmetric D1 (every second case)."""
    rng = np.random.default_rng(SEED + 8)
    items, exp = [], []
    for n in range(32):
        S = rng.integers(-9, 10, (16, 16)); S = S + S.T
        D1 = rng.integers(-9, 10, (16, 4)) @ rng.integers(-9, 10, (4, 16))
        if n % 2:
            D1 = D1 + D1.T
        items.append(np.concatenate([P.acc_pack(S), P.acc_pack(D1)]))
        exp.append((S @ D1, D1.T @ S, D1 @ S if n % 2 else None))
    R = lib.chain(np.stack(items))
    for r, (SD, DtS, DS) in zip(R, exp):
        assert (P.acc_unpack(r[:4]) == SD.astype(float)).all()
        assert (P.acc_unpack(r[4:]) == DtS.astype(float)).all()
        if DS is not None:
            assert (P.acc_unpack(r[4:]) == DS.astype(float)).all()


def lane_vectors(rng):
    """uint64 test words: (i) both 32-bit halves identify the lane and differ from each other (a swapped half or lane shows);
    (ii) 256 random bit patterns per lane with NaN payloads, -0.0 and subnormals among them (an exchange moves two 32-bit
    words and must not canonicalise anything)"""
    l = np.arange(64, dtype=np.uint64)
    tagged = ((np.uint64(0xA5000000) | l) << np.uint64(32)) | (np.uint64(0x5A000000) | (l << np.uint64(8)))
    rnd = rng.integers(0, 2 ** 64, (256, 64), dtype=np.uint64)
    rnd[0, ::3] = np.uint64(0x7FF0000000000001) + l[::3]            # signalling NaN payloads
    rnd[1, ::2] = np.uint64(0xFFF8000000000000) | (l[::2] << np.uint64(7))
    rnd[2, :] = np.where(l % 2 == 0, np.uint64(0x8000000000000000), l + np.uint64(1))   # -0.0 and subnormals
    return np.concatenate([tagged[None], rnd])


def lane_expected(v):
    """{row: expected (64,) uint64} of one vector, as numpy indexing with l the lane"""
    l = np.arange(64)
    e = {}
    for j in range(64):
        e[P.LANE_READLANE + j] = np.repeat(v[j], 64)
    for j in range(16):
        e[P.LANE_ROWBCAST + j] = v[(l & ~15) + j]
    for j in range(9):
        e[P.LANE_RBALL9 + j] = v[(l & ~15) + j]
    for j in range(6):
        e[P.LANE_RBALL6 + j] = v[(l & ~15) + j]
    e[P.LANE_DPP + 0] = v[l ^ 1]
    e[P.LANE_DPP + 1] = v[l ^ 2]
    e[P.LANE_DPP + 2] = v[(l & ~7) | (7 - (l & 7))]
    e[P.LANE_DPP + 3] = v[(l & ~15) | (15 - (l & 15))]
    e[P.LANE_XOR16] = v[l ^ 16]
    e[P.LANE_LOWER16] = v[l & ~16]
    e[P.LANE_XOR32] = v[l ^ 32]
    return e


def check_lanes(lib, rows):
    """bit-exact on the uint64 view"""
    V = lane_vectors(np.random.default_rng(SEED + 9))
    R = lib.lanes(V.view(np.float64)).view(np.uint64)
    for v, r in zip(V, R):
        e = lane_expected(v)
        for row in rows:
            assert (r[row] == e[row]).all(), ("row %d" % row, [hex(int(a)) for a in r[row][:20]], [hex(int(a)) for a in e[row][:20]])


# the exchanges the emulation has a stand-in for (MMPC_LANE_GET, MMPC_LANE_XOR16, MMPC_LANE_LOWER16)
HOST_LANE_ROWS = list(range(P.LANE_READLANE, P.LANE_READLANE + 64)) + [P.LANE_XOR16, P.LANE_LOWER16]

# ---- edge values.  What each function returns, by class, on the device and in the emulation, derived from the code:
#   mmpc_rcp(+-0): r = v_rcp = +-inf, e = fma(-x, r, 1) = fma(0, inf, 1) = NaN -> NaN (the emulation: 1.0 / 0 = +-inf);
#   mmpc_rcp(+-inf): r = +-0, e = fma(inf, 0, 1) = NaN (the emulation: +-0); a subnormal x: r = inf, e = -inf, e e + e = NaN
#   (mmpc_rcp_piv: fma(e, r, r) = -inf + inf = NaN; the emulation: +inf).  mmpc_rsqrt(+-0): y = +-inf, x y = NaN;
#   mmpc_rsqrt(inf): y = 0, x y = NaN (the emulation: +inf, -inf, +0).  mmpc_sqrt_pair starts like mmpc_rsqrt: NaN, NaN at
#   +-0 and inf (the emulation: n = sqrt(m), inv = -1 / (2 n): (+-0, -+inf), (inf, -0)).  mmpc_powf: (float)x, then log2 and
#   exp2 in single precision: 0, everything below the single-precision normals -> 0; above its range -> inf.
EDGES = {"+0": 0.0, "-0": -0.0, "+inf": np.inf, "-inf": -np.inf, "nan": np.nan, "min_normal": 2.2250738585072014e-308,
         "subnormal": 1e-310, "max_finite": 1.7976931348623157e308, "negative": -3.0}
_E = list(EDGES)
#                       +0      -0      +inf    -inf    nan    min_normal subnormal max_finite negative
EDGE_DEVICE = {
    "rcp":            ["nan",  "nan",  "nan",  "nan",  "nan", "fin",     "nan",    "fin",     "fin"],
    "rcp3":           ["nan",  "nan",  "nan",  "nan",  "nan", "fin",     "nan",    "fin",     "fin"],
    "rcp_piv":        ["nan",  "nan",  "nan",  "nan",  "nan", "fin",     "nan",    "fin",     "fin"],
    "rsqrt":          ["nan",  "nan",  "nan",  "nan",  "nan", "fin",     "fin",    "fin",     "nan"],
    "sqrt_pair.n":    ["nan",  "nan",  "nan",  "nan",  "nan", "fin",     "fin",    "fin",     "nan"],
    "sqrt_pair.inv":  ["nan",  "nan",  "nan",  "nan",  "nan", "fin",     "fin",    "fin",     "nan"],
    "powf":           ["+0",   "+0",   "+inf", "nan",  "nan", "+0",      "+0",     "+inf",    "nan"],
}
EDGE_HOST = {
    "rcp":            ["+inf", "-inf", "+0",   "-0",   "nan", "fin",     "+inf",   "fin",     "fin"],
    "rcp3":           ["+inf", "-inf", "+0",   "-0",   "nan", "fin",     "+inf",   "fin",     "fin"],
    "rcp_piv":        ["+inf", "-inf", "+0",   "-0",   "nan", "fin",     "+inf",   "fin",     "fin"],
    "rsqrt":          ["+inf", "-inf", "+0",   "nan",  "nan", "fin",     "fin",    "fin",     "nan"],
    "sqrt_pair.n":    ["+0",   "-0",   "+inf", "nan",  "nan", "fin",     "fin",    "fin",     "nan"],
    "sqrt_pair.inv":  ["-inf", "+inf", "-0",   "nan",  "nan", "fin",     "fin",    "fin",     "nan"],
    "powf":           ["+0",   "+0",   "+inf", "nan",  "nan", "+0",      "+0",     "+inf",    "nan"],
}


def classify(v):
    if v != v:
        return "nan"
    if math.isinf(v):
        return "+inf" if v > 0 else "-inf"
    if v == 0:
        return "-0" if math.copysign(1.0, v) < 0 else "+0"
    return "fin"


def _edge_rel_err(name, x, v):
    """relative error of the finite non-zero value v the function returned at x > 0 or (reciprocals) x < 0, exactly"""
    X, V = Fraction(x), Fraction(v)
    if name.startswith("rcp"):
        return abs(V * X - 1)
    y = {"rsqrt": V, "sqrt_pair.n": 1 / V, "sqrt_pair.inv": -2 * V}[name]     # each an approximation of 1 / sqrt(x)
    return abs(y * y * X - 1) / 2


def check_edges(lib, table):
    """the class table holds; a NaN in gives a NaN out; no edge input gives a finite non-zero WRONG value (relative error above
    1e-6, the tolerance of the parity tests: such a value would pass the `!(p > 0)` pivot test and the status 2 test unseen)"""
    x = np.array([EDGES[k] for k in _E])
    got = {n: lib.map(n, x) for n in ("rcp", "rcp3", "rcp_piv", "rsqrt")}
    sp = lib.map("sqrt_pair", x)
    got["sqrt_pair.n"], got["sqrt_pair.inv"] = sp[:, 0], sp[:, 1]
    got["powf"] = lib.map("powf", x, 1.1)
    seen = {n: [classify(float(v)) for v in g] for n, g in got.items()}
    print("%-14s %s" % ("", " ".join("%10s" % k for k in _E)))
    for n in table:
        print("%-14s %s" % (n, " ".join("%10s" % c for c in seen[n])))
    for n in table:
        assert seen[n] == table[n], (n, seen[n], table[n])
        assert seen[n][_E.index("nan")] == "nan"
        for k, c, v in zip(_E, seen[n], got[n]):
            if c == "fin" and n != "powf":
                assert _edge_rel_err(n, EDGES[k], float(v)) <= Fraction(1, 10 ** 6), (n, k, v)
    return seen


def zsafe_inputs(rng):
    """(z, t, mu): mu log-uniform in [1e-12, 1e2] (from mu_init down to a tenth of the tightest tolerance), t in [1e-15, 1e3]
    (mmpc_box_t's floor up to the widest box), z t / mu log-uniform in [1e-14, 1e14] (kappa = 1e10: all three branches), plus z
    within +-8 ulp of both branch boundaries"""
    n = 1 << 13
    mu = 10.0 ** rng.uniform(-12, 2, n); t = 10.0 ** rng.uniform(-15, 3, n)
    z = mu / t * 10.0 ** rng.uniform(-14, 14, n)
    zb, tb, mb = [], [], []
    for i in range(128):
        m, tt = 10.0 ** rng.uniform(-12, 2), 10.0 ** rng.uniform(-15, 3)
        for kap in (1e10, 1e-10):
            z0 = kap * m / tt
            for j in range(-8, 9):
                zb.append(z0 * (1 + j * 2.0 ** -52)); tb.append(tt); mb.append(m)
    return np.concatenate([z, zb]), np.concatenate([t, tb]), np.concatenate([mu, mb])


def check_zsafe(lib):
    """mmpc_z_safeguard_fast (one reciprocal, a clamp) against mmpc_z_safeguard (two divisions, three branches): equal to 4 ulp;
    and both against the exact clamp of z to [mu / (kappa t), kappa mu / t]: away from a branch boundary by more than 4 ulp they
    take the branch the exact quotient z t / mu asks for (the middle branch returns z itself, bit for bit; a clamped value lies
    within 4 ulp of the exact bound)"""
    z, t, mu = zsafe_inputs(np.random.default_rng(SEED + 10))
    fast = lib.map("zsafe_fast", z, t, mu)
    slow = lib.map("zsafe", z, t, mu)
    kap = Fraction(10 ** 10)
    for zi, ti, mi, f, s in zip(z, t, mu, fast, slow):
        assert abs(f - s) <= 4 * ulp(s), (zi, ti, mi, f, s)
        Z, T, M = Fraction(float(zi)), Fraction(float(ti)), Fraction(float(mi))
        rho = Z * T / M
        if min(abs(rho / kap - 1), abs(rho * kap - 1)) <= 4 * Fraction(2) ** -52:
            continue
        for g in (f, s):
            if rho > kap:
                assert g != zi and abs(Fraction(float(g)) - kap * M / T) <= 4 * Fraction(float(ulp(g))), ("upper", zi, ti, mi, g)
            elif rho < 1 / kap:
                assert g != zi and abs(Fraction(float(g)) - M / (kap * T)) <= 4 * Fraction(float(ulp(g))), ("lower", zi, ti, mi, g)
            else:
                assert g == zi, ("middle", zi, ti, mi, g)


def mul24_pairs(rng):
    s = [0, 1, 2, 3, 63, 64, 255, 4095, 4096, 2 ** 16, 2 ** 24 - 1]
    p = [(a, b) for a in s for b in s if a * b < 2 ** 31]
    return np.concatenate([np.array(p), rng.integers(0, 2 ** 15, (1 << 16, 2))])


def check_mul24(lib):
    p = mul24_pairs(np.random.default_rng(SEED + 11))
    got = lib.map("mul24", p[:, 0].astype(float), p[:, 1].astype(float))
    assert (got == (p[:, 0].astype(np.int64) * p[:, 1].astype(np.int64)).astype(float)).all()


def check_powf(lib):
    """x^e in single precision: relative error against x**e <= 1e-5 for x in [1e-30, 1e4], e in {1.1, 2.3} (the exponents of the
    filter's switching rule); 0 and every x below the smallest single-precision normal give 0.
    Named cases: x = 3.2e-17 and 1e-20 with e = 2.3 (x^e lies below the single-precision range from x = 3.2e-17 down)"""
    rng = np.random.default_rng(SEED + 12)
    x = np.concatenate([10.0 ** rng.uniform(-30, 4, 4096), [1e-30, 1e4, 1.0, 3.2e-17, 1e-20]])
    worst, at = 0.0, None
    for e in (1.1, 2.3):
        got = lib.map("powf", x, e)
        with _prec():
            for xi, g in zip(x, got):
                ref = _hp(xi) ** _hp(np.float32(e))          # (the exponent the function is handed is the float)
                err = float(abs(_hp(g) - ref) / ref)
                if err > worst:
                    worst, at = err, (xi, e)
        tiny = np.array([0.0, 1e-320, 1e-300, 1e-45, 1.1e-38])
        assert (lib.map("powf", tiny, e) == 0.0).all(), lib.map("powf", tiny, e)
    print("mmpc_powf: worst relative error %.3e at (x, e) = %r (bound 1e-5)" % (worst, at))
    assert worst <= 1e-5, (worst, at)
    return worst


# ---------------------------------------------------------------------------------------------------------------- tests
def test_sincos_host():
    check_sincos(host())


def test_arm_segments_host():
    check_arm_segments(host())


def test_self_row_host():
    check_self_row(host())


def test_logacc_host():
    check_logacc(host())


def test_log_mant_host():
    """mmpc_log_mant alone over every positive normal (it renormalises with frexp): the value lies in [log sqrt(1/2), log
    sqrt(2)] and |value + ex log 2 - log m| <= 3 x 2^-53 (1 + |log m|)"""
    rng = np.random.default_rng(SEED + 13)
    m = np.concatenate([rng.uniform(0.0, 1.0, 2048), 10.0 ** rng.uniform(-300, 300, 2048), [1.0, 0.5, 0.70710678118654752440, 2.0 ** -1022]])
    got = host().map("log_mant", m)
    log = _hpfun()[2]
    with _prec():
        for mi, (v, e) in zip(m, got):
            assert -0.3466 <= v <= 0.3466
            ref = log(_hp(mi))
            err = float(abs(_hp(v) + int(e) * log(_hp(2)) - ref))
            assert err <= 3 * U * (1 + abs(float(ref))), (mi, v, e, err)


def test_reductions_host_standins():
    """mmpc_emu_red (rows 0-2) and mmpc_emu_red_arr (rows 3-6) against exact sums / numpy"""
    check_reductions(host())


def test_red4_host_standin():
    check_red4(host())


def test_reduction_nan_host_standin():
    """A NaN in lane p.  The sums and MAXERR return NaN for every p.  The ternary max / min of the stand-in (a > b ? a : b)
    keeps a NaN that arrives as the partner's value and drops one the lane holds itself, so the two lanes of a pair no longer
    agree after a step: what lane 0 ends with is, depending on p, the NaN or the maximum over a SUBSET of the other lanes -
    unlike the device (v_max_f64 drops the NaN for every p and returns the maximum of the other 63, asserted in
    test_gpu_primitives.py).  Neither build relies on the maxima for NaNs: the sum over the same vector is NaN, which is what
    the status 2 test of the main loop sees."""
    rng = np.random.default_rng(SEED + 14)
    V = rng.standard_normal((64, 64))
    V[np.arange(64), np.arange(64)] = np.nan
    R = host().red(V)[:, :, 0]
    assert np.isnan(R[:, [0, 3, 6]]).all()
    kept = np.isnan(R[:, 1])
    assert kept.any() and not kept.all()
    for p in np.flatnonzero(~kept):
        assert R[p, 1] in V[p] and R[p, 1] <= np.nanmax(V[p])


def test_vmax_host_standin_semantics():
    """the stand-in of mmpc_vmax / mmpc_vmin hands a NaN in its SECOND argument through and drops one in its first (the device:
    v_max_f64 / v_min_f64 drop either, as numpy.fmax / fmin - asserted in test_gpu_primitives.py); mmpc_max_err keeps both"""
    h = host()
    assert np.isnan(h.map("vmax", 1.0, np.nan)) and h.map("vmax", np.nan, 1.0) == 1.0
    assert np.isnan(h.map("vmin", 1.0, np.nan)) and h.map("vmin", np.nan, 1.0) == 1.0
    rng = np.random.default_rng(SEED + 15)
    a, b = rng.standard_normal(4096), rng.standard_normal(4096)
    assert (h.map("vmax", a, b) == np.fmax(a, b)).all() and (h.map("vmin", a, b) == np.fmin(a, b)).all()
    assert np.isnan(h.map("max_err", np.nan, 1.0)) and np.isnan(h.map("max_err", 1.0, np.nan))


def test_mfma_host_standin():
    h = host()
    check_mfma_exact(h)
    check_mfma_real(h)
    check_mfma_chain(h)


def test_lane_standins_host():
    check_lanes(host(), HOST_LANE_ROWS)


def test_edge_values_host():
    check_edges(host(), EDGE_HOST)


def test_zsafe_host():
    check_zsafe(host())


def test_powf_host():
    check_powf(host())


def test_mul24_host_and_lds_offsets():
    """MMPC_MUL24 multiplies LDS word offsets: exact while both factors are below 2^24.  Every byte offset of a slab the kernels
    accept is: 8 x mmpc_emu_lds_doubles <= 160 KiB < 2^24 (the accepted envelope ends at the LDS limit, test_emu_kernel.py)"""
    check_mul24(host())
    assert 160 * 1024 < 2 ** 24
    for kind, N, M, ops in [(0, 20, 5, False), (0, 30, 8, False), (1, 15, 3, False), (2, 10, 2, False), (0, 20, 5, True)]:
        assert 0 < emu_helper.lds_bytes(kind, N, M, ops) <= 160 * 1024


@pytest.mark.parametrize("defs", [(), ("MMPC_RCP_NEWTON=1",), ("MMPC_PIV_NEWTON=0",)], ids=["default", "rcp_newton", "piv_cubic"])
def test_device_library_cross_compiles(defs):
    """hipcc --offload-arch=gfx950 builds tests/gpu_prim/mmpc_prim.hip without a GPU, in the three variants the GPU module uses"""
    if P.hipcc() is None:
        pytest.skip("no hipcc on this machine")
    import ctypes
    import os
    lib = P.build(defs)
    assert os.path.getsize(lib) > 0
    want = (1 if "MMPC_RCP_NEWTON=1" in defs else 0) | (0 if "MMPC_PIV_NEWTON=0" in defs else 2)
    assert ctypes.CDLL(lib).mmpc_prim_switches() == want
