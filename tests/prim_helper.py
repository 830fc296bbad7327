"""ctypes driver for the primitive test library (tests/gpu_prim/mmpc_prim.hip: the kernels' device-only primitives, one per
launch, on the GPU) and for its host twin in the lane-emulation build (tests/emu/mmpc_emu.cpp, mmpc_emu_prim_*).
TEST ONLY: never used by the product package.  Needs neither torch nor libmmpc.so."""
import ctypes as C
import os
import shutil
import subprocess
import numpy as np

import emu_helper

_HERE = os.path.dirname(os.path.abspath(__file__))
_DIR = os.path.join(_HERE, "gpu_prim")
_SRC = os.path.join(_DIR, "mmpc_prim.hip")
_OPS = os.path.join(_DIR, "mmpc_prim_ops.h")
_CSRC = os.path.join(_HERE, "..", "mobile-manipulator-mpc_amd", "csrc")

WAVE = 64
# name: (id, doubles in, doubles out) - MMPC_PRIM_OPS of mmpc_prim_ops.h (checked against the library when it is loaded)
OPS = dict(rcp=(0, 1, 1), rcp3=(1, 1, 1), rcp_piv=(2, 1, 1), rsqrt=(3, 1, 1), sqrt_pair=(4, 1, 2), vmax=(5, 2, 1), vmin=(6, 2, 1),
           zsafe_fast=(7, 3, 1), zsafe=(8, 3, 1), powf=(9, 2, 1), mul24=(10, 2, 1), sincos=(11, 1, 2), arm=(12, 3, 6),
           arm_fast=(13, 3, 6), logacc=(14, 15, 2), self_row=(15, 7, 7), box_t=(16, 1, 1), max_err=(17, 2, 1), log_mant=(18, 1, 2))
LOGACC_K = 14
# rows of a cross-lane item (MMPC_PRIM_LANE_* of mmpc_prim_ops.h)
LANE_READLANE, LANE_ROWBCAST, LANE_RBALL9, LANE_RBALL6, LANE_DPP, LANE_XOR16, LANE_LOWER16, LANE_XOR32, LANE_ROWS = 0, 64, 80, 89, 95, 99, 100, 101, 102
RED_ROWS = 7   # wave_sum, wave_max, wave_min, gwave_sum, gwave_max, gwave_min, gwave_maxerr


def hipcc():
    """path of hipcc, or None"""
    h = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return h if os.path.exists(h) else shutil.which("hipcc")


def build(defs=(), force=False):
    """hipcc --offload-arch=gfx950 (the flags of the product's build.py) -> tests/gpu_prim/_build/libmmpc_prim<tag>.so;
    cross-compiles without a GPU.  defs: extra -D switches of the kernel headers (MMPC_RCP_NEWTON=1, ...): a library per set"""
    tag = ("_" + "_".join(d.replace("=", "") for d in defs)) if defs else ""
    out = os.path.join(_DIR, "_build", "libmmpc_prim%s.so" % tag)
    deps = [_SRC, _OPS] + [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith((".h", ".inc"))]
    newest = max(os.path.getmtime(f) for f in deps)
    if force or not os.path.exists(out) or os.path.getmtime(out) < newest:
        cc = hipcc()
        if cc is None:
            raise RuntimeError("no hipcc")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call([cc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-mllvm", "-amdgpu-mfma-vgpr-form", "-fPIC", "-shared",
                               *["-D" + d for d in defs], "-o", out, _SRC])
    return out


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


_FAILED = []   # the first launcher that returned an error: nothing is launched after it (a faulted GPU is left alone)


def _checked(prefix, name, rc):
    if rc != 0:
        _FAILED.append("%s%s: error %d" % (prefix, name, rc))
        raise AssertionError(_FAILED[0])


class _Lib:
    """the entry points under one prefix: 'mmpc_prim_' (device library) or 'mmpc_emu_prim_' (host emulation build)"""

    def __init__(self, path, prefix):
        self.lib = C.CDLL(path)
        self.prefix = prefix
        nin, nout = C.c_int(), C.c_int()
        for name, (op, ni, no) in OPS.items():
            assert self._f("op_shape")(op, C.byref(nin), C.byref(nout)) == 0 and (nin.value, nout.value) == (ni, no), name

    def _f(self, name):
        assert not _FAILED, "not launched after " + _FAILED[0]
        return getattr(self.lib, self.prefix + name)

    def switches(self):
        """bit 0: MMPC_RCP_NEWTON, bit 1: MMPC_PIV_NEWTON of this build (device library only)"""
        return self._f("switches")()

    def map(self, name, *cols):
        """scalar function `name` on n items; cols: its arguments, each a scalar or an array of n.  Returns (n, nout),
        or (n,) for one output"""
        op, nin, nout = OPS[name]
        assert len(cols) == nin, (name, len(cols), nin)
        a = np.ascontiguousarray(np.stack(np.broadcast_arrays(*[np.asarray(c, float) for c in cols]), axis=-1).reshape(-1, nin))
        n = a.shape[0]
        out = np.full((n, nout), np.nan)
        _checked(self.prefix, name, self._f("map")(op, n, _p(a), _p(out)))
        return out[:, 0] if nout == 1 else out

    def _vec(self, fn, v, rows_in, rows_out):
        v = np.ascontiguousarray(v, float).reshape(-1, rows_in, WAVE) if rows_in > 1 else np.ascontiguousarray(v, float).reshape(-1, WAVE)
        n = v.shape[0]
        out = np.full((n, rows_out, WAVE), np.nan)
        _checked(self.prefix, fn, self._f(fn)(n, _p(v), _p(out)))
        return out

    def lanes(self, v):
        """(nvec, 64) -> (nvec, LANE_ROWS, 64): every exchange, every lane's result"""
        return self._vec("lanes", v, 1, LANE_ROWS)

    def red(self, v):
        """(nvec, 64) -> (nvec, RED_ROWS, 64)"""
        return self._vec("red", v, 1, RED_ROWS)

    def red4(self, v):
        """(nvec, 4, 64): a, b, c, d -> (nvec, 8, 64): out[0..3] of the four-way sum, then of the four-way maximum"""
        return self._vec("red4", v, 4, 8)

    def mfma(self, v):
        """(nvec, 6, 64): a, b, c[0..3] per lane -> (nvec, 8, 64): the registers after MMPC_MFMA0(a, b), after MMPC_MFMA(c; a, b)"""
        return self._vec("mfma", v, 6, 8)

    def chain(self, v):
        """(nvec, 8, 64): registers of S, of D -> (nvec, 8, 64): sum_r MFMA(A = S[r], B = D[r]), sum_r MFMA(A = D[r], B = S[r])"""
        return self._vec("chain", v, 8, 8)


def device(defs=()):
    return _Lib(build(defs), "mmpc_prim_")


def host(defs=()):
    return _Lib(emu_helper.build(defs=defs), "mmpc_emu_prim_")


# ---- the lane <-> element map of v_mfma_f64_16x16x4_f64 as mmpc_tile.h states it
_L = np.arange(WAVE)


def tile_pack(A, B, Cm=None):
    """A (16, 4), B (4, 16), C (16, 16) -> the (6, 64) item of mfma(): lane l supplies A[l & 15][l >> 4] and B[l >> 4][l & 15]
    and holds C[(l >> 4) + 4 r][l & 15] in register r"""
    it = np.zeros((6, WAVE))
    it[0] = np.asarray(A, float)[_L & 15, _L >> 4]
    it[1] = np.asarray(B, float)[_L >> 4, _L & 15]
    if Cm is not None:
        it[2:6] = acc_pack(Cm)
    return it


def acc_pack(Cm):
    """(16, 16) -> registers (4, 64)"""
    Cm = np.asarray(Cm, float)
    return np.stack([Cm[(_L >> 4) + 4 * r, _L & 15] for r in range(4)])


def acc_unpack(regs):
    """registers (4, 64) -> (16, 16)"""
    D = np.zeros((16, 16))
    for r in range(4):
        D[(_L >> 4) + 4 * r, _L & 15] = regs[r]
    return D
