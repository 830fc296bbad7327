"""What a solve of a host build starts on (tests/emu_common/mmpc_emu_poison.h), from Python: the fill of the LDS slab, the gain
block and the correction scratch, and the byte pattern written over the lane state at the entry of every solve.
TEST ONLY: never used by the product package.

The setting is a static of each host library and outlives the call, so it is only ever set through `poisoned`, which puts the
default (NaN slab, lane state left alone) back on the way out - a test that raises does not change what the next one runs on."""
import contextlib
import ctypes as C

# the header's enum, in its order
MODES = ("nan", "keep", "noise", "+1e300", "-1e300", "+inf", "-inf", "0", "1e-310")
LANE_PATTERNS = (0x00, 0x43, 0x7F, 0xFF)      # 0x43...: a finite double of 1e16; 0x7F...: a NaN with a finite upper half; 0xFF...: -NaN, int -1
SEED = 20240114


def _lib(lib):
    lib = C.CDLL(lib) if isinstance(lib, str) else lib
    lib.mmpc_emu_poison_set.argtypes = [C.c_int, C.c_ulonglong, C.c_int]
    lib.mmpc_emu_poison_set.restype = C.c_int
    lib.mmpc_emu_poison_fill.argtypes = [C.POINTER(C.c_double), C.c_longlong]
    lib.mmpc_emu_poison_fill.restype = None
    return lib


@contextlib.contextmanager
def poisoned(lib, mode="nan", lane=-1, seed=SEED):
    """lib: a host library (its path or its CDLL).  mode: one of MODES; lane: -1 (leave the lane state alone) or a byte"""
    lib = _lib(lib)
    assert lib.mmpc_emu_poison_set(MODES.index(mode), seed, int(lane)) == 0
    try:
        yield lib
    finally:
        assert lib.mmpc_emu_poison_set(0, 0, -1) == 0


def fill(lib, a):
    """a float64 array of the test's own (a save area) filled by the library's current mode"""
    assert a.dtype == "float64" and a.flags.c_contiguous
    _lib(lib).mmpc_emu_poison_fill(a.ctypes.data_as(C.POINTER(C.c_double)), a.size)
    return a
