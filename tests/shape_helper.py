"""Inputs, references and the host-emulation driver of the shape-library tests (tests/emu_shapes/mmpc_emu_shapes.cpp).
TEST ONLY: builds with g++ -DMMPC_EMU; never used by the product package.

A shape library holds the specialised kernels of one (kind, N, M) outside the four built-in shapes.  The shapes below are the
smallest at which each code path of the specialised template differs; the emulation builds one host library per shape."""
import ctypes as C
import os
import subprocess

import numpy as np

import emu_helper
from oracle import nlp, coracle, synth

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "emu_shapes", "mmpc_emu_shapes.cpp")
_CSRC = os.path.join(_HERE, "..", "mobile-manipulator-mpc_amd", "csrc")
_BUILD = os.path.join(_HERE, "emu_shapes", "_build")

# (kind, N, M): why
SHAPES = {
    (0, 5, 3): "plain pair map, N < NX",
    (0, 12, 4): "padded map, short",
    # (0, 21, 2) and (0, 22, .) are outside the envelope: the gain ring of the device roll-out does not fit the stage-matrix
    # extras there (MmpcFastEnvelope::RING_FITS, a static assertion of the template) - (0, 23, .) is the first slim whole-body horizon
    (0, 23, 2): "first slim horizon the template accepts",
    (0, 24, 6): "slim, circle rows spread over lane groups, padded map newly off",
    (0, 31, 8): "upper edge; 41 936 B of LDS, three problems per CU",
    (0, 20, 10): "more circle rows per lane than any listed shape",
    (1, 6, 1): "base kind",
    (1, 25, 4): "base kind, slim",
    (1, 55, 1): "base kind, upper edge: the longest roll-out the template unrolls",
}
SHAPE_LIST = list(SHAPES)
ASAN_SHAPES = [(0, 24, 6), (0, 5, 3)]
B_TEST = 32


def shape_id(s):
    return "%d-%d-%d" % tuple(s)


def build(shape, asan_main=False):
    """the host library of one shape; asan_main: the stand-alone sanitized program (its own main) instead"""
    k, n, m = shape
    out = os.path.join(_BUILD, ("mmpc_emu_shape_asan_%d_%d_%d" if asan_main else "libmmpc_emu_shape_%d_%d_%d.so") % (k, n, m))
    deps = [_SRC, emu_helper.POISON_H] + [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith((".h", ".inc"))]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in deps):
        os.makedirs(_BUILD, exist_ok=True)
        # (the sanitizers' runtimes linked into the program: it then runs under whatever the environment preloads, untouched)
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan",
                 "-static-libubsan", "-DMMPC_EMUSH_MAIN"] if asan_main \
            else ["-O2", "-fPIC", "-shared"]
        tmp = out + ".tmp.%d" % os.getpid()
        subprocess.check_call(["g++", "-std=c++17", "-Wno-unknown-pragmas", "-ffp-contract=off", *flags, "-DMMPC_EMUSH_KIND=%d" % k,
                               "-DMMPC_EMUSH_N=%d" % n, "-DMMPC_EMUSH_M=%d" % m, "-o", tmp, _SRC])
        os.replace(tmp, out)
    return out


def build_all(jobs=16):
    """every host library and the two sanitized programs, at most `jobs` compilers at a time"""
    from concurrent.futures import ThreadPoolExecutor
    work = [(s, False) for s in SHAPE_LIST] + [(s, True) for s in ASAN_SHAPES]
    with ThreadPoolExecutor(max(1, min(int(jobs), 16))) as ex:
        return list(ex.map(lambda w: build(*w), work))


_libs = {}


def lib(shape):
    shape = tuple(shape)
    if shape not in _libs:
        L = C.CDLL(build(shape))
        assert L.mmpc_emush_params_size() == C.sizeof(emu_helper.MmpcParams)
        _libs[shape] = L
    return _libs[shape]


def par_of(kind, N):
    return nlp.BaseParams(N=N) if kind == 1 else nlp.WholeBodyParams(N=N)


_inputs = {}


def inputs(shape, B=B_TEST):
    """synth.make_batch with the config id the existing tests use per kind (whole-body 3, base 2): dict(x_init [clipped], traj_ref,
    u_ref, u_last = 0, obs).  Computed once per shape and shared: treat as read-only."""
    key = (tuple(shape), B)
    if key not in _inputs:
        k, N, M = shape
        par = par_of(k, N)
        d = synth.make_batch(B, N=N, M=M, kind="base" if k == 1 else "wholebody", config_id=2 if k == 1 else 3)
        d = dict(x_init=nlp.clip_x_init(par, d["x_init"]) if k == 0 else d["x_init"], traj_ref=d["traj_ref"], u_ref=d["u_ref"],
                 u_last=np.zeros((B, N, par.nu)), obs=d["obs"])
        for v in d.values():
            v.setflags(write=False)
        _inputs[key] = (par, d)
    return _inputs[key]


_oracle = {}


def oracle(shape, B=B_TEST):
    """the C oracle's solve of inputs(shape, B), once per shape"""
    key = (tuple(shape), B)
    if key not in _oracle:
        par, d = inputs(shape, B)
        _oracle[key] = coracle.solve_batch(par, d["x_init"], d["traj_ref"], d["u_ref"], d["u_last"], d["obs"], nthreads=16, max_iter=2000)
    return _oracle[key]


_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_p = lambda a: a.ctypes.data_as(_dp) if a is not None else None
_i = lambda a: a.ctypes.data_as(_ip)


def solve(shape, par, d, obs=None, tick=None, mode=None, fast=True, reverse=False, budget=0, max_iter=2000):
    """One solve of the host emulation at `shape`: the specialised template (fast) or the generic kernel.  obs: (B, M, 3) static
    (mode 0), (B, N+1, M, 3) table (mode 1) or - with mode=2 - the record (B, M, 5) and `tick`.  budget > 0: budgeted launch,
    then one continuation without a budget, as the C ABI runs them.  Returns dict(X, U, s, status, iters, cost, err, launches)."""
    L = lib(shape)
    c = lambda a: np.ascontiguousarray(a, float)
    x_init, traj_ref, u_ref, u_last = c(d["x_init"]), c(d["traj_ref"]), c(d["u_ref"]), c(d["u_last"])
    obs = c(d["obs"] if obs is None else obs)
    if mode is None:
        mode = 1 if obs.ndim == 4 else 0
    kind, N, M = shape
    B, nx, nu = x_init.shape[0], par.nx, par.nu
    assert obs.shape == {0: (B, M, 3), 1: (B, N + 1, M, 3), 2: (B, M, 5)}[mode]
    prm = emu_helper.make_params(par, M, False, max_iter=max_iter)
    prm.obs_per_stage = mode
    tp = None
    if tick is not None:
        tick = np.ascontiguousarray(tick, np.int64)
        tp = tick.ctypes.data_as(C.POINTER(C.c_longlong))
    X = np.zeros((B, N + 1, nx)); U = np.zeros((B, N, nu)); s = np.zeros((B, N + 1))
    status = np.zeros(B, np.int32); iters = np.zeros(B, np.int32); cost = np.zeros(B); err = np.zeros(B)
    args = (kind, C.byref(prm), B, _p(x_init), _p(traj_ref), _p(u_ref), _p(u_last), _p(obs), tp, _p(X), _p(U), _p(s), _i(status), _i(iters),
            _p(cost), _p(err), int(reverse))
    launches = 1
    if not fast:
        assert L.mmpc_emush_solve(*args) == 0
    else:
        state = None
        if budget > 0:
            state = np.full((B, L.mmpc_emush_fast_state_doubles()), np.nan)
        assert L.mmpc_emush_solve_fast(*args, int(budget), _p(state), 0) == 0
        if budget > 0 and (status == 3).any():
            assert L.mmpc_emush_solve_fast(*args, 0, _p(state), 1) == 0
            launches += 1
    return dict(X=X, U=U, s=s, status=status, iters=iters, cost=cost, err=err, launches=launches)


_emu = {}


def emulated(shape, B=B_TEST, fast=True):
    """solve(shape, *inputs(shape, B)) in lane order, once per shape and kernel family"""
    key = (tuple(shape), B, fast)
    if key not in _emu:
        par, d = inputs(shape, B)
        _emu[key] = solve(shape, par, d, fast=fast)
    return _emu[key]


def fast_lds_bytes(shape, mode=0):
    return 8 * lib(shape).mmpc_emush_fast_lds_doubles(int(mode))


def generic_lds_bytes(shape, mode=0):
    return 8 * lib(shape).mmpc_emush_lds_doubles(int(mode))


def shape_ok(kind, N, M):
    """mmpc_fast_shape_ok as the host build evaluates it"""
    return bool(lib(SHAPE_LIST[0]).mmpc_emush_shape_ok(int(kind), int(N), int(M)))


def write_case(path, shape, B=2):
    """the case file of the sanitized program: int32 B | MmpcParams | x_init | traj_ref | u_ref | u_last | obs"""
    par, d = inputs(shape)
    prm = emu_helper.make_params(par, shape[2], False, max_iter=2000)
    with open(path, "wb") as f:
        f.write(np.int32(B).tobytes())
        f.write(bytes(prm))
        for k in ("x_init", "traj_ref", "u_ref", "u_last", "obs"):
            f.write(np.ascontiguousarray(d[k][:B], float).tobytes())
    return path


BIT_KEYS = ("X", "U", "s", "status", "iters", "cost")


def assert_bitwise(a, b, keys=BIT_KEYS, what="", rows=None):
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if rows is not None:
            x, y = x[rows], y[rows]
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), "%s: %s differs (max |diff| %g)" % (what, k, np.abs(x.astype(float) - y.astype(float)).max())


def max_dev(r, o):
    return tuple(float(np.abs(r[k] - o[k]).max()) for k in ("X", "U", "s"))


WRONG_TAG = 0x0123456789abcdef


def wrong_tag_library(mm):
    """a shape library of (0, 5, 3) compiled with another source tag than libmmpc.so's (what mmpc_load_shape_library must refuse);
    built once, by the entry point's build() - the test finds it there"""
    import sys
    b = sys.modules[mm.__name__ + ".build"]
    out = os.path.join(_BUILD, "libmmpc_shape_wrongtag_0_5_3.so")
    deps = [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith((".h", ".inc", ".hip"))]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in deps):
        assert b.source_tag() != WRONG_TAG
        b.build_shape_library(0, 5, 3, out=out, tag=WRONG_TAG)
    return out
