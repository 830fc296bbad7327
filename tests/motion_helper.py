"""Inputs and the host-emulation driver of the linear-motion obstacle tests (tests/emu_motion/mmpc_emu_motion.cpp).
TEST ONLY: builds with g++ -DMMPC_EMU; never used by the product package.

A motion input is the record (B, M, 5) = (c_x, c_y, r, v_x, v_y) plus a tick per instance; its table twin is the per-stage table
(B, N+1, M, 3) with centres c + v * ((tick + k) * dt), built here in numpy - every operation rounded on its own, the definition
the fleet tests hold the tick kernel to."""
import ctypes as C
import os
import subprocess

import numpy as np

import emu_helper

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "emu_motion", "mmpc_emu_motion.cpp")
_CSRC = os.path.join(_HERE, "..", "mobile-manipulator-mpc_amd", "csrc")

# ticks of a batch: 0, small ones, and counts beyond 2^31 (the kernels form (double)tick + (double)k)
TICKS = np.array([0, 1, 7, 2 ** 31 + 5, 3, 250, 2 ** 31 + 77, 12], np.int64)


def build(asan=False):
    out = os.path.join(_HERE, "emu_motion", "_build", "libmmpc_emu_motion_asan.so" if asan else "libmmpc_emu_motion.so")
    deps = [_SRC, emu_helper.POISON_H] + [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith((".h", ".inc"))]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-DMMPC_EMUM_SHAPES(X)=X(0, 30, 8)"] if asan else ["-O2"]
        subprocess.check_call(["g++", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-ffp-contract=off", *flags, "-o", out, _SRC])
    return out


def ticks(B):
    return np.resize(TICKS, B).astype(np.int64)


def record(obs, vel):
    """(B, M, 3) centres + radius and (B, M, 2) velocities -> the motion record (B, M, 5)"""
    return np.ascontiguousarray(np.concatenate([obs, vel], axis=2))


def table_twin(rec, tick, N, dt):
    """the per-stage table the record and the ticks stand for: c + v * ((tick + k) * dt)"""
    B, M = rec.shape[:2]
    t = (tick[:, None] + np.arange(N + 1, dtype=np.int64)[None, :]).astype(np.float64) * dt           # (B, N+1)
    tab = np.empty((B, N + 1, M, 3))
    tab[..., 0] = rec[:, None, :, 0] + rec[:, None, :, 3] * t[:, :, None]
    tab[..., 1] = rec[:, None, :, 1] + rec[:, None, :, 4] * t[:, :, None]
    tab[..., 2] = rec[:, None, :, 2]
    return tab


def scale_velocities(rec, tick, dt, reach=1.5):
    """Velocities scaled per instance so that an obstacle moves at most `reach` metres from its record position until the end of
    ITS horizon (a tick of 2^31 at 0.5 m/s is 1e8 m away: no obstacle left to avoid).  Signs are kept: some stay negative."""
    rec = rec.copy()
    t_end = (tick.astype(np.float64) + 64.0) * dt
    vmax = np.abs(rec[..., 3:]).max(axis=(1, 2))
    f = np.minimum(1.0, reach / np.maximum(vmax * t_end, 1e-300))
    rec[..., 3:] *= f[:, None, None]
    return rec


def motion_inputs(B, N, M, kind="wholebody", dt=0.1, config_id=5, seed=20240114):
    """synth.make_batch(..., moving=True) as a motion input: dict(x_init, traj_ref, u_ref, rec, tick) with per-instance ticks; the
    obstacles are moved back so that at the instance's tick they are where the generator put them."""
    from oracle import synth
    d = synth.make_batch(B, N=N, M=M, kind=kind, config_id=config_id, moving=True, dt=dt, seed=seed)
    tick = ticks(B)
    rec = scale_velocities(record(d["obs"], d["obs_vel"]), tick, dt)
    rec[..., :2] -= rec[..., 3:] * (tick.astype(np.float64) * dt)[:, None, None]
    return dict(x_init=d["x_init"], traj_ref=d["traj_ref"], u_ref=d["u_ref"], rec=np.ascontiguousarray(rec), tick=tick)


def kind_id(par):
    return (2 if getattr(par, "pose_ref", False) else 0) if par.kind == "wholebody" else 1


_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_p = lambda a: a.ctypes.data_as(_dp) if a is not None else None
_i = lambda a: a.ctypes.data_as(_ip)


def solve(par, x_init, traj_ref, u_ref, u_last, obs, tick=None, mode=None, fast=False, reverse=False, asan=False, budget=0, max_iter=200):
    """One solve of the host emulation.  obs: (B, M, 3) static (mode 0), (B, N+1, M, 3) table (mode 1) or - with mode=2 - the record
    (B, M, 5) and `tick` (B,) int64 or None.  budget > 0 (specialised kernels): budgeted launch, then continuations without a
    budget until nobody is suspended, as the C ABI runs them.  Returns dict(X, U, s, status, iters, cost, err, launches)."""
    lib = C.CDLL(build(asan))
    assert lib.mmpc_emum_params_size() == C.sizeof(emu_helper.MmpcParams)
    c = lambda a: np.ascontiguousarray(a, float)
    x_init, traj_ref, u_ref, u_last, obs = c(x_init), c(traj_ref), c(u_ref), c(u_last), c(obs)
    if mode is None:
        mode = 1 if obs.ndim == 4 else 0
    B, N, nx, nu, M = x_init.shape[0], par.N, par.nx, par.nu, obs.shape[-2]
    assert obs.shape == {0: (B, M, 3), 1: (B, N + 1, M, 3), 2: (B, M, 5)}[mode]
    prm = emu_helper.make_params(par, M, False, max_iter=max_iter)
    prm.obs_per_stage = mode
    if tick is not None:
        tick = np.ascontiguousarray(tick, np.int64)
        assert tick.shape == (B,)
    tp = tick.ctypes.data_as(C.POINTER(C.c_longlong)) if tick is not None else None
    X = np.zeros((B, N + 1, nx)); U = np.zeros((B, N, nu)); s = np.zeros((B, N + 1))
    status = np.zeros(B, np.int32); iters = np.zeros(B, np.int32); cost = np.zeros(B); err = np.zeros(B)
    kind = kind_id(par)
    launches = 1
    if not fast:
        rc = lib.mmpc_emum_solve(kind, C.byref(prm), B, _p(x_init), _p(traj_ref), _p(u_ref), _p(u_last), _p(obs), tp, _p(X), _p(U), _p(s),
                                 _i(status), _i(iters), _p(cost), _p(err), int(reverse))
        assert rc == 0
    else:
        state = None
        if budget > 0:
            sd = lib.mmpc_emum_fast_state_doubles(kind, N, M)
            assert sd > 0
            state = np.full((B, sd), np.nan)
        args = (kind, C.byref(prm), B, _p(x_init), _p(traj_ref), _p(u_ref), _p(u_last), _p(obs), tp, _p(X), _p(U), _p(s),
                _i(status), _i(iters), _p(cost), _p(err), int(reverse))
        rc = lib.mmpc_emum_solve_fast(*args, int(budget), _p(state), 0)
        if rc != 0:
            raise RuntimeError("no specialised instantiation for this configuration")
        if budget > 0 and (status == 3).any():
            assert lib.mmpc_emum_solve_fast(*args, 0, _p(state), 1) == 0
            launches += 1
    return dict(X=X, U=U, s=s, status=status, iters=iters, cost=cost, err=err, launches=launches)


def fast_lds_doubles(kind, N, M, mode):
    return C.CDLL(build()).mmpc_emum_fast_lds_doubles(int(kind), int(N), int(M), int(mode))


def lds_doubles(kind, N, M, mode):
    return C.CDLL(build()).mmpc_emum_lds_doubles(int(kind), int(N), int(M), int(mode))


def centres(c, v, tick, dt, n):
    a = np.zeros(n); b = np.zeros(n)
    fn = C.CDLL(build()).mmpc_emum_centres
    fn.argtypes = [C.c_double, C.c_double, C.c_longlong, C.c_double, C.c_int, _dp, _dp]
    fn(float(c), float(v), int(tick), float(dt), int(n), _p(a), _p(b))
    return a, b


OUT_KEYS = ("X", "U", "s", "status", "iters", "cost")


def assert_bitwise(a, b, keys=OUT_KEYS, what=""):
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), "%s: %s differs (max |diff| %g)" % (what, k, np.abs(x.astype(float) - y.astype(float)).max())
