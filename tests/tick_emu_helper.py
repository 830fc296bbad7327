"""ctypes driver for the host build of the fleet tick kernel (tests/tick_emu/mmpc_tick_emu.cpp) and the inputs and numpy
definitions the CPU and the GPU tests of that kernel share.  TEST ONLY: never used by the product package."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "tick_emu", "mmpc_tick_emu.cpp")
_CSRC = os.path.join(_HERE, "..", "mobile-manipulator-mpc_amd", "csrc")
_DEPS = [_SRC, os.path.join(_HERE, "emu_common", "mmpc_emu_poison.h")] + [os.path.join(_CSRC, f) for f in ("mmpc_tick.h", "mmpc_core.h", "mmpc_tile.h")]


def build():
    out = os.path.join(_HERE, "tick_emu", "_build", "libmmpc_tick_emu.so")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in _DEPS):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", out, _SRC])
    return out


def _p(a, t=C.c_double):
    return a.ctypes.data_as(C.POINTER(t)) if a is not None else None


def prepare(N, M, dt, xlim, x, tick, U_prev=None, glob=None, obs0=None, vel=None, want=("x_in", "traj_ref", "start", "obs", "u_guess", "x_guess"),
            reverse=False):
    """The kernel on the host.  x (B,9) and tick (B,) are NOT modified: the advanced copies come back as "x" and "tick" beside
    the outputs named in `want`."""
    lib = C.CDLL(build())
    B = x.shape[0]
    c = lambda a, t=np.float64: None if a is None else np.ascontiguousarray(a, t)
    x = np.array(x, np.float64, order="C"); tick = np.array(tick, np.int64, order="C")
    U_prev, glob, obs0, vel = c(U_prev), c(glob), c(obs0), c(vel)
    out = dict(x_in=np.full((B, 9), -7.0), traj_ref=np.full((B, N + 1, 9), -7.0), start=np.full(B, -7, np.int32),
               obs=np.full((B, N + 1, M, 3), -7.0), u_guess=np.full((B, N, 5), -7.0), x_guess=np.full((B, N + 1, 9), -7.0))
    g = lambda k: out[k] if k in want else None
    xl = np.ascontiguousarray(xlim, np.float64)
    assert xl.shape == (2, 9)
    rc = lib.mmpc_tick_emu_prepare(C.c_int(N), C.c_int(M), C.c_double(dt), _p(xl), C.c_int(B), _p(x), _p(tick, C.c_longlong), _p(U_prev), _p(glob),
                                   C.c_int(0 if glob is None else glob.shape[1]), _p(obs0), _p(vel), _p(g("x_in")), _p(g("traj_ref")),
                                   _p(g("start"), C.c_int), _p(g("obs")), _p(g("u_guess")), _p(g("x_guess")), C.c_int(int(reverse)))
    assert rc == 0
    res = {k: v for k, v in out.items() if k in want}
    res["x"], res["tick"] = x, tick
    return res


def straight_plan(traj_ref, N, rows=51):
    """The `rows`-row straight-line global plan through the first N + 1 reference rows of a synthetic batch (as the fleet tests
    and the benchmark build it)."""
    step = (traj_ref[:, N] - traj_ref[:, 0]) / N
    return np.ascontiguousarray(traj_ref[:, :1] + step[:, None, :] * np.arange(rows, dtype=np.float64)[None, :, None])


def fleet_inputs(B=1024, N=30, M=8, seed=7):
    """The inputs of the kernel tests: C5's obstacle field and plans, robots scattered around their plans."""
    from oracle import synth
    d = synth.make_batch(B, N=N, M=M, config_id=5, moving=True)
    glob = straight_plan(d["traj_ref"], N)
    rng = np.random.default_rng(seed)
    x = np.zeros((B, 9))
    row = rng.integers(0, glob.shape[1], B)
    x[:, :2] = glob[np.arange(B), row, :2] + rng.uniform(-0.3, 0.3, (B, 2))
    x[:, 2] = rng.uniform(-3.5, 3.5, B)
    x[:, 3:6] = rng.uniform(-1.5, 1.5, (B, 3))
    x[:, 6:] = d["x_init"][:, 6:]
    U_prev = rng.uniform(-1, 1, (B, N, 5))
    tick = rng.integers(0, 40, B).astype(np.int64)
    return dict(x=x, tick=tick, U_prev=U_prev, glob=glob, obs0=np.ascontiguousarray(d["obs"]), vel=np.ascontiguousarray(d["obs_vel"]))


def ulp_err(a, ref):
    """|a - ref| in units of the spacing of doubles at max(1, |ref|), per component"""
    return np.abs(a - ref) / np.spacing(np.maximum(1.0, np.abs(ref)))


def reference(mm, xlim, dt, N, x, tick, U_prev, glob, obs0, vel):
    """The definitions the kernel replaces, in numpy: f_kinematics of the package's robot model on the clipped state, np.clip,
    calc_local_ref_traj from the advanced position, the expression of BatchedRecedingHorizon.obstacles_now with per-robot ticks,
    the shift of the previous optimum."""
    from importlib import import_module
    iface = import_module(mm.__name__ + ".interface_wholebody_qref")
    robot = mm.MobileManipulator(dt)
    B = x.shape[0]
    r = {}
    if U_prev is not None:
        xc = np.clip(x, xlim[0], xlim[1])
        r["x"] = np.array([robot.f_kinematics(xc[b], U_prev[b, 0]) for b in range(B)])
        r["tick"] = tick + 1
        r["u_guess"] = np.concatenate([U_prev[:, 1:], U_prev[:, -1:]], axis=1)
    else:
        r["x"], r["tick"] = x.copy(), tick.copy()
    r["x_in"] = np.clip(r["x"], xlim[0], xlim[1])
    dist = np.linalg.norm(r["x"][:, None, :2] - glob[:, :, :2], axis=2)
    r["dist"] = dist
    r["start"] = np.argmin(dist, axis=1)
    r["traj_ref"], _ = iface.calc_local_ref_traj(r["x"], glob, np.zeros((B, glob.shape[1] - 1, 5)), N)
    k = (r["tick"][:, None] + np.arange(N + 1)[None, :])[:, :, None, None] * dt
    o = np.repeat(obs0[:, None, :, :], N + 1, axis=1).copy()
    o[..., :2] += vel[:, None, :, :] * k
    r["obs"] = o
    return r


def rollout_err(mm, dt, u_guess, x_guess):
    """max ulp_err of x_guess[k + 1] against f_kinematics applied to the build's OWN x_guess[k], u_guess[k], over all k"""
    robot = mm.MobileManipulator(dt)
    B, N = u_guess.shape[:2]
    worst = 0.0
    for k in range(N):
        ref = np.array([robot.f_kinematics(x_guess[b, k], u_guess[b, k]) for b in range(B)])
        worst = max(worst, float(ulp_err(x_guess[:, k + 1], ref).max()))
    return worst
