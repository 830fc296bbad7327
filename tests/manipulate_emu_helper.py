"""ctypes driver for the host build of the fleet manipulate kernel (tests/manipulate_emu/mmpc_manipulate_emu.cpp), the numpy
definition of what that kernel computes, and the inputs the CPU and the GPU tests share.  TEST ONLY: never used by the product package."""
import ctypes as C
import os
import subprocess

import numpy as np

import tick_emu_helper as TH

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "manipulate_emu", "mmpc_manipulate_emu.cpp")
_CSRC = os.path.join(_HERE, "..", "mobile-manipulator-mpc_amd", "csrc")
_DEPS = [_SRC, os.path.join(_HERE, "emu_common", "mmpc_emu_poison.h"), os.path.join(_HERE, "..", "include", "mmpc.h")] + [os.path.join(_CSRC, f) for f in ("mmpc_manipulate.h", "mmpc_ik.h", "mmpc_tick.h", "mmpc_core.h", "mmpc_tile.h")]

DONE, MANIPULATE, MANIP_DONE = 3, 4, 5
BX, BZ = -0.007, 0.606 + 0.333
Q_LO, Q_HI = np.array([-np.pi / 2, -3 * np.pi / 4, 0.0]), np.array([np.pi / 2, 0.0, 3 * np.pi / 2])
OUTPUTS = ("x_in", "traj_ref", "start", "obs")


def build():
    out = os.path.join(_HERE, "manipulate_emu", "_build", "libmmpc_manipulate_emu.so")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in _DEPS):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", out, _SRC])
    return out


_p = TH._p


def prepare(N, M, dt, xlim, x, tick, phase, pose, nplan, U_prev=None, plan=None, obs0=None, vel=None, want=OUTPUTS, reverse=False):
    """The kernel on the host.  x (B,9), tick (B,), phase (B,) and plan (B,nplan,9) are NOT modified: the new ones come back as "x",
    "tick", "phase" and "plan" beside the outputs named in `want`, "qgoal" (B,3), "ik_status" (B,), "list" (B,) and "counts" (2,).
    Every output, and the plan when none is given, starts at the sentinel -7."""
    lib = C.CDLL(build())
    B = x.shape[0]
    c = lambda a, t=np.float64: None if a is None else np.ascontiguousarray(a, t)
    x = np.array(x, np.float64, order="C"); tick = np.array(tick, np.int64, order="C"); phase = np.array(phase, np.int32, order="C")
    plan = np.full((B, nplan, 9), -7.0) if plan is None else np.array(plan, np.float64, order="C")
    U_prev, pose, obs0, vel = c(U_prev), c(pose), c(obs0), c(vel)
    out = dict(x_in=np.full((B, 9), -7.0), traj_ref=np.full((B, N + 1, 9), -7.0), start=np.full(B, -7, np.int32), obs=np.full((B, N + 1, M, 3), -7.0))
    qgoal, ik_status = np.full((B, 3), -7.0), np.full(B, -7, np.int32)
    lst, counts = np.full(B, -7, np.int32), np.full(2, -7, np.int32)
    g = lambda k: out[k] if k in want else None
    xl = np.ascontiguousarray(xlim, np.float64)
    assert xl.shape == (2, 9) and pose.shape == (B, 4) and plan.shape == (B, nplan, 9)
    rc = lib.mmpc_manipulate_emu_prepare(C.c_int(N), C.c_int(M), C.c_double(dt), _p(xl), C.c_int(B), _p(x), _p(tick, C.c_longlong), _p(phase, C.c_int),
                                         _p(U_prev), _p(pose), C.c_int(nplan), _p(plan), _p(qgoal), _p(ik_status, C.c_int), _p(obs0), _p(vel),
                                         _p(g("x_in")), _p(g("traj_ref")), _p(g("start"), C.c_int), _p(g("obs")), _p(lst, C.c_int), _p(counts, C.c_int),
                                         C.c_int(int(reverse)))
    assert rc == 0
    res = {k: v for k, v in out.items() if k in want}
    res.update(x=x, tick=tick, phase=phase, plan=plan, qgoal=qgoal, ik_status=ik_status, list=lst, counts=counts)
    return res


def endpoint(x):
    """the endpoint's world position as the host build's finish test forms it, (B,9) -> (B,3)"""
    lib = C.CDLL(build())
    x = np.ascontiguousarray(np.atleast_2d(x), np.float64)
    e = np.zeros((x.shape[0], 3))
    for b in range(x.shape[0]):
        lib.mmpc_manipulate_emu_endpoint(_p(x[b]), _p(e[b]))
    return e


def target(x, g):
    """the endpoint target in the arm frame as the host build's transition forms it, (B,9), (B,4) -> (B,2): tx, tz"""
    lib = C.CDLL(build())
    x, g = np.ascontiguousarray(np.atleast_2d(x), np.float64), np.ascontiguousarray(np.atleast_2d(g), np.float64)
    t = np.zeros((x.shape[0], 2))
    for b in range(x.shape[0]):
        lib.mmpc_manipulate_emu_target(_p(x[b]), _p(g[b]), _p(t[b]))
    return t


# ---- the numpy definition -------------------------------------------------------------------------------------------------------
def fk(mm, x):
    """the endpoint's world position by the package's forward_tranformation, as Interface.timerCallback forms current_joints_pose[:3]"""
    return np.asarray(mm.MobileManipulator(0.1).forward_tranformation(x)[0][:3], float)


def local_target(x, g):
    """the endpoint target in the arm frame (interface_wholebody_qref.py:206-210): (tx, tz)"""
    return np.array([np.sqrt((g[0] - x[0]) ** 2 + (g[1] - x[1]) ** 2) + 0.007, g[2] - (0.606 + 0.333)])


def quantities(mm, x, g):
    """what the finish test compares with zero, for one robot: |e - g| - 0.01"""
    return np.array([np.linalg.norm(fk(mm, x) - g[:3]) - 0.01])


def reference(mm, xlim, dt, N, x, tick, phase, pose, nplan, plan, q_goal, obs0, vel):
    """The manipulate tick AFTER the advance, in numpy: x (B,9) and tick (B,) are the advanced state, phase (B,) the phases on entry,
    plan (B,nplan,9) the plans on entry (read for the robots that come in at MANIPULATE), q_goal (B,3) the IK's answers (read for the
    robots that come in at DONE).  Rows of robots that are not in MANIPULATE after the call keep the sentinel -7."""
    from importlib import import_module
    iface = import_module(mm.__name__ + ".interface_wholebody_qref")
    B, M = x.shape[0], obs0.shape[1]
    r = dict(phase=np.array(phase, np.int32), plan=np.array(plan, float), x_in=np.full((B, 9), -7.0), traj_ref=np.full((B, N + 1, 9), -7.0),
             start=np.full(B, -7, np.int32), obs=np.full((B, N + 1, M, 3), -7.0), target=np.full((B, 2), -7.0), finish=np.zeros(B, bool))
    zero_u = np.zeros((1, nplan - 1, 5))
    for b in range(B):
        p = int(phase[b])
        if p not in (DONE, MANIPULATE):
            continue
        if p == DONE:
            r["target"][b] = local_target(x[b], pose[b])
            r["plan"][b] = np.linspace(x[b], np.hstack((x[b, :6], q_goal[b])), nplan)       # globalPlanManipulator (:284-293)
            p = MANIPULATE
        if np.linalg.norm(fk(mm, x[b]) - pose[b, :3]) <= 0.01:
            r["phase"][b], r["finish"][b] = MANIP_DONE, True
            continue
        r["phase"][b] = p
        r["x_in"][b] = np.clip(x[b], xlim[0], xlim[1])
        r["traj_ref"][b] = iface.calc_local_ref_traj(x[b], r["plan"][b][None], zero_u, N, [6, 7, 8])[0][0]
        r["start"][b] = np.argmin(np.linalg.norm(x[b, None, 6:] - r["plan"][b][:, 6:], axis=1))
        k = (tick[b] + np.arange(N + 1))[:, None, None] * dt
        o = np.repeat(obs0[b][None], N + 1, axis=0).copy()
        o[..., :2] += vel[b][None] * k
        r["obs"][b] = o
    r["rows"] = np.flatnonzero(r["phase"] == MANIPULATE)
    r["counts"] = np.array([(r["phase"] == MANIPULATE).sum(), (r["phase"] == MANIP_DONE).sum()], np.int32)
    return r


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
BRANCHES = ("driving", "transition, reachable", "transition, out of reach", "transition->finish", "manipulate", "manipulate->finish", "finished")
_AFTER = (-1, MANIPULATE, MANIPULATE, MANIP_DONE, MANIPULATE, MANIP_DONE, MANIP_DONE)


def _arm(q):
    """reach and height of the endpoint in the arm frame"""
    from oracle import nlp
    e = nlp.arm_fk(q)[0]
    return float(e[0]), float(e[2])


def _world(x):
    r, z = _arm(x[6:])
    return np.array([x[0] + (r + BX) * np.cos(x[2]), x[1] + (r + BX) * np.sin(x[2]), z + BZ])


def branch_inputs(B=448, N=20, M=3, nplan=21, seed=4):
    """Robot b is drawn for branch b % 7 of BRANCHES: its entry phase, where its endpoint is relative to its pose target, and - for a
    robot that comes in at MANIPULATE - its plan and where on it the arm is (even rounds of the branch in the middle of the plan, odd
    ones within the last three rows).  A robot in the manipulate phase is nearly at rest and its previous optimum is small, so that
    the branch is the same with and without the advance.  Returns the kernel's inputs and "branch" (B,)."""
    rng = np.random.default_rng(seed)
    br = np.arange(B) % len(BRANCHES)
    x = np.zeros((B, 9))
    x[:, :2] = rng.uniform(-5, 5, (B, 2))
    x[:, 2] = rng.uniform(-3.5, 3.5, B)
    x[:, 3:6] = rng.uniform(-1e-3, 1e-3, (B, 3))
    phase = np.zeros(B, np.int32)
    pose = np.zeros((B, 4))
    plan = np.full((B, nplan, 9), -7.0)
    U_prev = rng.uniform(-1, 1, (B, N, 5))
    unit = lambda: (lambda v: v / np.linalg.norm(v))(rng.normal(size=3))
    for b in range(B):
        k = br[b]
        while True:
            q = rng.uniform(Q_LO + 0.1, Q_HI - 0.1)
            if _arm(q)[0] > 0.2:
                break
        x[b, 6:] = q
        pose[b, 3] = x[b, 2]
        if k == 0:
            phase[b] = rng.integers(0, 3)
            x[b, 3:6] = rng.uniform(-1.5, 1.5, 3)
            pose[b, :3] = _world(x[b]) + rng.uniform(-0.5, 0.5, 3)
        elif k == 1:        # a target another arm configuration reaches, away from where the endpoint is
            phase[b] = DONE
            while True:
                qt = rng.uniform(Q_LO + 0.1, Q_HI - 0.1)
                pose[b, :3] = _world(np.hstack((x[b, :6], qt)))
                if _arm(qt)[0] > 0.2 and np.linalg.norm(pose[b, :3] - _world(x[b])) > 0.05:
                    break
        elif k == 2:        # far beyond the arm's 0.86 m: the minimiser (arm stretched towards the target) is the sharper the farther
            # the target is - curvature about 0.2 (d - 0.86) along the last joint -, and the oracle the IK is compared with stops at a
            # stationarity of 1e-8, not at a distance to the minimiser
            phase[b] = DONE
            d, h = rng.uniform(3.0, 5.0), rng.uniform(0.2, 1.2)
            pose[b, :3] = [x[b, 0] + d * np.cos(x[b, 2]), x[b, 1] + d * np.sin(x[b, 2]), BZ + h]
        elif k == 3:        # the endpoint is there already
            phase[b] = DONE
            pose[b, :3] = _world(x[b]) + rng.uniform(0.0005, 0.005) * unit()
        elif k in (4, 5):
            phase[b] = MANIPULATE
            U_prev[b] *= 1e-3 if k == 5 else 2e-2
            while True:
                s, t = x[b].copy(), x[b].copy()
                s[6:], t[6:] = rng.uniform(Q_LO + 0.1, Q_HI - 0.1), rng.uniform(Q_LO + 0.1, Q_HI - 0.1)
                if np.abs(t[6:] - s[6:]).min() < 0.05:
                    continue
                pl = np.linspace(s, t, nplan)
                row = max(0, nplan - 1 - int(rng.integers(0, 3))) if (b // len(BRANCHES)) % 2 else int(rng.integers(nplan // 3, 2 * nplan // 3))
                qx = pl[row, 6:] + rng.uniform(-0.3, 0.3, 3) * (t[6:] - s[6:]) / (nplan - 1)
                xb = np.hstack((x[b, :6], qx))
                tgt = _world(t) + rng.uniform(0.03, 0.08) * unit() if k == 4 else _world(xb) + rng.uniform(0.002, 0.005) * unit()
                if k == 5 or np.linalg.norm(_world(xb) - tgt) > 0.03:
                    break
            plan[b], x[b], pose[b, :3] = pl, xb, tgt
        else:
            phase[b] = MANIP_DONE
            x[b, 3:6] = rng.uniform(-1.5, 1.5, 3)
            pose[b, :3] = _world(x[b]) + rng.uniform(-0.5, 0.5, 3)
    obs0 = np.concatenate([rng.uniform(-8, 8, (B, M, 2)), rng.uniform(0.2, 0.6, (B, M, 1))], axis=2)
    vel = rng.uniform(-0.3, 0.3, (B, M, 2))
    tick = rng.integers(0, 40, B).astype(np.int64)
    return dict(x=x, tick=tick, phase=phase, pose=pose, nplan=nplan, U_prev=U_prev, plan=plan, obs0=np.ascontiguousarray(obs0), vel=vel), br


def expected_after(branch, phase_in):
    """the phase after the call: the branch's, a driving robot's own"""
    a = np.array(_AFTER, np.int32)[branch]
    return np.where(a < 0, phase_in, a).astype(np.int32)
