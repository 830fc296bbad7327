"""CPU: the fleet manipulate kernel (csrc/mmpc_manipulate.h) built for the host (g++ -DMMPC_EMU -ffp-contract=off,
tests/manipulate_emu) against a numpy definition of the manipulate tick, that definition against the package's port of the
reference's state machine (Interface on the CPU oracle, driven to 'manipulate finish'), and the resource usage of the kernel's
gfx950 code object.

Bounds.  The numpy definition is evaluated at the build's own advanced state and own q_goal, so everything it is compared in
consists of copies, comparisons and correctly rounded IEEE operations in the same order on both sides: bitwise (the plan: the
kernel's (j / T) (target - start) + start is np.linspace whenever a column has zero difference, and columns 0..5 always have).  The
advance is the mission host build's on the same rows, bitwise.  The endpoint of the finish test differs from the package's
forward_tranformation in sin / cos and in the order of the segment sums: <= 4 ulp of max(1, |e_i|), the plant step's bound in
tests/test_fleet_tick_cpu.py.  A comparison with a threshold can only come out differently on the two sides when its operands are a
rounding error apart, so the inputs are required to keep the finish quantity at least 1e-9 from zero and the two nearest plan rows
at least 1e-9 apart in distance.  The IK's answer is held to 1e-8 against the per-lane host build and the oracle, the tolerance of
tests/test_ik.py; the target it is solved for is within 1 ulp of Interface's (np.hypot there, sqrt(dx dx + dy dy) here)."""
import contextlib
import io
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import ik, nlp
from tests import emu_helper, oracle_engine

import manipulate_emu_helper as H
import mission_emu_helper as MH
import tick_emu_helper as TH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, M, DT = 20, 3, 0.1
KEYS = ("x_in", "traj_ref", "start", "obs")


def _xlim():
    return np.asarray(nlp.WholeBodyParams(N=N).xlim, float)


def _check_against_numpy(r, ref):
    """every output of one call `r` against the numpy definition `ref` at r's own advanced state and q_goal"""
    assert np.array_equal(r["phase"], ref["phase"])
    for k in ("plan",) + KEYS:
        assert np.array_equal(r[k], ref[k]), k
    assert np.array_equal(r["counts"], ref["counts"])
    n = int(r["counts"][0])
    assert np.array_equal(np.sort(r["list"][:n]), ref["rows"])
    assert (r["list"][n:] == -7).all()


def _input_condition(mm, x, pose, phase_after, plan):
    """the finish quantity of every robot the kernel tests, and the two nearest plan rows of every robot it lists"""
    tested = np.flatnonzero(phase_after >= H.MANIPULATE)
    q = np.array([H.quantities(mm, x[b], pose[b]) for b in tested])
    assert float(np.abs(q).min()) >= 1e-9, float(np.abs(q).min())
    live = phase_after == H.MANIPULATE
    two = np.sort(np.linalg.norm(x[live, None, 6:] - plan[live][:, :, 6:], axis=2), axis=1)[:, :2]
    assert float((two[:, 1] - two[:, 0]).min()) >= 1e-9, float((two[:, 1] - two[:, 0]).min())


@pytest.mark.parametrize("nplan", [21, 41])
@pytest.mark.parametrize("advance", [True, False], ids=["advance", "no_advance"])
def test_host_build_against_numpy_definition(mm, advance, nplan):
    B = 448
    d, branch = H.branch_inputs(B, N, M, nplan)
    xlim = _xlim()
    if not advance:
        d = dict(d, U_prev=None)
    own = d["phase"] == H.MANIPULATE                 # the robots this kernel advances
    for reverse in (False, True):
        r = H.prepare(N, M, DT, xlim, reverse=reverse, **d)
        assert np.array_equal(r["x"][~own], d["x"][~own]) and np.array_equal(r["tick"][~own], d["tick"][~own])
        if advance:
            # the mission host build on the same rows, entered as moving robots far from any goal: its advance of a live robot
            far = np.zeros((int(own.sum()), 2, 9)); far[:, :, :2] = 1e3
            adv = MH.prepare(N, M, DT, xlim, d["x"][own], d["tick"][own], np.zeros(int(own.sum()), np.int32), d["U_prev"][own], far,
                             d["obs0"][own], d["vel"][own])
            assert np.array_equal(r["x"][own], adv["x"]) and np.array_equal(r["tick"][own], adv["tick"])
            assert np.array_equal(r["tick"][own], d["tick"][own] + 1) and not np.array_equal(r["x"][own], d["x"][own])
        else:
            assert np.array_equal(r["x"], d["x"]) and np.array_equal(r["tick"], d["tick"])
        ref = H.reference(mm, xlim, DT, N, r["x"], r["tick"], d["phase"], d["pose"], nplan, d["plan"], r["qgoal"], d["obs0"], d["vel"])
        _input_condition(mm, r["x"], d["pose"], ref["phase"], ref["plan"])
        # every branch is taken, by the robots drawn for it: the count below is of the robots DRAWN for a branch and means something
        # only with the line before it, that each of them ends in its branch's phase.  Branches 1 and 2 end in the same phase: a
        # reachable target and one out of reach are told apart by the IK's residual, in test_ik_at_the_transition
        assert np.array_equal(ref["phase"], H.expected_after(branch, d["phase"]))
        taken = np.bincount(branch, minlength=len(H.BRANCHES))
        print(dict(zip(H.BRANCHES, taken.tolist())))
        assert taken.min() >= 8, taken
        st = ref["start"][branch == 4]
        assert (st < nplan - 1 - N).any() == (nplan == 41)            # windows without a repeated last row exist at nplan = 41 only
        assert ((st >= nplan // 3) & (st < 2 * nplan // 3)).sum() >= 8 and (st >= nplan - 4).sum() >= 8
        assert (ref["start"][np.isin(branch, (1, 2))] == 0).all()
        _check_against_numpy(r, ref)
        # the outputs of the transition only where there was one
        trans = d["phase"] == H.DONE
        assert (r["qgoal"][~trans] == -7).all() and (r["ik_status"][~trans] == -7).all() and (r["ik_status"][trans] >= 0).all()
        assert (r["plan"][~trans & ~own] == -7).all() and np.array_equal(r["plan"][own], d["plan"][own])
        assert int(r["counts"].sum()) == int((ref["phase"] >= H.MANIPULATE).sum())
        # the endpoint of the finish test against the package's forward kinematics
        e = H.endpoint(r["x"])
        e_ref = np.array([H.fk(mm, r["x"][b]) for b in range(B)])
        err = float(TH.ulp_err(e, e_ref).max())
        print("endpoint %.2f ulp" % err)
        assert err <= 4.0, err


def test_ik_at_the_transition(mm):
    nplan = 21
    d, branch = H.branch_inputs(448, N, M, nplan)
    r = H.prepare(N, M, DT, _xlim(), **d)
    trans = np.flatnonzero(d["phase"] == H.DONE)
    assert np.array_equal(np.unique(branch[trans]), [1, 2, 3])
    q0 = d["x"][trans, 6:]
    t = np.array([H.local_target(d["x"][b], d["pose"][b]) for b in trans])
    # the target the kernel's transition forms is the definition's, bit for bit
    assert np.array_equal(H.target(d["x"][trans], d["pose"][trans]), t)
    assert (r["ik_status"][trans] == 0).all()
    lane = emu_helper.ik_batch(q0, t)
    assert (lane["status"] == 0).all()
    assert float(np.abs(r["qgoal"][trans] - lane["q"]).max()) < 1e-8
    for i, b in enumerate(trans):
        qo, st, _ = ik.solve(q0[i], t[i])
        assert st == 0 and np.abs(r["qgoal"][b] - qo).max() < 1e-8, (b, r["qgoal"][b], qo)
        assert ((r["qgoal"][b] >= ik.LO) & (r["qgoal"][b] <= ik.HI)).all()
        assert ik.kkt(r["qgoal"][b], t[i]) < 1e-8
    # a reachable target is reached, one out of reach is not
    res = np.array([np.sqrt(ik.objective(r["qgoal"][b], t[i])) for i, b in enumerate(trans)])
    assert (res[branch[trans] == 2] > 0.1).all() and (res[branch[trans] == 3] < 1e-7).all()
    assert (res[branch[trans] == 1] < 1e-7).mean() > 0.9
    # the plan ends at the answer and starts at the state
    assert np.array_equal(r["plan"][trans, -1, 6:], r["qgoal"][trans]) and np.array_equal(r["plan"][trans, 0], d["x"][trans])
    assert np.array_equal(r["plan"][trans, :, :6], np.repeat(d["x"][trans, None, :6], nplan, axis=1))


def test_numpy_definition_is_the_port_of_the_reference(mm, monkeypatch):
    """Interface on the CPU oracle drives 4 robots of the mission fleet to 'manipulate finish'; at every manipulate tick the numpy
    definition, fed that tick's state, the previous phase and Interface's own q_goal, returns Interface's plan, local_traj_ref
    and finish flag bitwise."""
    oracle_engine.patch(monkeypatch, mm)
    F = MH.mission_fleet(mm, 16, N, DT)
    xlim = _xlim()
    nplan = int(2 / DT) + 1
    for b in range(4):
        obstacles = [mm.Obstacles(*F["obs0"][b, m]) for m in range(3)]
        ctrl = mm.MPCWholeBody(mm.MobileManipulator(DT), obstacles, [], N=N)
        world = mm.Interface(DT, 3.0, 2, F["x0"][b], F["pose"][b], ctrl, physical_sim=False)
        world.current_state = np.array(world.x_start, float)
        world.is_active = True
        pose = F["pose"][b:b + 1]
        prev, plan, ticks, total = H.DONE, np.full((1, nplan, 9), -7.0), 0, 0
        with contextlib.redirect_stdout(io.StringIO()):
            for t in range(400):
                x = world.current_state.copy()
                world.current_joints_pose = np.hstack([np.asarray(p, float).reshape(-1) for p in ctrl.robot_model.forward_tranformation(x)])
                before = world.task_flag
                active = world.stateMachineUpdate()
                total += 1
                if world.task_flag in ('manipulate', 'manipulate finish'):
                    if before != 'manipulate':
                        q_goal = world.traj_ref[-1, 6:].copy()
                        lt = H.local_target(x, pose[0])
                        assert world.local_pose_target[1] == 0.0
                        assert float(TH.ulp_err(lt, world.local_pose_target[[0, 2]]).max()) <= 1.0
                        # ... and so is what the kernel's transition forms from the same state
                        kt = H.target(x, pose[0])[0]
                        assert np.array_equal(kt, lt) and float(TH.ulp_err(kt, world.local_pose_target[[0, 2]]).max()) <= 1.0
                    ref = H.reference(mm, xlim, DT, N, x[None], np.zeros(1, np.int64), np.array([prev]), pose, nplan, plan, q_goal[None],
                                      F["obs0"][b:b + 1], F["vel"][b:b + 1])
                    assert np.array_equal(ref["plan"][0], world.traj_ref), (b, t)
                    assert bool(ref["finish"][0]) == (not active) and ref["phase"][0] == (H.MANIPULATE if active else H.MANIP_DONE), (b, t)
                    if not active:
                        assert world.task_flag == 'manipulate finish'
                        break
                    assert np.array_equal(ref["traj_ref"][0], world.local_traj_ref), (b, t)
                    assert not world.local_u_ref.any()
                    assert np.allclose(np.diag(ctrl.Q_value), [500, 500, 500, 0, 0, 1, 1, 1, 1])
                    prev, plan = H.MANIPULATE, ref["plan"]
                    ticks += 1
                assert active
                u = ctrl.solve(world.current_state, world.local_traj_ref, world.local_u_ref)      # raises when the solve does not converge
                world.current_state = np.asarray(ctrl.f_dynamics(world.current_state, u)).squeeze()
            else:
                raise AssertionError("robot %d not finished after 400 ticks" % b)
        err = float(np.linalg.norm(H.fk(mm, world.current_state) - pose[0, :3]))
        print("robot %d: %d ticks, %d of them in manipulate, final endpoint error %.1f mm" % (b, total, ticks, 1e3 * err))
        assert ticks >= 1 and err <= 0.01


def test_frozen_robots_are_neither_read_nor_written(mm):
    nplan = 21
    d, branch = H.branch_inputs(448, N, M, nplan)
    xlim = _xlim()
    r = H.prepare(N, M, DT, xlim, **d)
    out_in = ~np.isin(d["phase"], (H.DONE, H.MANIPULATE))          # driving (< 3) and finished (5) on entry
    now_done = r["phase"] == H.MANIP_DONE
    assert (d["phase"][out_in] < 3).sum() >= 8 and (d["phase"][out_in] == 5).sum() >= 8 and (now_done & ~out_in).sum() >= 16
    for k in KEYS:
        assert (r[k][out_in | now_done] == -7).all(), k
        assert not (r[k][r["phase"] == H.MANIPULATE] == -7).all(axis=tuple(range(1, r[k].ndim))).any(), k
    for k in ("x", "tick", "phase"):
        assert np.array_equal(r[k][out_in], d[k][out_in]), k
    assert (r["plan"][out_in] == -7).all() and (r["qgoal"][out_in] == -7).all()
    n = int(r["counts"][0])
    assert not np.isin(np.flatnonzero(out_in | now_done), r["list"][:n]).any()
    assert r["counts"][1] == now_done.sum() and r["counts"][0] == (r["phase"] == H.MANIPULATE).sum()
    # nothing of them is read: non-finite rows behind a frozen robot change nothing
    poison = dict(d, x=d["x"].copy(), pose=d["pose"].copy(), U_prev=d["U_prev"].copy(), plan=d["plan"].copy())
    for k in ("pose", "U_prev", "plan"):
        poison[k][out_in] = np.nan
    rp = H.prepare(N, M, DT, xlim, **poison)
    for k in KEYS + ("x", "tick", "phase", "qgoal", "ik_status", "counts"):
        assert np.array_equal(rp[k], r[k]), k
    assert np.array_equal(np.sort(rp["list"][:n]), np.sort(r["list"][:n]))
    # a second call on the result: the finished robots stay as they are, whatever the previous optimum says
    r2 = H.prepare(N, M, DT, xlim, r["x"], r["tick"], r["phase"], d["pose"], nplan, d["U_prev"], r["plan"], d["obs0"], d["vel"])
    frozen = out_in | now_done
    for k in ("x", "tick", "phase"):
        assert np.array_equal(r2[k][frozen], r[k][frozen]), k
    for k in KEYS:
        assert (r2[k][frozen] == -7).all(), k
    assert np.array_equal(r2["plan"], r["plan"]) and (r2["qgoal"] == -7).all()       # no transition is left
    assert r2["counts"][1] >= now_done.sum()


def test_non_finite_robot_keeps_its_phase_and_stays_alone(mm):
    nplan = 21
    d, branch = H.branch_inputs(70, N, M, nplan)
    xlim = _xlim()
    clean = H.prepare(N, M, DT, xlim, **d)
    x = d["x"].copy()
    bad = {4: (0, np.nan), 5: (7, np.nan), 11: (2, np.nan), 12: (2, -np.inf), 18: (6, np.nan),     # in MANIPULATE on entry
           1: (0, np.nan), 3: (6, np.nan), 9: (2, np.nan)}                                         # at the transition
    for b, (c, v) in bad.items():
        assert d["phase"][b] == (H.MANIPULATE if b % 7 in (4, 5) else H.DONE)
        x[b, c] = v
    r = H.prepare(N, M, DT, xlim, **dict(d, x=x))
    n = int(r["counts"][0])
    for b in bad:
        assert r["phase"][b] == H.MANIPULATE and not np.isfinite(r["x_in"][b]).all(), b
        assert b in r["list"][:n] and 0 <= r["start"][b] < nplan
    # a failed IK does not stop the robot: with a NaN in the base position the target is NaN, no step of the solver is accepted and
    # the status says so; the robot is in MANIPULATE all the same (above), its plan goes to the point the solver returned - the
    # start's joints, which lie inside the box
    assert r["ik_status"][1] == 1 and np.array_equal(r["qgoal"][1], d["x"][1, 6:]) and np.array_equal(r["plan"][1, -1, 6:], r["qgoal"][1])
    assert r["ik_status"][9] == 0                      # (a NaN heading does not reach the target: the IK is the clean run's)
    assert r["ik_status"][3] >= 0 and np.isfinite(r["qgoal"][3]).all()
    rest = np.ones(70, bool); rest[list(bad)] = False
    for k in KEYS + ("x", "tick", "phase", "plan", "qgoal", "ik_status"):
        assert np.array_equal(r[k][rest], clean[k][rest]), k


def test_shortest_plan(mm):
    """nplan = 2: the plan is the state and the target, every window is the target from its second row on at the latest"""
    nplan = 2
    d, branch = H.branch_inputs(70, N, M, nplan)
    xlim = _xlim()
    r = H.prepare(N, M, DT, xlim, **d)
    ref = H.reference(mm, xlim, DT, N, r["x"], r["tick"], d["phase"], d["pose"], nplan, d["plan"], r["qgoal"], d["obs0"], d["vel"])
    _input_condition(mm, r["x"], d["pose"], ref["phase"], ref["plan"])
    _check_against_numpy(r, ref)
    trans = d["phase"] == H.DONE
    assert np.array_equal(r["plan"][trans, 0], d["x"][trans]) and np.array_equal(r["plan"][trans, 1, 6:], r["qgoal"][trans])
    live = r["phase"] == H.MANIPULATE
    assert live.sum() >= 20 and np.array_equal(r["traj_ref"][live, 1:], np.repeat(r["plan"][live, 1:2], N, axis=1))
    assert set(np.unique(r["start"][live])) == {0, 1}


def test_manipulate_kernel_resource_usage_on_gfx950(mm):
    """The kernel source cross-compiled for gfx950: the manipulate kernel's own resource usage, as the compiler reports it (the
    IK's small local arrays may cost it scratch: reported, not bounded)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = "hipcc"
    src = os.path.join(ROOT, "tests", "manipulate_emu", "mmpc_manipulate_probe.hip")
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage", src], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    m = re.search(r"Function Name: mmpc_manipulate_probe_kernel(.*?)LDS Size \[bytes/block\]: (\d+)", p.stderr, re.S)
    assert m, p.stderr[-2000:]
    get = lambda name: int(re.search(re.escape(name) + r": (\d+)", m.group(1)).group(1))
    usage = "VGPRs %d, SGPRs %d, occupancy %d waves/SIMD, scratch %d B/lane, LDS %s B" % (
        get("VGPRs"), get("SGPRs"), get("Occupancy [waves/SIMD]"), get("ScratchSize [bytes/lane]"), m.group(2))
    print(usage)
    # LDS: the tick kernel's slots, no more
    assert int(m.group(2)) == 8 * H.C.CDLL(H.build()).mmpc_manipulate_emu_lds_doubles() == 8 * H.C.CDLL(TH.build()).mmpc_tick_emu_lds_doubles(), usage
