"""CPU: the fleet mission kernel (csrc/mmpc_mission.h) built for the host (g++ -DMMPC_EMU -ffp-contract=off, tests/mission_emu)
against a numpy definition of the mission tick, that definition against the package's port of the reference's state machine
(Interface on the CPU oracle), and the resource usage of the kernel's gfx950 code object.

Bounds.  The numpy definition is evaluated at the build's own advanced state, so everything it is compared in consists of copies,
comparisons and correctly rounded IEEE operations in the same order on both sides (fmod is exact): bitwise.  The advance itself
differs from f_kinematics in sin / cos alone: <= 4 ulp of max(1, |x_i|), the bound of tests/test_fleet_tick_cpu.py.  A comparison
with a threshold can only come out differently on the two sides when its two operands are a rounding error apart, so the inputs
are required to keep every threshold quantity at least 1e-9 from zero."""
import contextlib
import io
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import nlp
from tests import oracle_engine

import mission_emu_helper as H
import tick_emu_helper as TH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, M, DT, NGLOB = 20, 3, 0.1, 31
KEYS = ("x_in", "traj_ref", "start", "obs")


def _xlim():
    return np.asarray(nlp.WholeBodyParams(N=N).xlim, float)


def _margins(mm, x, glob, live):
    return np.array([H.quantities(mm, x[b], glob[b, -1]) for b in np.flatnonzero(live)])


def _check_against_numpy(mm, d, r, ref):
    """every output of one call `r` against the numpy definition `ref` at r's own advanced state"""
    assert np.array_equal(r["phase"], ref["phase"])
    for k in KEYS:
        assert np.array_equal(r[k], ref[k]), k
    assert np.array_equal(r["counts"], ref["counts"])
    for p in range(3):
        n = int(r["counts"][p])
        assert np.array_equal(np.sort(r["lists"][p, :n]), ref["rows"][p]), p
        assert (r["lists"][p, n:] == -7).all(), p


@pytest.mark.parametrize("advance", [True, False], ids=["advance", "no_advance"])
def test_host_build_against_numpy_definition(mm, advance):
    d, branch = H.branch_inputs(512, N, M, NGLOB)
    xlim = _xlim()
    B = 512
    if not advance:
        d = dict(d, U_prev=None)
    done_in = d["phase"] == H.DONE
    for reverse in (False, True):
        r = H.prepare(N, M, DT, xlim, reverse=reverse, **d)
        # the advance: robots that came in DONE are frozen, the others stepped like the tick kernel's
        assert np.array_equal(r["x"][done_in], d["x"][done_in]) and np.array_equal(r["tick"][done_in], d["tick"][done_in])
        live = ~done_in
        if advance:
            adv = TH.reference(mm, xlim, DT, N, d["x"][live], d["tick"][live], d["U_prev"][live], d["glob"][live], d["obs0"][live], d["vel"][live])
            e_adv = float(TH.ulp_err(r["x"][live], adv["x"]).max())
            print("advance %.2f ulp" % e_adv)
            assert e_adv <= 4.0, e_adv
            assert np.array_equal(r["tick"][live], d["tick"][live] + 1)
        else:
            assert np.array_equal(r["x"], d["x"]) and np.array_equal(r["tick"], d["tick"])
        # input condition: no threshold quantity of any robot within 1e-9 of zero; the nearest plan row of a moving robot unambiguous
        q = _margins(mm, r["x"], d["glob"], live)
        assert float(np.abs(q).min()) >= 1e-9, float(np.abs(q).min())
        ref = H.reference(mm, xlim, DT, N, r["x"], r["tick"], d["phase"], d["glob"], d["obs0"], d["vel"])
        mv = ref["phase"] == H.MOVE
        two = np.sort(np.linalg.norm(r["x"][mv, None, :2] - d["glob"][mv, :, :2], axis=2), axis=1)[:, :2]
        assert float((two[:, 1] - two[:, 0]).min()) > 1e-9
        # every branch is taken, by the robots drawn for it
        assert np.array_equal(ref["phase"], H.expected_after(branch))
        taken = np.bincount(branch, minlength=len(H.BRANCHES))
        print(dict(zip(H.BRANCHES, taken.tolist())))
        assert taken.min() >= 8, taken
        # headings on both sides of +-pi: for each of the goal headings -pi, pi and 3.1, robots whose wrapped heading is on either
        # side of the cut decide the rotate branches
        rot = np.isin(branch, (3, 6, 7, 8, 9))
        wrap = np.fmod(r["x"][:, 2] + np.pi, 2 * np.pi) - np.pi
        for gh in (-np.pi, np.pi, 3.1):
            sel = rot & (d["glob"][:, -1, 2] == gh)
            assert (wrap[sel] > 3.0).any() and ((wrap[sel] < -3.0).any() or gh == 3.1), gh
            assert (ref["phase"][sel] == H.DONE).any() and (ref["phase"][sel] == H.ROTATE).any(), gh
        _check_against_numpy(mm, d, r, ref)
        assert int(r["counts"].sum()) == B


def test_done_robots_are_frozen(mm):
    d, branch = H.branch_inputs(512, N, M, NGLOB)
    xlim = _xlim()
    r = H.prepare(N, M, DT, xlim, **d)
    came_done = d["phase"] == H.DONE
    now_done = r["phase"] == H.DONE
    assert came_done.sum() >= 8 and (now_done & ~came_done).sum() >= 24
    for k in KEYS:
        assert (r[k][now_done] == -7).all(), k
        assert not (r[k][~now_done] == -7).all(axis=tuple(range(1, r[k].ndim))).any(), k
    assert np.array_equal(r["x"][came_done], d["x"][came_done]) and np.array_equal(r["tick"][came_done], d["tick"][came_done])
    listed = np.concatenate([r["lists"][p, :r["counts"][p]] for p in range(3)])
    assert not np.isin(np.flatnonzero(now_done), listed).any()
    assert r["counts"][3] == now_done.sum()
    # a second call on the result: the finished robots stay as they are, whatever the previous optimum says
    r2 = H.prepare(N, M, DT, xlim, r["x"], r["tick"], r["phase"], d["U_prev"], d["glob"], d["obs0"], d["vel"])
    assert np.array_equal(r2["x"][now_done], r["x"][now_done]) and np.array_equal(r2["tick"][now_done], r["tick"][now_done])
    assert (r2["phase"][now_done] == H.DONE).all()


def test_the_box_edge_is_inclusive(mm):
    """|x0 - g0| <= 2 and |x1 - g1| <= 2 on representable values, no advance: exactly on the edge is inside, one ulp out is outside."""
    xlim = _xlim()
    # (goal at the origin: x - g is x itself, so "one ulp outside" is not rounded away by the subtraction)
    out_hi, out_lo = np.nextafter(2.0, np.inf), np.nextafter(-2.0, -np.inf)
    cases = [(-2.0, 0.5, 1), (2.0, 0.5, 1), (0.5, -2.0, 1), (0.5, 2.0, 1), (2.0, -2.0, 1),
             (out_lo, 0.5, 0), (out_hi, 0.5, 0), (0.5, out_lo, 0), (0.5, out_hi, 0)]
    B = len(cases)
    x = np.zeros((B, 9))
    x[:, 0], x[:, 1] = [c[0] for c in cases], [c[1] for c in cases]
    goal = np.zeros(9)
    first = goal.copy(); first[0] = 8.0
    glob = np.ascontiguousarray(np.repeat(np.linspace(first, goal, NGLOB)[None], B, axis=0))
    r = H.prepare(N, M, DT, xlim, x, np.zeros(B, np.int64), np.zeros(B, np.int32), None, glob, np.zeros((B, M, 3)), np.zeros((B, M, 2)))
    assert np.array_equal(r["phase"], [c[2] for c in cases])
    assert np.array_equal(r["phase"], [H.state_machine(mm, x[b], goal, 0) for b in range(B)])
    assert np.array_equal(r["counts"], [4, 5, 0, 0])


def test_non_finite_robot_keeps_its_phase_and_stays_alone(mm):
    d, _ = H.branch_inputs(66, N, M, NGLOB)
    xlim = _xlim()
    clean = H.prepare(N, M, DT, xlim, **d)
    x = d["x"].copy()
    bad = {0: (0, np.nan), 1: (1, np.nan), 4: (2, np.nan), 7: (2, -np.inf), 8: (0, np.nan)}     # a robot of entry phase 0, 0, 1, 2, 2
    for b, (c, v) in bad.items():
        x[b, c] = v
    r = H.prepare(N, M, DT, xlim, **dict(d, x=x))
    for b in bad:
        assert r["phase"][b] == d["phase"][b] and not np.isfinite(r["x_in"][b]).all(), b
        assert b in r["lists"][d["phase"][b], :r["counts"][d["phase"][b]]]
    rest = np.ones(66, bool); rest[list(bad)] = False
    for k in KEYS + ("x", "tick", "phase"):
        assert np.array_equal(r[k][rest], clean[k][rest]), k


def test_mission_kernel_uses_no_scratch_on_gfx950(mm):
    """The kernel source cross-compiled for gfx950: the mission kernel's own resource usage, as the compiler reports it."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = "hipcc"
    src = os.path.join(ROOT, "tests", "mission_emu", "mmpc_mission_probe.hip")
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage", src], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    m = re.search(r"Function Name: mmpc_mission_probe_kernel(.*?)LDS Size \[bytes/block\]: (\d+)", p.stderr, re.S)
    assert m, p.stderr[-2000:]
    get = lambda name: int(re.search(re.escape(name) + r": (\d+)", m.group(1)).group(1))
    usage = "VGPRs %d, SGPRs %d, occupancy %d waves/SIMD, scratch %d B/lane, LDS %s B" % (
        get("VGPRs"), get("SGPRs"), get("Occupancy [waves/SIMD]"), get("ScratchSize [bytes/lane]"), m.group(2))
    print(usage)
    assert get("ScratchSize [bytes/lane]") == 0, usage
    # LDS of the tick kernel's order: the very same slots
    assert int(m.group(2)) == 8 * H.C.CDLL(H.build()).mmpc_mission_emu_lds_doubles() == 8 * H.C.CDLL(TH.build()).mmpc_tick_emu_lds_doubles(), usage


def test_numpy_state_machine_is_the_port_of_the_reference(mm, monkeypatch):
    """Interface on the CPU oracle drives 4 robots of the mission fleet to 'move finish'; at every tick the numpy definition, fed
    that tick's state and the previous phase, returns Interface's flag and local_traj_ref bitwise."""
    oracle_engine.patch(monkeypatch, mm)
    iface = __import__("importlib").import_module(mm.__name__ + ".interface_wholebody_qref")
    F = H.mission_fleet(mm, 16, N, DT)
    xlim = _xlim()
    names = {'move': H.MOVE, 'approach': H.APPROACH, 'rotate': H.ROTATE}
    for b in range(4):
        obstacles = [mm.Obstacles(*F["obs0"][b, m]) for m in range(3)]
        ctrl = mm.MPCWholeBody(mm.MobileManipulator(DT), obstacles, [], N=N)
        world = mm.Interface(DT, 3.0, 2, F["x0"][b], F["pose"][b], ctrl, physical_sim=False)
        assert np.array_equal(world.x_target, F["glob"][b, -1])
        world.current_state = np.array(world.x_start, float)
        world.is_active = True
        prev, seq = H.MOVE, []
        with contextlib.redirect_stdout(io.StringIO()):
            for t in range(400):
                x = world.current_state.copy()
                world.current_joints_pose = np.hstack([np.asarray(p, float).reshape(-1) for p in ctrl.robot_model.forward_tranformation(x)])
                assert world.stateMachineUpdate()
                ref = H.reference(mm, xlim, DT, N, x[None], np.zeros(1, np.int64), np.array([prev]), F["glob"][b:b + 1], F["obs0"][b:b + 1], F["vel"][b:b + 1])
                if world.task_flag not in names:            # 'move finish' is passed through at once (:179-185)
                    assert world.task_flag == 'manipulate' and ref["phase"][0] == H.DONE
                    break
                assert np.array_equal(world.traj_ref, F["glob"][b])
                assert ref["phase"][0] == names[world.task_flag], (b, t)
                assert np.array_equal(ref["traj_ref"][0], world.local_traj_ref), (b, t)
                assert not world.local_u_ref.any()
                prev = int(ref["phase"][0])
                seq.append(prev)
                u = ctrl.solve(world.current_state, world.local_traj_ref, world.local_u_ref)      # raises when the solve does not converge
                world.current_state = np.asarray(ctrl.f_dynamics(world.current_state, u)).squeeze()
            else:
                raise AssertionError("robot %d not finished after 400 ticks" % b)
        ph = [k for k, _ in itertools.groupby(seq)]
        print("robot %d: %d ticks, %s" % (b, len(seq), [(k, len(list(v))) for k, v in itertools.groupby(seq)]))
        assert ph == [H.MOVE, H.APPROACH, H.ROTATE], ph
