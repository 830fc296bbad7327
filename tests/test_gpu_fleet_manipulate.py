"""GPU (MI355X): the fleet manipulate kernel (mmpc_manipulate_prepare_device) through the C ABI against its host build and the numpy
definition, and DeviceFleet.run_mission(manipulate=...) to 'manipulate finish'.  Bounds as in tests/test_fleet_manipulate_cpu.py:
state, phase, counts and list are bitwise the host build's (same source, every operation rounded on its own; the inputs keep every
threshold quantity 1e-9 from zero, which the CPU test asserts); the IK's answer is the host build's to 1e-8 (library sin / cos on both
sides, not the same ones); plan, window, start, x_in and obstacle table are bitwise the numpy definition at the device's own state and
q_goal.  In the end-to-end run the one place where two sides may differ is a threshold comparison replayed in numpy inside 1e-9 of
the threshold; the share of such (robot, tick) pairs is bounded by 2 %, the cap of tests/test_gpu_fleet_mission.py."""
import ctypes as C

import numpy as np
import pytest

from oracle import nlp

import manipulate_emu_helper as H
import mission_emu_helper as MH

pytestmark = pytest.mark.gpu
N, M, DT = 20, 3, 0.1
KEYS = ("x_in", "traj_ref", "start", "obs")


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _ctrl(mm, B, n=N, m=M, **kw):
    kw.setdefault("obs_per_stage", True)
    return mm.MPCWholeBody(mm.MobileManipulator(DT), [], [], N=n, max_batch=B, n_obstacles=m, **kw)


def _run_kernel(eng, d, rows=None, motion=False, advance=True):
    """d: numpy inputs of H.branch_inputs -> numpy outputs of one mmpc_manipulate_prepare_device call (buffers of `rows` rows)"""
    import torch
    B, nplan = d["x"].shape[0], d["nplan"]
    R = B if rows is None else rows
    f = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device="cuda:0")
    i = lambda *s: torch.full(s, -7, dtype=torch.int32, device="cuda:0")
    out = dict(x_in=f(R, 9), traj_ref=f(R, N + 1, 9), start=i(R), obs=f(R, N + 1, M, 3), plan=f(R, nplan, 9), qgoal=f(R, 3), ik_status=i(R))
    out["plan"][:B] = _dev(d["plan"])
    x, tick, phase = _dev(d["x"]), _dev(d["tick"]), _dev(d["phase"])
    lst, counts = i(B), i(2)
    kw = {k: out[k][:B] for k in KEYS + ("plan", "qgoal", "ik_status") if not (motion and k == "obs")}
    if not motion:
        kw.update(obs0=_dev(d["obs0"]), vel=_dev(d["vel"]))
    eng.manipulate_prepare(x, tick, phase, _dev(d["pose"]), lst=lst, counts=counts, U_prev=_dev(d["U_prev"]) if advance else None, **kw)
    torch.cuda.synchronize()
    r = {k: v.cpu().numpy() for k, v in out.items()}
    r.update(x=x.cpu().numpy(), tick=tick.cpu().numpy(), phase=phase.cpu().numpy(), list=lst.cpu().numpy(), counts=counts.cpu().numpy())
    return r


def _against_host_and_numpy(mm, d, r, h, xlim, keys):
    B, nplan = d["x"].shape[0], d["nplan"]
    for k in ("x", "tick", "phase", "counts", "ik_status"):
        assert np.array_equal(r[k], h[k]), k
    n = int(h["counts"][0])
    assert np.array_equal(np.sort(r["list"][:n]), np.sort(h["list"][:n])) and (r["list"][n:] == -7).all()
    trans = d["phase"] == H.DONE
    assert (r["qgoal"][~trans] == -7).all()
    dq = float(np.abs(r["qgoal"][trans] - h["qgoal"][trans]).max())
    print("q_goal against the host build: %.2e" % dq)
    assert dq < 1e-8, dq
    ref = H.reference(mm, xlim, DT, N, r["x"], r["tick"], d["phase"], d["pose"], nplan, d["plan"], r["qgoal"], d["obs0"], d["vel"])
    assert np.array_equal(r["phase"], ref["phase"])
    for k in ("plan",) + keys:
        assert np.array_equal(r[k][:B], ref[k]), k


@pytest.mark.parametrize("nplan", [21, 41])
def test_kernel_against_its_host_build_and_the_numpy_definition(mm, nplan):
    d, _ = H.branch_inputs(448, N, M, nplan)
    table = _ctrl(mm, 448)
    xlim = np.asarray(table.xlim, float)
    assert np.array_equal(xlim, np.asarray(nlp.WholeBodyParams(N=N).xlim, float))
    h = H.prepare(N, M, DT, xlim, **d)
    _against_host_and_numpy(mm, d, _run_kernel(table._engine, d), h, xlim, KEYS)
    if nplan == 21:
        _against_host_and_numpy(mm, d, _run_kernel(table._engine, d, advance=False), H.prepare(N, M, DT, xlim, **dict(d, U_prev=None)), xlim, KEYS)
        motion = _ctrl(mm, 448, obs_per_stage="motion")
        r = _run_kernel(motion._engine, d, motion=True)
        _against_host_and_numpy(mm, d, r, h, xlim, ("x_in", "traj_ref", "start"))
        assert (r["obs"] == -7).all()


def test_failed_ik_does_not_stop_the_robot(mm):
    """A NaN in a robot's base position makes its arm-frame target NaN: the IK accepts no step and reports it (status 1).  The robot
    goes to MANIPULATE all the same, with a plan to the point the solver returned (the start's joints), and no other robot changes."""
    nplan = 21
    d, _ = H.branch_inputs(70, N, M, nplan)
    assert d["phase"][1] == H.DONE
    ctrl = _ctrl(mm, 70)
    xlim = np.asarray(ctrl.xlim, float)
    clean = _run_kernel(ctrl._engine, d)
    bad = dict(d, x=d["x"].copy())
    bad["x"][1, 0] = np.nan
    r, h = _run_kernel(ctrl._engine, bad), H.prepare(N, M, DT, xlim, **bad)
    n = int(r["counts"][0])
    assert r["ik_status"][1] == 1 == h["ik_status"][1] and clean["ik_status"][1] == 0
    assert r["phase"][1] == H.MANIPULATE and 1 in r["list"][:n] and r["start"][1] == 0
    assert np.array_equal(r["qgoal"][1], d["x"][1, 6:]) and np.array_equal(r["plan"][1, -1, 6:], r["qgoal"][1])
    assert np.array_equal(r["plan"][1], h["plan"][1], equal_nan=True) and np.array_equal(r["traj_ref"][1], h["traj_ref"][1], equal_nan=True)
    rest = np.arange(70) != 1
    for k in KEYS + ("x", "tick", "phase", "plan", "qgoal", "ik_status"):
        assert np.array_equal(r[k][rest], clean[k][rest]), k
    assert np.array_equal(r["counts"], clean["counts"])


def test_rows_beyond_the_batch_are_not_written_and_error_codes(mm):
    import torch
    nplan = 21
    d, _ = H.branch_inputs(200, N, M, nplan)
    ctrl = _ctrl(mm, 256)
    eng = ctrl._engine
    full = _run_kernel(eng, d)
    part = _run_kernel(eng, d, rows=256)
    for k in KEYS + ("plan", "qgoal", "ik_status"):
        assert np.array_equal(part[k][:200], full[k]), k
        assert (part[k][200:] == -7).all(), k
    x, tick, phase, pose, plan, obs0, vel, U = (_dev(d[k]) for k in ("x", "tick", "phase", "pose", "plan", "obs0", "vel", "U_prev"))
    lst = torch.zeros(200, dtype=torch.int32, device="cuda:0"); counts = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    obs = torch.zeros((200, N + 1, M, 3), dtype=torch.float64, device="cuda:0")
    req = dict(phase=phase, pose=pose, plan=plan, lst=lst, counts=counts)
    base = mm.MPCBase(mm.Base(DT), [], N=15, max_batch=256)
    with pytest.raises(RuntimeError, match=r"mmpc_manipulate_prepare_device failed \(-4\)"):
        base._engine.manipulate_prepare(x, tick, **req)
    with pytest.raises(RuntimeError, match=r"\(-4\).*obs_per_stage"):
        _ctrl(mm, 256, obs_per_stage=False)._engine.manipulate_prepare(x, tick, **req)
    with pytest.raises(RuntimeError, match=r"\(-1\).*d_obs must be NULL"):
        _ctrl(mm, 256, obs_per_stage="motion")._engine.manipulate_prepare(x, tick, obs0=obs0, vel=vel, obs=obs, **req)
    with pytest.raises(RuntimeError, match=r"\(-1\).*max_batch"):
        _ctrl(mm, 100)._engine.manipulate_prepare(x, tick, **req)
    with pytest.raises(RuntimeError, match=r"\(-1\).*d_obs0 and d_vel"):
        eng.manipulate_prepare(x, tick, obs=obs, **req)
    with pytest.raises(RuntimeError, match=r"\(-1\).*nplan"):
        eng.manipulate_prepare(x, tick, **dict(req, plan=plan[:, :1].contiguous()))
    for name in req:
        with pytest.raises(ValueError, match="%s is required" % name):
            eng.manipulate_prepare(x, tick, **dict(req, **{name: None}))
    # ... and the C entry point itself, which the wrapper's checks keep such calls from
    fn = mm._capi.lib().mmpc_manipulate_prepare_device
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    x_before, phase_before = x.clone(), phase.clone()

    def call(a, npl=nplan, tk=tick, B=200):
        return fn(eng._h, B, p(a.get("x", x)), p(tk), p(a["phase"]), p(U), p(a["pose"]), npl, p(a["plan"]), None, None, p(obs0), p(vel), None, None,
                  None, None, p(a["lst"]), p(a["counts"]), None)

    for miss in req:
        assert call(dict(req, **{miss: None})) == -1, miss
    assert call(dict(req, x=None)) == -1
    for npl in (1, 0, -3, (1 << 16) + 1):
        assert call(req, npl=npl) == -1, npl
    assert call(req, tk=None) == -1                 # the advance needs d_tick
    assert call(req, B=257) == -1 and call(req, B=-1) == -1
    assert fn(None, 200, p(x), p(tick), p(phase), p(U), p(pose), nplan, p(plan), None, None, None, None, None, None, None, None, p(lst), p(counts), None) == -1
    assert call(req, B=0) == 0                       # a no-op
    torch.cuda.synchronize()
    assert torch.equal(x, x_before) and torch.equal(phase, phase_before)


T_MISSION = 220


@pytest.fixture(scope="module")
def mission(mm):
    """the fleet of 16 of MH.mission_fleet with its pose targets, run once for T_MISSION ticks to 'manipulate finish', with every tick's
    inputs, states, plans and U rows logged; and the same fleet's mission without the manipulate phase"""
    import torch
    F = MH.mission_fleet(mm, 16, N, DT)
    fleet = mm.DeviceFleet(mm, F["x0"], F["glob"], F["obs0"], F["vel"], N=N)
    log = []

    def on_tick(t, s):
        log.append({k: s[k].clone() for k in ("x", "x_in", "loc", "obs", "u_last", "U", "plan")})

    man = dict(pose=F["pose"], t_manipulate=2)
    res = fleet.run_mission(T_MISSION, streams=1, on_tick=on_tick, manipulate=man)
    torch.cuda.synchronize()
    plain = fleet.run_mission(T_MISSION, streams=1)
    torch.cuda.synchronize()
    np_ = lambda r: {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in r.items()}
    return dict(F=F, fleet=fleet, log=log, man=man, res=np_(res), plain=np_(plain))


def test_mission_end_to_end(mm, mission):
    import torch
    F, fleet, log, r, plain = mission["F"], mission["fleet"], mission["log"], mission["res"], mission["plain"]
    B, T, nplan = 16, T_MISSION, 21
    ph, pose = r["phase"], F["pose"]
    assert r["plan"].shape == (B, nplan, 9) and r["mcounts"].shape == (T, 2) and r["counts"].shape == (T, 4)
    ticks = [[int((ph[b] == p).sum()) for p in (0, 1, 2, 4)] for b in range(B)]
    print("ticks in move / approach / rotate / manipulate per robot:", ticks)
    assert (ph[:, -1] == 5).all() and (r["final_phase"] == 5).all(), ph[:, -1]
    assert bool(r["all_converged"]) and (r["status"] == 0).all() and (r["ik_status"] == 0).all()
    assert (np.diff(ph, axis=1) >= 0).all() and not (ph == 3).any()
    assert all(min(tk) >= 1 for tk in ticks)                                      # every robot passes through every phase
    assert np.array_equal(r["counts"], np.stack([(ph == 0).sum(axis=0), (ph == 1).sum(axis=0), (ph == 2).sum(axis=0), (ph >= 3).sum(axis=0)], axis=1))
    assert np.array_equal(r["mcounts"], np.stack([(ph == 4).sum(axis=0), (ph == 5).sum(axis=0)], axis=1))
    solved = (ph < 3) | (ph == 4)
    assert (r["iters"][solved] > 0).all() and (r["iters"][~solved] == 0).all() and (r["u0"][~solved] == 0).all()
    # the pose target is reached as the state machine defines it
    err = np.array([np.linalg.norm(H.fk(mm, r["x"][b]) - pose[b, :3]) for b in range(B)])
    print("final endpoint error, mm: %.1f-%.1f" % (1e3 * err.min(), 1e3 * err.max()))
    assert (err <= 0.01).all(), err
    # replay of the numpy state machine on the logged states; the plan of every robot is the definition's at its transition
    X = np.stack([l["x"].cpu().numpy() for l in log], axis=1)                    # (B, T, 9): the state tick t's state machine saw
    g = F["glob"][:, -1]
    pairs = inside = 0
    for b in range(B):
        prev = MH.MOVE
        for t in range(T):
            if prev == H.MANIP_DONE:
                assert ph[b, t] == H.MANIP_DONE and np.array_equal(X[b, t], X[b, t - 1])
                continue
            pairs += 1
            p, q = prev, []
            if p < 3:
                q += list(MH.quantities(mm, X[b, t], g[b]))
                p = MH.state_machine(mm, X[b, t], g[b], p)
            if p >= 3:
                if prev < 3 and ph[b, t] >= H.MANIPULATE:
                    tgt = np.hstack((X[b, t, :6], r["qgoal"][b]))
                    assert np.array_equal(log[t]["plan"][b].cpu().numpy(), np.linspace(X[b, t], tgt, nplan)), (b, t)
                    assert np.array_equal(r["plan"][b], log[t]["plan"][b].cpu().numpy())
                fq = H.quantities(mm, X[b, t], pose[b])
                q += list(fq)
                p = H.MANIP_DONE if fq[0] <= 0 else H.MANIPULATE
            if np.abs(q).min() >= 1e-9:
                assert p == ph[b, t], (b, t)
            else:
                inside += 1
            prev = int(ph[b, t])
    print("(robot, tick) pairs inside 1e-9 of a threshold: %d of %d" % (inside, pairs))
    assert inside <= 0.02 * pairs, (inside, pairs)
    # robot 0, first manipulate tick: the logged U row is that of a whole-batch solve of the tick's inputs on the fourth handle
    eng = fleet._mission_ctrls[3]._engine
    assert fleet.engs[0].runs_specialised and not eng.runs_specialised
    assert np.allclose(np.diag(fleet._mission_ctrls[3].Q_value), [500, 500, 500, 0, 0, 1, 1, 1, 1])
    t = int(np.argmax(ph[0] == 4))
    l = log[t]
    o = eng.solve_batch_device(l["x_in"], l["loc"], fleet.uref, l["u_last"], l["obs"])
    torch.cuda.synchronize()
    assert torch.equal(o["U"][0], l["U"][0]), t
    assert np.array_equal(o["U"][0, 0].cpu().numpy(), r["u0"][0, t])
    # its window: the plan from its nearest row (the first one: the arm has not moved yet)
    assert np.array_equal(l["loc"][0].cpu().numpy(), r["plan"][0][np.minimum(np.arange(N + 1), nplan - 1)])
    # up to each robot's 'move finish' tick the mission is the one without the manipulate phase
    for b in range(B):
        assert (plain["phase"][b] == 3).any()
        td = int(np.argmax(plain["phase"][b] == 3))
        for k in ("u0", "iters", "phase", "status"):
            assert np.array_equal(r[k][b, :td], plain[k][b, :td]), (b, k)
        assert ph[b, td] >= 4 and (plain["phase"][b, td:] == 3).all()


def test_robots_do_not_interact_and_streams_do_not_matter(mm, mission):
    import torch
    F, r = mission["F"], mission["res"]
    keys = ("u0", "iters", "status", "phase", "x", "final_phase", "qgoal", "ik_status", "plan")
    for b in range(4):
        one = mm.DeviceFleet(mm, F["x0"][b:b + 1], F["glob"][b:b + 1], F["obs0"][b:b + 1], F["vel"][b:b + 1], N=N).run_mission(
            T_MISSION, manipulate=dict(pose=F["pose"][b:b + 1], t_manipulate=2))
        torch.cuda.synchronize()
        for k in keys:
            assert np.array_equal(one[k].cpu().numpy()[0], r[k][b]), (b, k)
    s3 = mission["fleet"].run_mission(T_MISSION, streams=3, manipulate=mission["man"])
    torch.cuda.synchronize()
    for k in keys + ("counts", "mcounts"):
        assert np.array_equal(s3[k].cpu().numpy(), r[k]), k


def test_manipulate_argument_errors(mm):
    F = MH.mission_fleet(mm, 2, N, DT)
    fleet = mm.DeviceFleet(mm, F["x0"], F["glob"], F["obs0"], F["vel"], N=N)
    with pytest.raises(ValueError, match="pose.*shape"):
        fleet.run_mission(2, manipulate=dict(pose=F["pose"][:, :3]))
    with pytest.raises(ValueError, match="pose.*shape"):
        fleet.run_mission(2, manipulate=dict(pose=F["pose"][:1]))
    with pytest.raises(ValueError, match="t_manipulate"):
        fleet.run_mission(2, manipulate=dict(pose=F["pose"], t_manipulate=0.05))
    with pytest.raises(ValueError, match="t_manipulate"):
        fleet.run_mission(2, manipulate=dict(pose=F["pose"], t_manipulate=float("nan")))
