"""GPU (MI355X): the glue of a mission under iteration budgets through the C ABI (mmpc_mission_round_device,
mmpc_manipulate_round_device, mmpc_mission_commit_device) against its host build, and DeviceFleet.run_mission(budget=..., sets=...)
against the same fleet without a budget.

Bounds.  The kernels are bitwise their host build's (same source, every operation rounded on its own) - except, as in
tests/test_gpu_fleet_manipulate.py, the IK's answer (library sin / cos: 1e-8), so the plan and the window of a robot in transition are
compared with the numpy definition at the device's own q_goal.  End to end the governing claim is that robots do not interact: every
number a robot produces under any budget and any number of handle sets is bit for bit what the same fleet computes without a budget.
The comparator is a generic_budget=True fleet with budget=0 (the run-time-sized generic kernel is another instantiation than a
default fleet's)."""
import ctypes as C

import numpy as np
import pytest

from oracle import nlp

import manipulate_emu_helper as MANH
import mission_emu_helper as MH
import round_emu_helper as R

pytestmark = pytest.mark.gpu
N, M, DT, NGLOB, NPLAN = 20, 3, 0.1, 31, 21
KEYS = ("x_in", "traj_ref", "start", "obs")
LIMIT = 30          # the inputs' ticks are 0..39: a quarter of the READY robots retire


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _ctrl(mm, B, **kw):
    kw.setdefault("obs_per_stage", True)
    return mm.MPCWholeBody(mm.MobileManipulator(DT), [], [], N=N, max_batch=B, n_obstacles=M, **kw)


def _xlim():
    return np.asarray(nlp.WholeBodyParams(N=N).xlim, float)


def _holds(B):
    return np.array(R.MIXED, np.int32)[np.arange(B) % len(R.MIXED)], (100 + np.arange(B)).astype(np.int32)


def _run_round(eng, d, hold, sp, kind, rows, motion=False):
    """numpy inputs -> numpy outputs of one round call on buffers of `rows` >= B rows (everything beyond B starts at -7)"""
    import torch
    B = d["x"].shape[0]
    f = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device="cuda:0")
    i = lambda *s: torch.full(s, -7, dtype=torch.int32, device="cuda:0")

    def big(a, dtype):
        t = torch.full((rows,) + a.shape[1:], -7, dtype=dtype, device="cuda:0")
        t[:B] = _dev(a)
        return t
    st = dict(x=big(d["x"], torch.float64), tick=big(d["tick"], torch.int64), phase=big(d["phase"], torch.int32), hold=big(hold, torch.int32),
              solve_phase=big(sp, torch.int32))
    out = dict(x_in=f(rows, 9), traj_ref=f(rows, N + 1, 9), start=i(rows), obs=f(rows, N + 1, M, 3))
    kw = {k: out[k][:B] for k in KEYS if not (motion and k == "obs")}
    if not motion:
        kw.update(obs0=_dev(d["obs0"]), vel=_dev(d["vel"]))
    s = {k: v[:B] for k, v in st.items()}
    U = _dev(d["U_prev"])
    if kind == "mission":
        lists, counts = i(3, B), i(4)
        eng.mission_round(s["x"], s["tick"], s["phase"], lists, counts, U, s["hold"], s["solve_phase"], LIMIT, glob=_dev(d["glob"]), **kw)
        extra = dict(lists=lists, counts=counts)
    else:
        out.update(plan=big(d["plan"], torch.float64), qgoal=f(rows, 3), ik_status=i(rows))
        lst, counts = i(B), i(2)
        eng.manipulate_round(s["x"], s["tick"], s["phase"], _dev(d["pose"]), out["plan"][:B], lst, counts, U, s["hold"], s["solve_phase"], LIMIT,
                             qgoal=out["qgoal"][:B], ik_status=out["ik_status"][:B], **kw)
        extra = dict(list=lst, counts=counts)
    torch.cuda.synchronize()
    r = {k: v.cpu().numpy() for k, v in {**st, **out, **extra}.items()}
    for k in st.keys() | out.keys():
        assert (r[k][B:] == -7).all(), k             # rows beyond the batch
        r[k] = r[k][:B]
    return r


def _lists_equal(r, h):
    if "lists" in h:
        for p in range(3):
            n = int(h["counts"][p])
            assert np.array_equal(np.sort(r["lists"][p, :n]), np.sort(h["lists"][p, :n])) and (r["lists"][p, n:] == -7).all(), p
    else:
        n = int(h["counts"][0])
        assert np.array_equal(np.sort(r["list"][:n]), np.sort(h["list"][:n])) and (r["list"][n:] == -7).all()


@pytest.mark.parametrize("motion", [False, True], ids=["table", "motion"])
def test_mission_round_kernel_against_its_host_build(mm, motion):
    B = 512
    d, _ = MH.branch_inputs(B, N, M, NGLOB)
    hold, sp = _holds(B)
    h = R.mission_round(N, M, DT, _xlim(), d["x"], d["tick"], d["phase"], d["U_prev"], hold, LIMIT, d["glob"], d["obs0"], d["vel"], solve_phase=sp)
    assert ((hold == R.READY) & (h["hold"] == R.RETIRED)).sum() >= 10 and (h["hold"] == R.RETIRED_AT_DONE).sum() >= 3 and (h["hold"] == R.LISTED).sum() >= 60
    ctrl = _ctrl(mm, B + 32, obs_per_stage="motion" if motion else True)
    assert np.array_equal(np.asarray(ctrl.xlim, float), _xlim())
    r = _run_round(ctrl._engine, d, hold, sp, "mission", B + 32, motion=motion)
    for k in ("x", "tick", "phase", "hold", "solve_phase", "counts", "x_in", "traj_ref", "start"):
        assert np.array_equal(r[k], h[k]), k
    assert (r["obs"] == -7).all() if motion else np.array_equal(r["obs"], h["obs"])
    _lists_equal(r, h)


@pytest.mark.parametrize("motion", [False, True], ids=["table", "motion"])
def test_manipulate_round_kernel_against_its_host_build(mm, motion):
    B = 448
    d, _ = MANH.branch_inputs(B, N, M, NPLAN)
    hold, sp = _holds(B)
    hold = np.where((np.arange(B) % 5 == 0) & (d["phase"] == 3) & ~np.isin(hold, (R.NEW, R.READY)), R.RETIRED_AT_DONE, hold).astype(np.int32)
    xlim = _xlim()
    h = R.manipulate_round(N, M, DT, xlim, d["x"], d["tick"], d["phase"], d["pose"], NPLAN, d["U_prev"], hold, LIMIT, plan=d["plan"],
                           obs0=d["obs0"], vel=d["vel"], solve_phase=sp)
    assert ((hold == R.RETIRED_AT_DONE) & (h["hold"] == R.RETIRED)).sum() >= 5 and ((hold == R.READY) & (h["hold"] == R.RETIRED)).sum() >= 3
    assert (h["hold"] == R.LISTED).sum() >= 30
    ctrl = _ctrl(mm, B + 32, obs_per_stage="motion" if motion else True)
    r = _run_round(ctrl._engine, d, hold, sp, "manipulate", B + 32, motion=motion)
    for k in ("x", "tick", "phase", "hold", "solve_phase", "counts", "ik_status", "x_in", "start"):
        assert np.array_equal(r[k], h[k]), k
    assert (r["obs"] == -7).all() if motion else np.array_equal(r["obs"], h["obs"])
    _lists_equal(r, h)
    trans = h["ik_status"] != -7
    assert trans.sum() >= 40 and (r["qgoal"][~trans] == -7).all()
    dq = float(np.abs(r["qgoal"][trans] - h["qgoal"][trans]).max())
    print("q_goal against the host build: %.2e" % dq)
    assert dq < 1e-8, dq
    # plan and window: the host build's where no IK enters, the numpy definition at the device's own q_goal at a transition
    for k in ("plan", "traj_ref"):
        assert np.array_equal(r[k][~trans], h[k][~trans]), k
    ref = MANH.reference(mm, xlim, DT, N, r["x"], r["tick"], d["phase"], d["pose"], NPLAN, d["plan"], r["qgoal"], d["obs0"], d["vel"])
    assert np.array_equal(r["plan"][trans], ref["plan"][trans])
    listed = trans & (h["hold"] == R.LISTED)
    assert listed.sum() >= 20 and np.array_equal(r["traj_ref"][listed], ref["traj_ref"][listed])
    assert (r["traj_ref"][trans & ~listed] == -7).all()


@pytest.mark.parametrize("rejoin", [0, 1])
@pytest.mark.parametrize("set_", [1, 3])
def test_commit_kernel_against_its_host_build(mm, set_, rejoin):
    import torch
    B, T, rows = 512, 7, 544
    s = R.commit_inputs(B, N, T)
    h = R.commit(N, s, set_, rejoin)
    eng = _ctrl(mm, rows)._engine

    def big(a):
        t = torch.full((rows,) + a.shape[1:], -7, dtype=_dev(a[:1]).dtype, device="cuda:0")
        t[:B] = _dev(a)
        return t
    t = {k: big(v) for k, v in s.items()}
    counters = torch.full((4,), -7, dtype=torch.int32, device="cuda:0")
    v = lambda k: t[k][:B]
    eng.mission_commit(v("hold"), v("solve_phase"), set_, rejoin, dict(U=v("U"), status=v("status"), iters=v("iters")), v("tick"), v("phase"),
                       v("U_last"), v("u0"), v("iters_hist"), v("status_hist"), v("phase_hist"), counters)
    torch.cuda.synchronize()
    for k in R.COMMIT_STATE:
        got = t[k].cpu().numpy()
        assert np.array_equal(got[:B], h[k]) and (got[B:] == -7).all(), k
    assert np.array_equal(counters.cpu().numpy(), h["counters"])


def test_error_codes(mm):
    import torch
    B = 200
    d, _ = MH.branch_inputs(B, N, M, NGLOB)
    dm, _ = MANH.branch_inputs(B, N, M, NPLAN)
    eng = _ctrl(mm, 256)._engine
    i32 = dict(dtype=torch.int32, device="cuda:0")
    x, tick, phase, U, glob, obs0, vel = (_dev(d[k]) for k in ("x", "tick", "phase", "U_prev", "glob", "obs0", "vel"))
    pose, plan = _dev(dm["pose"]), _dev(dm["plan"])
    hold, sp = torch.full((B,), R.RETIRED, **i32), torch.full((B,), -1, **i32)         # (every robot skipped: a call that gets through writes nothing)
    lists, counts, lst, mcounts = torch.zeros((3, B), **i32), torch.zeros(4, **i32), torch.zeros(B, **i32), torch.zeros(2, **i32)
    obs = torch.zeros((B, N + 1, M, 3), dtype=torch.float64, device="cuda:0")
    req = dict(phase=phase, lists=lists, counts=counts, U_last=U, hold=hold, solve_phase=sp, tick_limit=9, glob=glob)
    mreq = dict(phase=phase, pose=pose, plan=plan, lst=lst, counts=mcounts, U_last=U, hold=hold, solve_phase=sp, tick_limit=9)
    for call, rq, name in ((lambda e, **k: e.mission_round(x, tick, **k), req, "mmpc_mission_round_device"),
                           (lambda e, **k: e.manipulate_round(x, tick, **k), mreq, "mmpc_manipulate_round_device")):
        with pytest.raises(RuntimeError, match=name + r" failed \(-4\)"):
            call(mm.MPCBase(mm.Base(DT), [], N=15, max_batch=256)._engine, **dict(rq, U_last=U[:, :15].contiguous()))
        with pytest.raises(RuntimeError, match=r"\(-4\).*obs_per_stage"):
            call(_ctrl(mm, 256, obs_per_stage=False)._engine, **rq)
        with pytest.raises(RuntimeError, match=r"\(-1\).*d_obs must be NULL"):
            call(_ctrl(mm, 256, obs_per_stage="motion")._engine, obs0=obs0, vel=vel, obs=obs, **rq)
        with pytest.raises(RuntimeError, match=r"\(-1\).*max_batch"):
            call(_ctrl(mm, 100)._engine, **rq)
        with pytest.raises(RuntimeError, match=r"\(-1\).*d_obs0 and d_vel"):
            call(eng, obs=obs, **rq)
        with pytest.raises(RuntimeError, match=r"\(-1\).*tick_limit"):
            call(eng, **dict(rq, tick_limit=0))
        for k in rq:
            if k != "tick_limit":
                with pytest.raises(ValueError, match="%s is required" % k):
                    call(eng, **dict(rq, **{k: None}))
    with pytest.raises(RuntimeError, match=r"\(-1\).*nplan"):
        eng.manipulate_round(x, tick, **dict(mreq, plan=plan[:, :1].contiguous()))
    # the C entry points themselves
    L = mm._capi.lib()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    x0, ph0 = x.clone(), phase.clone()

    def mission(B_=B, h=eng._h, **a):
        g = lambda k, v: p(a.get(k, v))
        return L.mmpc_mission_round_device(h, B_, g("x", x), g("tick", tick), g("phase", phase), g("U_last", U), g("glob", glob), a.get("nglob", NGLOB),
                                           p(obs0), p(vel), None, None, None, None, g("lists", lists), g("counts", counts), g("hold", hold),
                                           g("solve_phase", sp), a.get("limit", 9), None)

    def manipulate(B_=B, h=eng._h, **a):
        g = lambda k, v: p(a.get(k, v))
        return L.mmpc_manipulate_round_device(h, B_, g("x", x), g("tick", tick), g("phase", phase), g("U_last", U), g("pose", pose), a.get("nplan", NPLAN),
                                              g("plan", plan), None, None, p(obs0), p(vel), None, None, None, None, g("lst", lst), g("counts", mcounts),
                                              g("hold", hold), g("solve_phase", sp), a.get("limit", 9), None)

    for fn, names in ((mission, ("x", "tick", "phase", "U_last", "glob", "lists", "counts", "hold", "solve_phase")),
                      (manipulate, ("x", "tick", "phase", "U_last", "pose", "plan", "lst", "counts", "hold", "solve_phase"))):
        assert fn() == 0
        for k in names:
            assert fn(**{k: None}) == -1, k
        assert fn(limit=0) == -1 and fn(B_=257) == -1 and fn(B_=-1) == -1 and fn(h=None) == -1
        assert fn(B_=0) == 0
    assert mission(nglob=0) == -1 and manipulate(nplan=1) == -1 and manipulate(nplan=(1 << 16) + 1) == -1
    T = 5
    hist = torch.zeros((B, T, 5), dtype=torch.float64, device="cuda:0")
    ih, sh, phh, cnt = torch.zeros((B, T), **i32), torch.zeros((B, T), **i32), torch.zeros((B, T), **i32), torch.zeros(4, **i32)
    U2, status, iters = U.clone(), torch.zeros(B, **i32), torch.zeros(B, **i32)
    arrays = dict(hold=hold, solve_phase=sp, U=U2, status=status, iters=iters, tick=tick, phase=phase, U_last=U, u0=hist, ih=ih, sh=sh, ph=phh, cnt=cnt)

    def commit(B_=B, h=eng._h, set_=0, rejoin=0, T_=T, **a):
        g = lambda k: p(a.get(k, arrays[k]))
        return L.mmpc_mission_commit_device(h, B_, g("hold"), g("solve_phase"), set_, rejoin, g("U"), g("status"), g("iters"), g("tick"), g("phase"),
                                            g("U_last"), g("u0"), g("ih"), g("sh"), g("ph"), T_, g("cnt"), None)

    assert commit() == 0 and commit(set_=15, rejoin=1) == 0 and commit(B_=0) == 0
    for k in arrays:
        assert commit(**{k: None}) == -1, k
    assert commit(U_last=U2) == -1 and commit(set_=16) == -1 and commit(set_=-1) == -1 and commit(rejoin=2) == -1 and commit(T_=0) == -1
    assert commit(B_=257) == -1 and commit(h=None) == -1
    assert L.mmpc_mission_commit_device(mm.MPCBase(mm.Base(DT), [], N=15, max_batch=256)._engine._h, B, *([p(hold)] * 2), 0, 0, *([p(hold)] * 10), T,
                                        p(cnt), None) == -4
    torch.cuda.synchronize()
    assert torch.equal(x, x0) and torch.equal(phase, ph0) and (hold == R.RETIRED).all() and not hist.any()


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def _np(r):
    import torch
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in r.items()}


def _budget(r, manip):
    """min over the phases of (max iterations in that phase) - 1, from a run without a budget"""
    ph = r["phase"]
    phases = [p for p in ((0, 1, 2, 4) if manip else (0, 1, 2)) if (ph == p).any()]
    assert len(phases) == (4 if manip else 3)
    return min(int(r["iters"][ph == p].max()) for p in phases) - 1


def _fleet(mm, F, B, **kw):
    return mm.DeviceFleet(mm, F["x0"][:B], F["glob"][:B], F["obs0"][:B], F["vel"][:B], N=N, generic_budget=True, **kw)


def _same(a, r, keys, what):
    for k in keys:
        assert np.array_equal(a[k], r[k]), (what, k)


KEYS_E2E = ("u0", "iters", "status", "phase", "counts", "x", "final_phase")
KEYS_MAN = KEYS_E2E + ("mcounts", "qgoal", "ik_status", "plan")
T_MISSION, T_MANIP = 200, 220


@pytest.fixture(scope="module")
def mission(mm):
    import torch
    F = MH.mission_fleet(mm, 16, N, DT)
    fleet = _fleet(mm, F, 16)
    lock = _np(fleet.run_mission(T_MISSION))
    torch.cuda.synchronize()
    return dict(F=F, fleet=fleet, lock=lock, budget=_budget(lock, False), runs={})


@pytest.fixture(scope="module")
def manipulate(mm):
    import torch
    F = MH.mission_fleet(mm, 16, N, DT)
    fleet = _fleet(mm, F, 8)
    man = dict(pose=F["pose"][:8], t_manipulate=2)
    lock = _np(fleet.run_mission(T_MANIP, manipulate=man))
    torch.cuda.synchronize()
    return dict(F=F, fleet=fleet, man=man, lock=lock, budget=_budget(lock, True))


def _solved(r):
    return (r["phase"] < 3) | (r["phase"] == 4)


def _check_budget_run(a, lock, budget, keys, what):
    solved = _solved(lock)
    print("%s: budget %d, %d rounds, %d of %d solves suspended" % (what, budget, a["rounds"], a["suspended"], solved.sum()))
    _same(a, lock, keys, what)
    assert bool(a["all_converged"]) == bool(lock["all_converged"])
    assert a["suspended"] == (lock["iters"][solved] > budget).sum()


@pytest.mark.parametrize("sets", [2, 3])
def test_mission_under_a_budget_is_the_lock_step_per_robot(mm, mission, sets):
    import torch
    lock, b = mission["lock"], mission["budget"]
    assert (lock["final_phase"] == 3).all() and bool(lock["all_converged"])
    a = _np(mission["fleet"].run_mission(T_MISSION, budget=b, sets=sets))
    torch.cuda.synchronize()
    mission["runs"][sets] = a
    _check_budget_run(a, lock, b, KEYS_E2E, "mission, sets %d" % sets)
    assert 0 < a["suspended"] < _solved(lock).sum() and T_MISSION <= a["rounds"] <= (sets + 2) * T_MISSION + 8


def test_mission_budget_nobody_reaches(mm, mission):
    import torch
    lock = mission["lock"]
    b = int(lock["iters"].max()) + 1
    a = _np(mission["fleet"].run_mission(T_MISSION, budget=b, sets=2))
    torch.cuda.synchronize()
    _check_budget_run(a, lock, b, KEYS_E2E, "mission, budget out of reach")
    # round T retires the robots that were solved at tick T - 1; if there are none the loop sees the end after round T - 1
    assert a["suspended"] == 0 and a["rounds"] == T_MISSION + int(_solved(lock)[:, -1].any())


@pytest.mark.parametrize("sets", [2, 3])
def test_manipulate_mission_under_a_budget_is_the_lock_step_per_robot(mm, manipulate, sets):
    import torch
    lock, b = manipulate["lock"], manipulate["budget"]
    assert (lock["final_phase"] == 5).all() and (lock["ik_status"] == 0).all()
    a = _np(manipulate["fleet"].run_mission(T_MANIP, manipulate=manipulate["man"], budget=b, sets=sets))
    torch.cuda.synchronize()
    _check_budget_run(a, lock, b, KEYS_MAN, "manipulate, sets %d" % sets)
    assert 0 < a["suspended"] < _solved(lock).sum()
    if sets == 2:
        far = int(lock["iters"].max()) + 1
        c = _np(manipulate["fleet"].run_mission(T_MANIP, manipulate=manipulate["man"], budget=far, sets=2))
        torch.cuda.synchronize()
        _check_budget_run(c, lock, far, KEYS_MAN, "manipulate, budget out of reach")
        assert c["suspended"] == 0 and c["rounds"] == T_MANIP + int(_solved(lock)[:, -1].any())


def test_shifted_warm_start_under_a_budget(mm, manipulate):
    import torch
    fleet, man = manipulate["fleet"], manipulate["man"]
    lock = _np(fleet.run_mission(T_MANIP, manipulate=man, warm_start="shifted"))
    torch.cuda.synchronize()
    assert not np.array_equal(lock["iters"], manipulate["lock"]["iters"])
    b = _budget(lock, True)
    a = _np(fleet.run_mission(T_MANIP, manipulate=man, warm_start="shifted", budget=b, sets=2))
    torch.cuda.synchronize()
    _check_budget_run(a, lock, b, KEYS_MAN, "shifted")
    assert a["suspended"] > 0
    # the handles are back at the reference protocol
    again = _np(fleet.run_mission(T_MANIP, manipulate=man, budget=manipulate["budget"], sets=2))
    torch.cuda.synchronize()
    _same(again, manipulate["lock"], KEYS_MAN, "after shifted")


def test_motion_mode_under_a_budget(mm, mission):
    import torch
    b = mission["budget"]
    table = mission["runs"].get(2)
    if table is None:
        table = _np(mission["fleet"].run_mission(T_MISSION, budget=b, sets=2))
    motion = _np(_fleet(mm, mission["F"], 16, obstacles="motion").run_mission(T_MISSION, budget=b, sets=2))
    torch.cuda.synchronize()
    _same(motion, table, KEYS_E2E + ("rounds", "suspended"), "motion")
    assert motion["suspended"] > 0


def test_argument_errors(mm, mission):
    F = mission["F"]
    default = mm.DeviceFleet(mm, F["x0"][:2], F["glob"][:2], F["obs0"][:2], F["vel"][:2], N=N)
    with pytest.raises(ValueError, match="generic_budget"):
        default.run_mission(2, budget=10)
    fleet = mission["fleet"]
    for sets in (1, 5):
        with pytest.raises(ValueError, match="sets"):
            fleet.run_mission(2, budget=10, sets=sets)
    with pytest.raises(ValueError, match="on_tick"):
        fleet.run_mission(2, budget=10, on_tick=lambda t, s: None)
    with pytest.raises(ValueError, match="budget"):
        fleet.run_mission(2, budget=-1)
