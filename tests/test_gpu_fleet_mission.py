"""GPU (MI355X): the fleet mission kernel (mmpc_mission_prepare_device) through the C ABI against its host build, the list launch
for either kernel family (mmpc_solve_rows_device), and DeviceFleet.run_mission.  Bounds as in tests/test_fleet_mission_cpu.py:
everything is bitwise - the kernel against its host build (same source, every operation rounded on its own, exact fmod), a listed
row against the same row of a whole-batch launch (results never depend on which workgroup solves an instance), a robot in a fleet
against the same robot alone (robots do not interact).  The one place where two sides may differ is a threshold comparison replayed
in numpy inside 1e-9 of the threshold; the share of such (robot, tick) pairs is bounded."""
import ctypes as C

import numpy as np
import pytest

from oracle import nlp, synth

import mission_emu_helper as H
import tick_emu_helper as TH

pytestmark = pytest.mark.gpu
N, M, DT, NGLOB = 20, 3, 0.1, 31
KEYS = ("x_in", "traj_ref", "start", "obs")


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _ctrl(mm, B, n=N, m=M, **kw):
    kw.setdefault("obs_per_stage", True)
    return mm.MPCWholeBody(mm.MobileManipulator(DT), [], [], N=n, max_batch=B, n_obstacles=m, **kw)


def _run_kernel(eng, d, rows=None, motion=False, advance=True):
    """d: numpy inputs of H.branch_inputs -> numpy outputs of one mmpc_mission_prepare_device call (buffers of `rows` rows)"""
    import torch
    B = d["x"].shape[0]
    R = B if rows is None else rows
    f = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device="cuda:0")
    out = dict(x_in=f(R, 9), traj_ref=f(R, N + 1, 9), start=torch.full((R,), -7, dtype=torch.int32, device="cuda:0"), obs=f(R, N + 1, M, 3))
    x, tick, phase = _dev(d["x"]), _dev(d["tick"]), _dev(d["phase"])
    lists = torch.full((3, B), -7, dtype=torch.int32, device="cuda:0"); counts = torch.full((4,), -7, dtype=torch.int32, device="cuda:0")
    kw = {k: out[k][:B] for k in KEYS if not (motion and k == "obs")}
    if not motion:
        kw.update(obs0=_dev(d["obs0"]), vel=_dev(d["vel"]))
    eng.mission_prepare(x, tick, phase, lists, counts, U_prev=_dev(d["U_prev"]) if advance else None, glob=_dev(d["glob"]), **kw)
    torch.cuda.synchronize()
    r = {k: v.cpu().numpy() for k, v in out.items()}
    r.update(x=x.cpu().numpy(), tick=tick.cpu().numpy(), phase=phase.cpu().numpy(), lists=lists.cpu().numpy(), counts=counts.cpu().numpy())
    return r


def _same(r, h, keys):
    for k in keys + ("x", "tick", "phase", "counts"):
        assert np.array_equal(r[k], h[k], equal_nan=True), k
    for p in range(3):
        n = int(h["counts"][p])
        assert np.array_equal(np.sort(r["lists"][p, :n]), np.sort(h["lists"][p, :n])), p
        assert (r["lists"][p, n:] == -7).all(), p


def test_kernel_against_its_host_build(mm):
    d, _ = H.branch_inputs(512, N, M, NGLOB)
    table, motion = _ctrl(mm, 512), _ctrl(mm, 512, obs_per_stage="motion")
    xlim = np.asarray(table.xlim, float)
    assert np.array_equal(xlim, np.asarray(nlp.WholeBodyParams(N=N).xlim, float))
    for advance in (True, False):
        h = H.prepare(N, M, DT, xlim, **(d if advance else dict(d, U_prev=None)))
        _same(_run_kernel(table._engine, d, advance=advance), h, KEYS)
        r = _run_kernel(motion._engine, d, motion=True, advance=advance)
        _same(r, h, ("x_in", "traj_ref", "start"))
        assert (r["obs"] == -7).all()


def test_rows_beyond_the_batch_are_not_written_and_error_codes(mm):
    import torch
    d, _ = H.branch_inputs(200, N, M, NGLOB)
    ctrl = _ctrl(mm, 256)
    eng = ctrl._engine
    full = _run_kernel(eng, d)
    part = _run_kernel(eng, d, rows=256)
    for k in KEYS:
        assert np.array_equal(part[k][:200], full[k]), k
        assert (part[k][200:] == -7).all(), k
    x, tick, phase, glob, obs0, vel, U = (_dev(d[k]) for k in ("x", "tick", "phase", "glob", "obs0", "vel", "U_prev"))
    lists = torch.zeros((3, 200), dtype=torch.int32, device="cuda:0"); counts = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    obs = torch.zeros((200, N + 1, M, 3), dtype=torch.float64, device="cuda:0")
    base = mm.MPCBase(mm.Base(DT), [], N=15, max_batch=256)
    with pytest.raises(RuntimeError, match=r"mmpc_mission_prepare_device failed \(-4\)"):
        base._engine.mission_prepare(x, tick, phase, lists, counts, glob=glob)
    with pytest.raises(RuntimeError, match=r"\(-4\).*obs_per_stage"):
        _ctrl(mm, 256, obs_per_stage=False)._engine.mission_prepare(x, tick, phase, lists, counts, glob=glob)
    with pytest.raises(RuntimeError, match=r"\(-1\).*d_obs must be NULL"):
        _ctrl(mm, 256, obs_per_stage="motion")._engine.mission_prepare(x, tick, phase, lists, counts, glob=glob, obs0=obs0, vel=vel, obs=obs)
    with pytest.raises(RuntimeError, match=r"\(-1\).*max_batch"):
        _ctrl(mm, 100)._engine.mission_prepare(x, tick, phase, lists, counts, glob=glob)
    for name in ("phase", "lists", "counts", "glob"):
        with pytest.raises(ValueError, match="%s is required" % name):
            eng.mission_prepare(x, tick, **dict(dict(phase=phase, lists=lists, counts=counts, glob=glob), **{name: None}))
    # ... and the C entry point itself, which the wrapper's checks keep such calls from
    fn = mm._capi.lib().mmpc_mission_prepare_device
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    x_before = x.clone()
    for miss in ("phase", "lists", "counts", "glob"):
        a = dict(phase=phase, lists=lists, counts=counts, glob=glob); a[miss] = None
        rc = fn(eng._h, 200, p(x), p(tick), p(a["phase"]), p(U), p(a["glob"]), NGLOB, p(obs0), p(vel), None, None, None, None, p(a["lists"]), p(a["counts"]), None)
        assert rc == -1, (miss, rc)
    torch.cuda.synchronize()
    assert torch.equal(x, x_before)


def _batch(B, n, m, dev):
    import torch
    d = synth.make_batch(B, N=n, M=m)
    par = nlp.WholeBodyParams(N=n)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return (t(np.clip(d["x_init"], par.xlim[0], par.xlim[1])), t(d["traj_ref"]), t(d["u_ref"]), torch.zeros((B, n, 5), dtype=torch.float64, device=dev),
            t(d["obs"]))


@pytest.mark.parametrize("terminal", [False, True], ids=["plain", "terminal_xy_equality"])
def test_rows_launch_on_the_generic_kernel(mm, terminal):
    import torch
    B, n, m = 64, 12, 2
    dev = torch.device("cuda", 0)
    ctrl = _ctrl(mm, B, n, m, obs_per_stage=False)
    eng = ctrl._engine
    if terminal:
        ctrl.opti.subject_to(ctrl.X[n, :2] == ctrl.X_ref[n, :2])
    assert not eng.runs_specialised
    xi, tr, ur, ul, ob = _batch(B, n, m, dev)
    if terminal:
        # a reference the equality can be met from: hold the point half a metre ahead of the start (the plan's row N is out of
        # reach of most starts within N = 12 stages)
        tr = xi[:, None, :].repeat(1, n + 1, 1)
        tr[:, :, 0] += 0.5 * torch.cos(xi[:, 2])[:, None]; tr[:, :, 1] += 0.5 * torch.sin(xi[:, 2])[:, None]; tr[:, :, 3:6] = 0
        tr = tr.contiguous()
    ref = {k: v.clone() for k, v in eng.solve_batch_device(xi, tr, ur, ul, ob).items()}
    torch.cuda.synchronize()
    assert int((ref["status"] == 0).sum()) >= B // 2
    blank = lambda: {k: torch.full_like(v, -7) for k, v in ref.items()}

    def launch(entries, count=None):
        lst = torch.zeros(B, dtype=torch.int32, device=dev); lst[:len(entries)] = torch.tensor(entries, dtype=torch.int32, device=dev)
        cnt = torch.tensor([len(entries) if count is None else count], dtype=torch.int32, device=dev)
        out = blank()
        eng.solve_rows_device((lst, cnt), xi, tr, ur, ul, ob, out)
        torch.cuda.synchronize()
        return out

    def check(out, sel):
        rest = torch.ones(B, dtype=torch.bool, device=dev); rest[sel] = False
        for k in ("X", "U", "s", "status", "iters", "cost", "err"):
            assert torch.equal(out[k][sel], ref[k][sel]), k
            assert bool((out[k][rest] == -7).all()), k

    check(launch([5, 60, 17, 33, 1, 63, 0]), [5, 60, 17, 33, 1, 63, 0])
    assert all(bool((v == -7).all()) for v in launch([5, 60, 17], count=0).values())          # an empty list touches nothing
    check(launch([5, -1, B, 2 ** 30, 17]), [5, 17])                                            # entries outside the batch are skipped
    # the list launch of the specialised kernels still refuses this handle
    lst = torch.zeros(B, dtype=torch.int32, device=dev); cnt = torch.ones(1, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match=r"mmpc_solve_list_device failed \(-4\).*list launches need a specialised kernel"):
        eng.solve_batch_device(xi, tr, ur, ul, ob, out=blank(), rows=(lst, cnt))


def test_rows_launch_on_a_specialised_handle_is_the_list_launch(mm):
    import torch
    B, n, m = 64, 20, 5
    dev = torch.device("cuda", 0)
    eng = _ctrl(mm, B, n, m, obs_per_stage=False)._engine
    assert eng.runs_specialised
    xi, tr, ur, ul, ob = _batch(B, n, m, dev)
    lst = torch.zeros(B, dtype=torch.int32, device=dev); lst[:5] = torch.tensor([9, 63, 0, 31, 32], dtype=torch.int32, device=dev)
    cnt = torch.tensor([5], dtype=torch.int32, device=dev)
    mk = lambda: dict(X=torch.full((B, n + 1, 9), -7.0, dtype=torch.float64, device=dev), U=torch.full((B, n, 5), -7.0, dtype=torch.float64, device=dev),
                      s=torch.full((B, n + 1), -7.0, dtype=torch.float64, device=dev), status=torch.full((B,), -7, dtype=torch.int32, device=dev),
                      iters=torch.full((B,), -7, dtype=torch.int32, device=dev), cost=torch.full((B,), -7.0, dtype=torch.float64, device=dev),
                      err=torch.full((B,), -7.0, dtype=torch.float64, device=dev))
    a, b = mk(), mk()
    eng.solve_batch_device(xi, tr, ur, ul, ob, out=a, rows=(lst, cnt))
    eng.solve_rows_device((lst, cnt), xi, tr, ur, ul, ob, b)
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert bool((a["status"][[9, 63, 0, 31, 32]] == 0).all()) and int((a["status"] == -7).sum()) == B - 5
    eng.set_iteration_budget(12)
    with pytest.raises(RuntimeError, match=r"mmpc_solve_rows_device failed \(-4\).*budget"):
        eng.solve_rows_device((lst, cnt), xi, tr, ur, ul, ob, b)
    eng.set_iteration_budget(0)


def test_all_move_fleet_is_the_fused_fleet(mm):
    """The C5 fleet of tests/test_gpu_fleet_tick.py: no robot comes inside the box around its goal within the run, so a mission is
    the fused lock step - one list launch of all rows on the move handle per tick."""
    import torch
    n, m, B, T = 30, 8, 256, 4
    d = synth.make_batch(B, N=n, M=m, config_id=5, moving=True)
    par = nlp.WholeBodyParams(N=n)
    glob = _dev(TH.straight_plan(d["traj_ref"], n))
    x0 = np.clip(d["x_init"], par.xlim[0], par.xlim[1])
    a = mm.DeviceFleet(mm, x0, glob, d["obs"], d["obs_vel"], N=n, fused=True).run_lockstep(T)
    r = mm.DeviceFleet(mm, x0, glob, d["obs"], d["obs_vel"], N=n).run_mission(T)
    torch.cuda.synchronize()
    assert bool((r["phase"] == 0).all()) and bool((r["final_phase"] == 0).all())
    assert bool((r["counts"] == torch.tensor([B, 0, 0, 0], dtype=torch.int32, device=r["counts"].device)).all())
    assert bool(a["all_converged"]) and bool(r["all_converged"])
    assert torch.equal(a["u0"], r["u0"]) and torch.equal(a["x"], r["x"]) and torch.equal(a["iters"], r["iters"])


T_MISSION = 200


@pytest.fixture(scope="module")
def mission(mm):
    """the fleet of 16 of H.mission_fleet, run once for T_MISSION ticks, with every tick's inputs, states and U rows logged"""
    import torch
    F = H.mission_fleet(mm, 16, N, DT)
    fleet = mm.DeviceFleet(mm, F["x0"], F["glob"], F["obs0"], F["vel"], N=N)
    log = []

    def on_tick(t, s):
        log.append({k: s[k].clone() for k in ("x", "x_in", "loc", "obs", "u_last", "U")})

    res = fleet.run_mission(T_MISSION, streams=1, on_tick=on_tick)
    torch.cuda.synchronize()
    return dict(F=F, fleet=fleet, log=log, res={k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in res.items()})


def test_mission_end_to_end(mm, mission):
    import torch
    F, fleet, log, r = mission["F"], mission["fleet"], mission["log"], mission["res"]
    B, T = 16, T_MISSION
    ph = r["phase"]
    assert fleet.engs[0].runs_specialised and not fleet._mission_ctrls[1]._engine.runs_specialised
    ticks = [[int((ph[b] == p).sum()) for p in range(3)] for b in range(B)]
    print("ticks in move / approach / rotate per robot:", ticks)
    assert (ph[:, -1] == 3).all() and (r["final_phase"] == 3).all(), ph[:, -1]
    assert bool(r["all_converged"]) and (r["status"] == 0).all()
    assert (np.diff(ph, axis=1) >= 0).all()
    assert all(min(tk) >= 1 for tk in ticks)                                      # every robot passes through every phase
    assert np.array_equal(r["counts"], np.stack([(ph == p).sum(axis=0) for p in range(4)], axis=1))
    solved = ph < 3
    assert (r["iters"][solved] > 0).all() and (r["iters"][~solved] == 0).all() and (r["u0"][~solved] == 0).all()
    # the goal is reached as the state machine defines it
    g = F["glob"][:, -1]
    assert (np.hypot(r["x"][:, 0] - g[:, 0], r["x"][:, 1] - g[:, 1]) <= 0.01).all()
    # replay of the numpy state machine on the logged states
    X = np.stack([l["x"].cpu().numpy() for l in log], axis=1)                    # (B, T, 9): the state tick t's state machine saw
    pairs = inside = 0
    for b in range(B):
        prev = H.MOVE
        for t in range(T):
            if prev == H.DONE:
                assert ph[b, t] == H.DONE and np.array_equal(X[b, t], X[b, t - 1])
                continue
            pairs += 1
            if np.abs(H.quantities(mm, X[b, t], g[b])).min() >= 1e-9:
                assert H.state_machine(mm, X[b, t], g[b], prev) == ph[b, t], (b, t)
            else:
                inside += 1
            prev = int(ph[b, t])
    print("(robot, tick) pairs inside 1e-9 of a threshold: %d of %d" % (inside, pairs))
    assert inside <= 0.02 * pairs, (inside, pairs)
    # robot 0, first tick of each phase: the logged U row is that of a whole-batch solve of the tick's inputs on the phase's handle
    for p in range(3):
        t = int(np.argmax(ph[0] == p))
        l = log[t]
        eng = fleet._mission_ctrls[p]._engine
        o = eng.solve_batch_device(l["x_in"], l["loc"], fleet.uref, l["u_last"], l["obs"])
        torch.cuda.synchronize()
        assert torch.equal(o["U"][0], l["U"][0]), (p, t)
        assert np.array_equal(o["U"][0, 0].cpu().numpy(), r["u0"][0, t])


def test_robots_do_not_interact_and_streams_do_not_matter(mm, mission):
    import torch
    F, r = mission["F"], mission["res"]
    for b in range(4):
        one = mm.DeviceFleet(mm, F["x0"][b:b + 1], F["glob"][b:b + 1], F["obs0"][b:b + 1], F["vel"][b:b + 1], N=N).run_mission(T_MISSION)
        torch.cuda.synchronize()
        for k in ("u0", "iters", "phase", "x"):
            assert np.array_equal(one[k].cpu().numpy()[0], r[k][b]), (b, k)
    s3 = mission["fleet"].run_mission(T_MISSION, streams=3)
    torch.cuda.synchronize()
    for k in ("u0", "iters", "status", "phase", "counts", "x", "final_phase"):
        assert np.array_equal(s3[k].cpu().numpy(), r[k]), k


def test_mission_argument_errors(mm):
    F = H.mission_fleet(mm, 2, N, DT)
    with pytest.raises(ValueError, match="shifted"):
        mm.DeviceFleet(mm, F["x0"], F["glob"], F["obs0"], F["vel"], N=N, fused=True, warm_start="shifted").run_mission(2)
    with pytest.raises(ValueError, match="streams must be"):
        mm.DeviceFleet(mm, F["x0"], F["glob"], F["obs0"], F["vel"], N=N).run_mission(2, streams=2)
