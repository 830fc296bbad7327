"""GPU (MI355X): the fleet tick kernel (mmpc_tick_prepare_device) through the C ABI against its host build, and the fused /
shifted modes of DeviceFleet against the drivers that exist without them.  Bounds as in tests/test_fleet_tick_cpu.py: what
consists of copies and of correctly rounded operations is bitwise; the advanced state and the roll-out differ from numpy in
sin / cos alone, <= 4 ulp of max(1, |x_i|) per component."""
import numpy as np
import pytest

from oracle import nlp, synth

import tick_emu_helper as H

pytestmark = pytest.mark.gpu
N, M, DT = 30, 8, 0.1


def _ctrl(mm, B, **kw):
    kw.setdefault("obs_per_stage", True)
    return mm.MPCWholeBody(mm.MobileManipulator(DT), [], [], N=N, max_batch=B, n_obstacles=M, **kw)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _outputs(B, rows=None):
    import torch
    R = B if rows is None else rows
    f = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device="cuda:0")
    return dict(x_in=f(R, 9), traj_ref=f(R, N + 1, 9), start=torch.full((R,), -7, dtype=torch.int32, device="cuda:0"), obs=f(R, N + 1, M, 3),
                u_guess=f(R, N, 5), x_guess=f(R, N + 1, 9))


def _run_kernel(eng, d, want=("x_in", "traj_ref", "start", "obs", "u_guess", "x_guess"), advance=True, rows=None):
    """d: numpy inputs of H.fleet_inputs -> numpy outputs (and the advanced x, tick) of one mmpc_tick_prepare_device call"""
    import torch
    B = d["x"].shape[0]
    x, tick = _dev(d["x"]), _dev(d["tick"])
    out = _outputs(B, rows)
    kw = {k: out[k][:B] for k in want}
    eng.tick_prepare(x, tick, U_prev=_dev(d["U_prev"]) if advance else None, glob=_dev(d["glob"]), obs0=_dev(d["obs0"]), vel=_dev(d["vel"]), **kw)
    torch.cuda.synchronize()
    r = {k: v.cpu().numpy() for k, v in out.items()}
    r["x"], r["tick"] = x.cpu().numpy(), tick.cpu().numpy()
    return r


def _same_as_host_build(mm, r, h, warm=True):
    """check 1's comparison: kernel outputs r against the host build's h"""
    for k in ("start", "traj_ref", "obs", "tick", "x_in") + (("u_guess",) if warm else ()):
        assert np.array_equal(r[k], h[k]), k
    e_adv = float(H.ulp_err(r["x"], h["x"]).max())
    assert e_adv <= 4.0, e_adv
    e_roll = 0.0
    if warm:
        assert np.array_equal(r["x_guess"][:, 0], r["x_in"])
        e_roll = H.rollout_err(mm, DT, r["u_guess"], r["x_guess"])
        assert e_roll <= 4.0, e_roll
        e_host = float(H.ulp_err(r["x_guess"], h["x_guess"]).max())
        print("x_guess against the host build's: %.2f ulp (reported; the chains may drift apart over N steps)" % e_host)
    print("advance %.2f ulp against the host build, roll-out %.2f ulp step by step" % (e_adv, e_roll))


def test_kernel_against_its_host_build(mm):
    d = H.fleet_inputs()
    B = d["x"].shape[0]
    ctrl = _ctrl(mm, B)
    eng, xlim = ctrl._engine, np.asarray(ctrl.xlim, float)
    assert np.array_equal(xlim, np.asarray(nlp.WholeBodyParams(N=N).xlim, float))
    h = H.prepare(N, M, DT, xlim, **d)
    ref = H.reference(mm, xlim, DT, N, **d)
    r = _run_kernel(eng, d)
    _same_as_host_build(mm, r, h)
    assert float(H.ulp_err(r["x"], ref["x"]).max()) <= 4.0                      # and against numpy itself
    assert np.array_equal(r["start"], ref["start"]) and np.array_equal(r["obs"], ref["obs"]) and np.array_equal(r["traj_ref"], ref["traj_ref"])
    # advance only
    a = _run_kernel(eng, d, want=())
    assert np.array_equal(a["x"], r["x"]) and np.array_equal(a["tick"], r["tick"])
    assert all((a[k] == -7).all() for k in ("x_in", "traj_ref", "start", "obs", "u_guess", "x_guess"))
    # prepare only: no previous optimum - x and tick untouched, no warm start written even when its outputs are given
    p = _run_kernel(eng, d, advance=False)
    hp = H.prepare(N, M, DT, xlim, d["x"], d["tick"], None, d["glob"], d["obs0"], d["vel"])
    assert np.array_equal(p["x"], d["x"]) and np.array_equal(p["tick"], d["tick"])
    for k in ("x_in", "traj_ref", "start", "obs"):
        assert np.array_equal(p[k], hp[k]), k
    assert (p["u_guess"] == -7).all() and (p["x_guess"] == -7).all()
    # no warm-start outputs
    w = _run_kernel(eng, d, want=("x_in", "traj_ref", "start", "obs"))
    for k in ("x", "tick", "x_in", "traj_ref", "start", "obs"):
        assert np.array_equal(w[k], r[k]), k
    assert (w["u_guess"] == -7).all() and (w["x_guess"] == -7).all()


def test_rows_beyond_the_batch_are_not_written(mm):
    d = H.fleet_inputs(B=200)
    ctrl = _ctrl(mm, 256)
    full = _run_kernel(ctrl._engine, d)
    part = _run_kernel(ctrl._engine, d, rows=256)
    for k in ("x_in", "traj_ref", "start", "obs", "u_guess", "x_guess"):
        assert np.array_equal(part[k][:200], full[k]), k
        assert (part[k][200:] == -7).all(), k


def test_one_non_finite_robot_stays_alone(mm):
    d = H.fleet_inputs(B=256)
    ctrl = _ctrl(mm, 256)
    clean = _run_kernel(ctrl._engine, d)
    x = d["x"].copy(); x[77, 1] = np.nan
    r = _run_kernel(ctrl._engine, dict(d, x=x))
    assert r["start"][77] == 0 and np.isnan(r["x_in"][77, 1])
    rest = np.arange(256) != 77
    for k in clean:
        assert np.array_equal(r[k][rest], clean[k][rest]), k


def test_error_codes(mm):
    import torch
    d = H.fleet_inputs(B=32)
    ctrl = _ctrl(mm, 16)
    eng = ctrl._engine
    x, tick, glob, obs0, vel, U = (_dev(d[k]) for k in ("x", "tick", "glob", "obs0", "vel", "U_prev"))
    out = _outputs(32)
    with pytest.raises(RuntimeError, match=r"mmpc_tick_prepare_device failed \(-1\).*max_batch"):
        eng.tick_prepare(x, tick, U_prev=U)
    x, tick, glob, obs0, vel, U = (t[:16].contiguous() for t in (x, tick, glob, obs0, vel, U))
    x_before = x.clone()
    with pytest.raises(RuntimeError, match=r"\(-1\).*d_glob"):
        eng.tick_prepare(x, tick, traj_ref=out["traj_ref"][:16])
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        eng.tick_prepare(x, tick, glob=glob[:, :0].contiguous(), traj_ref=out["traj_ref"][:16])                  # nglob = 0
    with pytest.raises(RuntimeError, match=r"\(-1\).*d_obs0"):
        eng.tick_prepare(x, tick, obs=out["obs"][:16], obs0=obs0)
    with pytest.raises(ValueError, match="tick is required"):
        eng.tick_prepare(x, None, U_prev=U)
    with pytest.raises(ValueError, match="traj_ref must be"):
        eng.tick_prepare(x, tick, glob=glob, traj_ref=out["traj_ref"][:16, :N])
    with pytest.raises(ValueError, match="must not be U_prev"):
        eng.tick_prepare(x, tick, U_prev=U, u_guess=U, x_guess=out["x_guess"][:16])
    eng.tick_prepare(x[:0], tick[:0], U_prev=U[:0])                                                              # B = 0: a no-op
    torch.cuda.synchronize()
    assert torch.equal(x, x_before)
    static = _ctrl(mm, 16, obs_per_stage=False)
    with pytest.raises(RuntimeError, match=r"\(-4\).*obs_per_stage"):
        static._engine.tick_prepare(x, tick, U_prev=U)
    base = mm.MPCBase(mm.Base(DT), [], N=15, max_batch=16)
    with pytest.raises(RuntimeError, match=r"\(-4\)"):
        base._engine.tick_prepare(x, tick)


def _c5_fleet(mm, B=1024, **kw):
    import torch
    d = synth.make_batch(B, N=N, M=M, config_id=5, moving=True)
    par = nlp.WholeBodyParams(N=N)
    glob = _dev(H.straight_plan(d["traj_ref"], N))
    x0 = np.clip(d["x_init"], par.xlim[0], par.xlim[1])
    return mm.DeviceFleet(mm, x0, glob, d["obs"], d["obs_vel"], N=N, **kw), d, x0


def test_fleet_argument_errors(mm):
    with pytest.raises(ValueError, match="needs fused=True"):
        _c5_fleet(mm, 8, warm_start="shifted")
    with pytest.raises(ValueError, match="warm_start must be"):
        _c5_fleet(mm, 8, fused=True, warm_start="cold")
    fleet, _, _ = _c5_fleet(mm, 8, fused=True)
    with pytest.raises(ValueError, match="no fused form"):
        fleet.run_async(2)


def test_fused_tick_zero_is_bitwise_the_unfused(mm):
    import torch
    a = _c5_fleet(mm)[0].run_lockstep(1)
    b = _c5_fleet(mm, fused=True)[0].run_lockstep(1)
    torch.cuda.synchronize()
    assert bool(a["all_converged"]) and bool(b["all_converged"])
    assert torch.equal(a["u0"], b["u0"]) and torch.equal(a["iters"], b["iters"])


@pytest.mark.parametrize("warm_start", ["reference", "shifted"])
def test_fused_lock_step_equals_fused_groups(mm, warm_start):
    import torch
    T = 6
    fleet = _c5_fleet(mm, fused=True, warm_start=warm_start)[0]
    a = fleet.run_lockstep(T)
    torch.cuda.synchronize()
    assert bool(a["all_converged"])
    a = {k: v.clone() for k, v in a.items() if torch.is_tensor(v)}
    for G in (2, 3):
        g = fleet.run_groups(T, groups=G)
        torch.cuda.synchronize()
        assert bool(g["all_converged"]) and g["groups"] == G
        assert torch.equal(a["u0"], g["u0"]) and torch.equal(a["x"], g["x"]) and torch.equal(a["iters"], g["iters"]), (warm_start, G)


def test_fused_against_unfused_over_six_ticks(mm):
    """After the first plant step the fused and the torch driver may differ in the last bit of sin / cos, and six ticks of an
    interior-point loop carry that on.  The yardstick is the same effect between two drivers that exist without the tick
    kernel: DeviceFleet.run_lockstep (torch glue on the GPU) and BatchedRecedingHorizon (numpy glue on the host) - E0 = max |du0|
    between them, A0 = their share of (robot, tick) pairs with equal iteration counts.  Required of the fused driver against
    run_lockstep: max |du0| <= 10 max(E0, 1e-9) (E0 is one draw of a maximum over 6144 solves of the same mechanism) and an
    equal-iteration share >= A0 - 0.01; every solve of all three converged."""
    import torch
    T, B = 6, 1024
    fleet, d, x0 = _c5_fleet(mm)
    a = fleet.run_lockstep(T)
    f = _c5_fleet(mm, fused=True)[0].run_lockstep(T)
    torch.cuda.synchronize()
    ctrl = _ctrl(mm, B)
    brh = mm.BatchedRecedingHorizon(ctrl, x0, x0, obs=d["obs"], obs_vel=d["obs_vel"])
    brh.traj_ref = H.straight_plan(d["traj_ref"], N); brh.u_ref = np.zeros((B, 50, 5))
    _, u_host = brh.run(T)                                                   # raises when a solve does not converge
    it_host = np.array(brh.iters_log).T
    u_a, it_a = a["u0"].cpu().numpy(), a["iters"].cpu().numpy()
    u_f, it_f = f["u0"].cpu().numpy(), f["iters"].cpu().numpy()
    E0 = float(np.abs(u_a - np.transpose(u_host, (1, 0, 2))).max()); A0 = float((it_a == it_host).mean())
    E1 = float(np.abs(u_f - u_a).max()); A1 = float((it_f == it_a).mean())
    Ex = float(np.abs(f["x"].cpu().numpy() - a["x"].cpu().numpy()).max())
    msg = "torch glue against numpy glue: E0 = %.3e, A0 = %.4f; fused against torch glue: max |du0| = %.3e, equal iterations %.4f, max |dx| = %.3e, bitwise %s" % (
        E0, A0, E1, A1, Ex, bool(np.array_equal(u_f, u_a)))
    print(msg)
    assert bool(a["all_converged"]) and bool(f["all_converged"]), msg
    assert E1 <= 10 * max(E0, 1e-9), msg
    assert A1 >= A0 - 0.01, msg


def test_shifted_warm_start_of_the_fleet(mm):
    import torch
    T, B = 6, 1024
    fleet, d, x0 = _c5_fleet(mm, fused=True, warm_start="shifted")
    ref = _c5_fleet(mm, fused=True)[0].run_lockstep(T)
    seen = {}

    def on_tick(t, u0):
        # after tick 1's solve is queued: the guess it started from, and tick 0's optimum it was built from (the other output set)
        if t == 1:
            seen.update(ug=fleet._fin["ug"].clone(), xg=fleet._fin["xg"].clone(), U0=fleet._fsets[0]["U"].clone(), x_in=fleet._fin["x_in"].clone())

    res = {}
    for _ in fleet._lockstep_ticks(T, res, on_tick):
        pass
    torch.cuda.synchronize()
    assert bool(res["all_converged"]) and bool(ref["all_converged"])
    # the u_guess / x_guess handed to tick 1 are the kernel test's definitions for the fleet's own state
    h = H.prepare(N, M, DT, np.asarray(fleet.ctrls[0].xlim, float), x0, np.zeros(B, np.int64), seen["U0"].cpu().numpy(), fleet.glob.cpu().numpy(),
                  d["obs"], d["obs_vel"])
    ug, xg = seen["ug"].cpu().numpy(), seen["xg"].cpu().numpy()
    assert np.array_equal(ug, h["u_guess"]) and np.array_equal(seen["x_in"].cpu().numpy(), h["x_in"]) and np.array_equal(xg[:, 0], h["x_in"])
    e_roll = H.rollout_err(mm, DT, ug, xg)
    assert e_roll <= 4.0, e_roll
    m_s = float(res["iters"][:, 1:].double().mean()); m_r = float(ref["iters"][:, 1:].double().mean())
    print("mean iterations over ticks 1..%d: shifted %.2f, reference %.2f, ratio %.3f" % (T - 1, m_s, m_r, m_s / m_r))
    assert m_s < m_r, (m_s, m_r)
    # the handle's warm start was put back: a plain solve on it is bitwise that of a fresh handle
    eng = fleet.engs[0]
    loc, obs = fleet.inputs(fleet.x0, torch.zeros(B, dtype=torch.int64, device=fleet.dev))
    zero = torch.zeros((B, N, 5), dtype=torch.float64, device=fleet.dev)
    o1 = eng.solve_batch_device(fleet.x0, loc, fleet.uref, zero, obs)
    o2 = _ctrl(mm, B)._engine.solve_batch_device(fleet.x0, loc, fleet.uref, zero, obs)
    torch.cuda.synchronize()
    for k in ("X", "U", "s", "status", "iters", "cost"):
        assert torch.equal(o1[k], o2[k]), k
    # and on an exception inside a run as well
    def boom(t, u0):
        if t == 2:
            raise KeyError("stop")
    with pytest.raises(KeyError):
        for _ in fleet._lockstep_ticks(T, {}, boom):
            pass
    o3 = eng.solve_batch_device(fleet.x0, loc, fleet.uref, zero, obs)
    torch.cuda.synchronize()
    assert torch.equal(o3["U"], o2["U"]) and torch.equal(o3["iters"], o2["iters"])
