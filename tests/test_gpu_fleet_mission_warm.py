"""GPU (MI355X): the mission's warm-start kernel (mmpc_shift_guess_device) through the C ABI against its host build and against the
tick kernel on the same device, and DeviceFleet.run_mission(warm_start="shifted") end to end.  Bounds as in
tests/test_fleet_guess_cpu.py: the shift is a copy (bitwise against the host build); the roll-out is held step by step to <= 4 ulp
against the package's f_kinematics on the device's own previous stage; against mmpc_tick_prepare_device on the same device and the
same x_in both outputs are bitwise (the same functions, no contraction).  A warm-started solve and a cold one of the same inputs solve
the same NLP to 1e-8: |dcost| <= 1e-6 max(1, |cost_cold|), with at most 2 % of the compared solves allowed to miss (device rounding
on 'rotate' costs near zero; the CPU oracle misses on none)."""
import ctypes as C

import numpy as np
import pytest

import guess_emu_helper as G
import mission_emu_helper as MH
import tick_emu_helper as TH

pytestmark = pytest.mark.gpu
N, M, DT = 20, 3, 0.1


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _ctrl(mm, B, n=N, m=M, **kw):
    kw.setdefault("obs_per_stage", True)
    return mm.MPCWholeBody(mm.MobileManipulator(DT), [], [], N=n, max_batch=B, n_obstacles=m, **kw)


def _sentinel(*s):
    import torch
    return torch.full(s, -7.0, dtype=torch.float64, device="cuda:0")


@pytest.mark.parametrize("n,m", [(20, 3), (30, 8)])
def test_entry_point_against_host_build_and_tick_kernel(mm, n, m):
    import torch
    B = 256
    d = TH.fleet_inputs(B=B, N=n, M=m)
    eng = _ctrl(mm, B, n, m)._engine
    ph = np.random.default_rng(2).integers(-1, 7, B).astype(np.int32)
    solved = np.isin(ph, G.SOLVED)
    assert np.bincount(ph + 1, minlength=8).min() >= 8
    # the tick kernel on the same device: its x_in is this call's input, its guess what this call has to write
    x, tick, U = _dev(d["x"]), _dev(d["tick"]), _dev(d["U_prev"])
    x_in, ug_t, xg_t = _sentinel(B, 9), _sentinel(B, n, 5), _sentinel(B, n + 1, 9)
    eng.tick_prepare(x, tick, U_prev=U, x_in=x_in, u_guess=ug_t, x_guess=xg_t)
    ug, xg = _sentinel(B, n, 5), _sentinel(B, n + 1, 9)
    eng.shift_guess(_dev(ph), U, x_in, ug, xg)
    ug_all, xg_all = _sentinel(B, n, 5), _sentinel(B, n + 1, 9)
    eng.shift_guess(None, U, x_in, ug_all, xg_all)
    torch.cuda.synchronize()
    x_in, ug_t, xg_t, ug, xg, ug_all, xg_all = (a.cpu().numpy() for a in (x_in, ug_t, xg_t, ug, xg, ug_all, xg_all))
    assert not (ug_t == -7).any() and not (xg_t == -7).any()
    assert np.array_equal(ug_all, ug_t) and np.array_equal(xg_all, xg_t)
    assert np.array_equal(ug[solved], ug_t[solved]) and np.array_equal(xg[solved], xg_t[solved])
    assert (ug[~solved] == -7).all() and (xg[~solved] == -7).all()
    hu, hx = G.shift(n, DT, d["U_prev"], x_in, ph)
    assert np.array_equal(ug, hu)
    assert np.array_equal(xg[:, 0][solved], x_in[solved])
    e_roll = TH.rollout_err(mm, DT, ug[solved], xg[solved])
    print("N = %d: roll-out %.2f ulp; x_guess against the host build: %.2f ulp, bitwise %s" % (
        n, e_roll, float(TH.ulp_err(xg[solved], hx[solved]).max()), np.array_equal(xg, hx)))
    assert e_roll <= 4.0, e_roll


def test_rows_beyond_the_batch_are_not_written_and_error_codes(mm):
    import torch
    B = 200
    d = TH.fleet_inputs(B=B, N=N, M=M)
    eng = _ctrl(mm, 256)._engine
    U, x_in = _dev(d["U_prev"]), _dev(np.clip(d["x"], -2, 2))
    ug, xg = _sentinel(B, N, 5), _sentinel(B, N + 1, 9)
    eng.shift_guess(None, U, x_in, ug, xg)
    big_u, big_x = _sentinel(256, N, 5), _sentinel(256, N + 1, 9)
    eng.shift_guess(None, U, x_in, big_u[:B], big_x[:B])
    torch.cuda.synchronize()
    assert torch.equal(big_u[:B], ug) and torch.equal(big_x[:B], xg) and not (ug == -7).any()
    assert bool((big_u[B:] == -7).all()) and bool((big_x[B:] == -7).all())
    # the wrapper
    with pytest.raises(ValueError, match="u_guess must not be U_prev"):
        eng.shift_guess(None, U, x_in, U, xg)
    for name in ("U_prev", "x_in", "u_guess", "x_guess"):
        kw = dict(U_prev=U, x_in=x_in, u_guess=ug, x_guess=xg)
        kw[name] = None
        with pytest.raises(ValueError, match="%s is required" % name):
            eng.shift_guess(None, **kw)
    with pytest.raises(ValueError, match="phase must be"):
        eng.shift_guess(torch.zeros(B, dtype=torch.int64, device="cuda:0"), U, x_in, ug, xg)
    with pytest.raises(ValueError, match="x_guess must be"):
        eng.shift_guess(None, U, x_in, ug, xg[:, :N].contiguous())
    base = mm.MPCBase(mm.Base(DT), [], N=15, max_batch=256)
    with pytest.raises(RuntimeError, match=r"mmpc_shift_guess_device failed \(-4\)"):
        base._engine.shift_guess(None, U[:, :15].contiguous(), x_in, _sentinel(B, 15, 5), _sentinel(B, 16, 9))
    with pytest.raises(RuntimeError, match=r"\(-1\).*max_batch"):
        _ctrl(mm, 100)._engine.shift_guess(None, U, x_in, ug, xg)
    # no requirement on the obstacle layout
    plain = _ctrl(mm, 256, obs_per_stage=False)._engine
    ug2, xg2 = _sentinel(B, N, 5), _sentinel(B, N + 1, 9)
    plain.shift_guess(None, U, x_in, ug2, xg2)
    torch.cuda.synchronize()
    assert torch.equal(ug2, ug) and torch.equal(xg2, xg)
    # ... and the C entry point itself, which the wrapper's checks keep such calls from
    fn = mm._capi.lib().mmpc_shift_guess_device
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    req = dict(U=U, x_in=x_in, ug=ug, xg=xg)
    call = lambda a, B_=B, h=eng._h: fn(h, B_, None, p(a["U"]), p(a["x_in"]), p(a["ug"]), p(a["xg"]), None)
    before_u, before_x = ug.clone(), xg.clone()
    for miss in req:
        assert call(dict(req, **{miss: None})) == -1, miss
    assert call(dict(req, ug=U)) == -1
    assert call(req, B_=257) == -1 and call(req, B_=-1) == -1
    assert call(req, h=base._engine._h) == -4
    assert call(req, h=None) == -1
    ug.fill_(-7); xg.fill_(-7)
    assert call(req, B_=0) == 0                      # a no-op
    torch.cuda.synchronize()
    assert bool((ug == -7).all()) and bool((xg == -7).all())
    assert call(req) == 0
    torch.cuda.synchronize()
    assert torch.equal(ug, before_u) and torch.equal(xg, before_x)


# ---- missions -------------------------------------------------------------------------------------------------------------------
CASES = {"drive": (200, False), "manipulate": (220, True)}
LOGGED = ("x", "phase", "x_in", "loc", "obs", "u_last", "U", "u_guess", "x_guess")
KEYS = ("u0", "iters", "status", "phase", "x", "final_phase", "counts")


def _np(r):
    import torch
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in r.items()}


def _fleet(mm, F, rows=slice(None)):
    return mm.DeviceFleet(mm, F["x0"][rows], F["glob"][rows], F["obs0"][rows], F["vel"][rows], N=N)


@pytest.fixture(scope="module")
def missions(mm):
    """the fleet of 16 of MH.mission_fleet, per case run once under the reference protocol and once with warm_start="shifted", every
    tick of the latter logged (with the cost of its solves, from the output set of the tick)"""
    import torch
    F = MH.mission_fleet(mm, 16, N, DT)
    fleet = _fleet(mm, F)
    out = dict(F=F, fleet=fleet)
    for name, (T, manip) in CASES.items():
        kw = dict(manipulate=dict(pose=F["pose"], t_manipulate=2)) if manip else {}
        ref = fleet.run_mission(T, streams=1, **kw)
        torch.cuda.synchronize()
        log = []

        def on_tick(t, s):
            l = {k: s[k].clone() for k in LOGGED}
            l["cost"] = fleet._msets[t & 1]["cost"].clone()
            log.append(l)

        warm = fleet.run_mission(T, streams=1, on_tick=on_tick, warm_start="shifted", **kw)
        torch.cuda.synchronize()
        out[name] = dict(T=T, kw=kw, ref=_np(ref), warm=_np(warm), log=[_np(l) for l in log])
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_mission_with_the_shifted_warm_start(mm, missions, case):
    import torch
    F, c = missions["F"], missions[case]
    T, manip = CASES[case]
    ref, warm, log = c["ref"], c["warm"], c["log"]
    B, last = 16, 5 if manip else 3
    assert set(ref) == set(warm) and len(log) == T
    # tick 0 is the reference protocol's, bit for bit
    for k in ("u0", "iters", "status", "phase"):
        assert np.array_equal(warm[k][:, 0], ref[k][:, 0]), k
    assert np.array_equal(warm["counts"][0], ref["counts"][0])
    for r in (ref, warm):
        assert (r["final_phase"] == last).all() and (r["phase"][:, -1] == last).all(), r["final_phase"]
        assert bool(r["all_converged"]) and (r["status"] == 0).all()
    ph = warm["phase"]
    solved = np.isin(ph, G.SOLVED)
    assert np.array_equal(solved, (ph < 3) | (ph == 4))
    # the logged guesses of the solved robots are the host build's on the logged inputs
    ugs, xgs = [], []
    for t in range(1, T):
        l, rows = log[t], solved[:, t]
        assert np.array_equal(l["phase"], ph[:, t])
        if not rows.any():
            continue
        hu, hx = G.shift(N, DT, l["u_last"], l["x_in"], l["phase"])
        assert np.array_equal(l["u_guess"][rows], hu[rows]), t
        assert np.array_equal(l["x_guess"][rows, 0], l["x_in"][rows]), t
        assert np.array_equal(l["u_last"][rows], log[t - 1]["U"][rows]), t
        ugs.append(l["u_guess"][rows]); xgs.append(l["x_guess"][rows])
    e_roll = TH.rollout_err(mm, DT, np.concatenate(ugs), np.concatenate(xgs))
    print("%s: roll-out of %d logged guesses %.2f ulp" % (case, sum(u.shape[0] for u in ugs), e_roll))
    assert e_roll <= 4.0, e_roll
    # cold re-solves on the handles of a fresh fleet: every fifth tick, and each robot's first tick in each phase
    fresh = _fleet(mm, F)
    engs = fresh._mission_handles(manip)
    pick = set(range(5, T, 5))
    for b in range(B):
        for p in G.SOLVED:
            if (ph[b, 1:] == p).any():
                pick.add(1 + int(np.argmax(ph[b, 1:] == p)))
    compared = missed = 0
    worst = 0.0
    for t in sorted(pick):
        l = log[t]
        if not solved[:, t].any():
            continue
        o = dict(X=_sentinel(B, N + 1, 9), U=_sentinel(B, N, 5), s=_sentinel(B, N + 1), cost=_sentinel(B), err=_sentinel(B),
                 status=torch.full((B,), -7, dtype=torch.int32, device="cuda:0"), iters=torch.full((B,), -7, dtype=torch.int32, device="cuda:0"))
        for p, e in zip(G.SOLVED, engs):
            rows = np.flatnonzero(ph[:, t] == p).astype(np.int32)
            if rows.size:
                e.solve_rows_device((_dev(rows), _dev(np.array([rows.size], np.int32))), _dev(l["x_in"]), _dev(l["loc"]), fresh.uref,
                                    _dev(l["u_last"]), _dev(l["obs"]), o)
        torch.cuda.synchronize()
        rows = solved[:, t]
        cold, cw = o["cost"].cpu().numpy()[rows], l["cost"][rows]
        assert (o["status"].cpu().numpy()[rows] == 0).all() and (warm["status"][rows, t] == 0).all(), t
        rel = np.abs(cw - cold) / np.maximum(1.0, np.abs(cold))
        compared += rel.size; missed += int((rel > 1e-6).sum()); worst = max(worst, float(rel.max()))
    print("%s: %d warm solves re-solved cold, %d miss |dcost| <= 1e-6 max(1, |cost|), worst %.2e" % (case, compared, missed, worst))
    assert compared >= 100 and missed <= 0.02 * compared, (missed, compared)
    # fewer iterations
    means = [float(r["iters"][:, 1:][np.isin(r["phase"][:, 1:], G.SOLVED)].mean()) for r in (ref, warm)]
    print("%s: mean iterations from tick 1 on, reference %.2f, shifted %.2f; slowest %d / %d" % (
        case, means[0], means[1], ref["iters"].max(), warm["iters"].max()))
    assert means[1] < means[0], means


def test_robots_do_not_interact_and_streams_do_not_matter(mm, missions):
    import torch
    F, c = missions["F"], missions["manipulate"]
    T, kw, r = c["T"], c["kw"], c["warm"]
    keys = KEYS + ("mcounts", "qgoal", "ik_status", "plan")
    s3 = _np(missions["fleet"].run_mission(T, streams=3, warm_start="shifted", **kw))
    torch.cuda.synchronize()
    for k in keys:
        assert np.array_equal(s3[k], r[k]), k
    d3 = _np(missions["fleet"].run_mission(CASES["drive"][0], streams=3, warm_start="shifted"))
    for k in KEYS:
        assert np.array_equal(d3[k], missions["drive"]["warm"][k]), k
    for b in (0, 7):
        one = _np(_fleet(mm, F, slice(b, b + 1)).run_mission(T, warm_start="shifted", manipulate=dict(pose=F["pose"][b:b + 1], t_manipulate=2)))
        for k in ("u0", "iters", "status", "phase", "x", "final_phase", "qgoal", "ik_status", "plan"):
            assert np.array_equal(one[k][0], r[k][b]), (b, k)


def test_handles_are_restored(mm, missions):
    import torch
    F, fleet, c = missions["F"], missions["fleet"], missions["manipulate"]
    T, kw = c["T"], c["kw"]
    keys = KEYS + ("mcounts", "qgoal", "ik_status", "plan")
    expect = _np(_fleet(mm, F).run_mission(T, **kw))
    for k in keys:                                   # (a fresh fleet's, and the run before the shifted ones of the fixture)
        assert np.array_equal(expect[k], c["ref"][k]), k
    # after the shifted runs of the fixture
    after = _np(fleet.run_mission(T, **kw))
    for k in keys:
        assert np.array_equal(after[k], expect[k]), k

    # after a shifted run whose on_tick raises
    class Stop(Exception):
        pass

    def on_tick(t, s):
        if t == 40:
            raise Stop()

    with pytest.raises(Stop):
        fleet.run_mission(T, on_tick=on_tick, warm_start="shifted", **kw)
    torch.cuda.synchronize()
    after = _np(fleet.run_mission(T, **kw))
    for k in keys:
        assert np.array_equal(after[k], expect[k]), k
    # the lock-step handle of the same fleet is handle 0 of the mission: back at the reference protocol as well
    a, b = _np(fleet.run_lockstep(3)), _np(_fleet(mm, F).run_lockstep(3))
    for k in ("u0", "iters", "x"):
        assert np.array_equal(a[k], b[k]), k


def test_warm_start_argument_errors(mm):
    F = MH.mission_fleet(mm, 2, N, DT)
    with pytest.raises(ValueError, match="shifted"):
        mm.DeviceFleet(mm, F["x0"], F["glob"], F["obs0"], F["vel"], N=N, fused=True, warm_start="shifted").run_mission(2)
    with pytest.raises(ValueError, match="shifted"):
        mm.DeviceFleet(mm, F["x0"], F["glob"], F["obs0"], F["vel"], N=N, fused=True, warm_start="shifted").run_mission(2, warm_start="shifted")
    fleet = mm.DeviceFleet(mm, F["x0"], F["glob"], F["obs0"], F["vel"], N=N)
    for bad in ("cold", None, True):
        with pytest.raises(ValueError, match="warm_start must be"):
            fleet.run_mission(2, warm_start=bad)
