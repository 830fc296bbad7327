"""GPU (MI355X): the linear-motion obstacle mode (obs_per_stage = 2: record (B, M, 5) + per-instance clock) through the C ABI
against its table twin - the same solve with the per-stage table c + v ((tick + k) dt) built in numpy.  Both runs see identical
centres and run the same iteration: every motion-against-table comparison is bitwise on X, U, s, status, iters, cost."""
import numpy as np
import pytest

from oracle import nlp, coracle

import motion_helper as mh
import tick_emu_helper as H
import test_motion_cpu as T

pytestmark = pytest.mark.gpu
MODES = {0: False, 1: True, 2: "motion"}
FAST = T.FAST
WB = [s for s in FAST if s[0] == 0]


@pytest.fixture(autouse=True)
def _motion_abi(mm):
    """a library without the mode (it would take "motion" for a table handle) is found out from the missing symbol, before
    anything is launched"""
    assert hasattr(mm._capi.lib(), "mmpc_set_obstacle_clock"), "libmmpc.so has no mmpc_set_obstacle_clock: no motion mode"
    assert hasattr(mm._capi.Engine, "set_obstacle_clock")


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _engine(mm, kind, par, M, mode, B):
    return mm._capi.Engine(kind, par.N, M, par.dt, par.ulim, par.xlim, par.dulim, max_batch=B, obs_per_stage=MODES[mode], max_iter=2000)


def _np(r):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def _solve(eng, d, obs, **kw):
    par_nu = d["u_ref"].shape[2]
    ul = np.zeros((d["x_init"].shape[0], d["u_ref"].shape[1], par_nu))
    return _np(eng.solve_batch_device(_dev(d["x_init"]), _dev(d["traj_ref"]), _dev(d["u_ref"]), _dev(ul), _dev(obs), **kw))


def _case(k, N, M, B):
    par = nlp.WholeBodyParams(N=N) if k == 0 else nlp.BaseParams(N=N)
    d = mh.motion_inputs(B, N, M, kind="wholebody" if k == 0 else "base")
    if k == 0:
        d["x_init"] = np.clip(d["x_init"], par.xlim[0], par.xlim[1])
    d["tab"] = mh.table_twin(d["rec"], d["tick"], N, par.dt)
    return par, d


def _pair(mm, k, par, M, B, d, weights=None):
    """a table handle and a motion handle with the case's clock registered; their outputs of one device-pointer launch"""
    et, em = _engine(mm, k, par, M, 1, B), _engine(mm, k, par, M, 2, B)
    if weights is not None:
        et.set_weights(**weights); em.set_weights(**weights)
    em.set_obstacle_clock(_dev(d["tick"]))
    return et, em, _solve(et, d, d["tab"]), _solve(em, d, d["rec"])


@pytest.mark.parametrize("k,N,M", FAST)
def test_specialised_motion_equals_table_and_oracle(mm, k, N, M):
    B = 64
    par, d = _case(k, N, M, B)
    et, em, t, m = _pair(mm, k, par, M, B, d)
    assert em.lds_bytes == 8 * mh.fast_lds_doubles(k, N, M, 2) and et.lds_bytes == 8 * mh.fast_lds_doubles(k, N, M, 1)   # the specialised kernels
    mh.assert_bitwise(m, t, what="motion vs table")
    assert (m["status"] == 0).all(), m["status"]
    o = coracle.solve_batch(par, d["x_init"], d["traj_ref"], d["u_ref"], np.zeros((B, N, par.nu)), d["tab"], nthreads=16, max_iter=2000)
    assert (o["status"] == 0).all()
    e = np.abs(m["X"] - o["X"]).reshape(B, -1).max(axis=1)
    print("max |X - oracle| per instance: max %.3e, instances above 1e-6: %s" % (e.max(), np.nonzero(e > 1e-6)[0]))
    assert e.max() <= 1e-6, e.max()


@pytest.mark.parametrize("kind,N,M", T.GENERIC)
def test_generic_motion_equals_table(mm, kind, N, M):
    B = 8
    par = T._par(kind, N)
    d = T._inputs(kind, B, N, M)
    d["tab"] = mh.table_twin(d["rec"], d["tick"], N, par.dt)
    k = {"wb": 0, "base": 1, "pose": 2}[kind]
    et, em, t, m = _pair(mm, k, par, M, B, d)
    assert em.lds_bytes == 8 * mh.lds_doubles(k, N, M, 2)
    assert (t["status"] == 0).all()
    mh.assert_bitwise(m, t, what="motion vs table")


def test_specialised_shape_on_the_generic_kernel(mm):
    """(0,20,5) with one non-zero off-diagonal weight: the handle runs the generic kernel"""
    B, N, M = 16, 20, 5
    par, d = _case(0, N, M, B)
    Q = np.diag([25.0, 25, 0, 0, 0, 5, 5, 5, 5]); Q[0, 1] = Q[1, 0] = 0.5
    et, em, t, m = _pair(mm, 0, par, M, B, d, weights=dict(Q=Q))
    assert em.lds_bytes == 8 * mh.lds_doubles(0, N, M, 2)
    assert (t["status"] == 0).all()
    mh.assert_bitwise(m, t, what="motion vs table")


def test_launch_forms(mm):
    import torch
    k, N, M, B = 0, 30, 8, 64
    par, d = _case(k, N, M, B)
    em = _engine(mm, k, par, M, 2, B)
    em.set_obstacle_clock(_dev(d["tick"]))
    full = _solve(em, d, d["rec"])
    assert (full["status"] == 0).all() and full["iters"].max() > 12
    # list launch over a shuffled half of the rows
    rows = np.random.default_rng(3).permutation(B)[:B // 2].astype(np.int32)
    f = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device="cuda:0")
    i = lambda *s: torch.full(s, -7, dtype=torch.int32, device="cuda:0")
    out = dict(X=f(B, N + 1, 9), U=f(B, N, 5), s=f(B, N + 1), status=i(B), iters=i(B), cost=f(B), err=f(B))
    lst = _solve(em, d, d["rec"], out=out, rows=(_dev(rows), _dev(np.array([len(rows)], np.int32))))
    rest = np.setdiff1d(np.arange(B), rows)
    for key in mh.OUT_KEYS:
        assert np.array_equal(lst[key][rows], full[key][rows]), key
        assert (lst[key][rest] == -7).all(), key
    # budgeted launch + continuation
    em.set_iteration_budget(12)
    x, tr, ur, ul, rec = (_dev(a) for a in (d["x_init"], d["traj_ref"], d["u_ref"], np.zeros((B, N, 5)), d["rec"]))
    o = em.solve_batch_device(x, tr, ur, ul, rec)
    nsusp = em.suspended_count()
    assert 0 < nsusp and int((o["status"] == 3).sum()) == nsusp
    em.resume_batch_device(x, tr, ur, ul, rec, o)
    mh.assert_bitwise(_np(o), full, what="budget 12 + continuation")
    em.set_iteration_budget(0)
    # the host-pointer call (the handle's warm start is zero after a reset: U_last = 0, as the device call above)
    em.reset()
    hp = em.solve_batch(d["x_init"], d["traj_ref"], d["u_ref"], d["rec"])
    mh.assert_bitwise(hp, full, what="host-pointer call")
    assert np.array_equal(hp["u0"], full["U"][:, 0])


def test_clock_registration(mm):
    k, N, M, B = 0, 20, 3, 16
    par, d = _case(k, N, M, B)
    em = _engine(mm, k, par, M, 2, B)
    unset = _solve(em, d, d["rec"])
    em.set_obstacle_clock(_dev(d["tick"]))
    ticked = _solve(em, d, d["rec"])
    em.set_obstacle_clock(_dev(np.zeros(B, np.int64)))
    zeros = _solve(em, d, d["rec"])
    em.set_obstacle_clock(None)
    cleared = _solve(em, d, d["rec"])
    mh.assert_bitwise(cleared, zeros, what="NULL clock vs zeros")
    mh.assert_bitwise(unset, zeros, what="default clock vs zeros")
    assert not np.array_equal(ticked["X"], zeros["X"])
    et = _engine(mm, k, par, M, 1, B)
    with pytest.raises(RuntimeError, match=r"mmpc_set_obstacle_clock failed \(-4\)"):
        et.set_obstacle_clock(_dev(d["tick"]))
    with pytest.raises(RuntimeError, match=r"\(-4\)"):
        _engine(mm, k, par, M, 0, B).set_obstacle_clock(None)
    assert em.obs_shape(B) == (B, M, 5) and et.obs_shape(B) == (B, N + 1, M, 3)


def test_problems_per_cu(mm):
    for k, N, M in WB:
        par = nlp.WholeBodyParams(N=N)
        m, t = _engine(mm, k, par, M, 2, 4).problems_per_cu, _engine(mm, k, par, M, 1, 4).problems_per_cu
        print("(0,%d,%d): problems per CU motion %d, table %d" % (N, M, m, t))
        assert m == 4 and m >= t, (N, M, m, t)


def test_create_and_tick_prepare_errors(mm):
    import torch
    N, M, B = 30, 8, 32
    par = nlp.WholeBodyParams(N=N)
    with pytest.raises(RuntimeError, match=r"mmpc_create failed \(-1\)"):
        mm._capi.Engine(0, N, M, par.dt, par.ulim, par.xlim, par.dulim, max_batch=B, obs_per_stage=3)
    d = H.fleet_inputs(B=B)
    em, et = _engine(mm, 0, par, M, 2, B), _engine(mm, 0, par, M, 1, B)

    def run(eng, **kw):
        x, tick = _dev(d["x"]), _dev(d["tick"])
        f = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device="cuda:0")
        out = dict(x_in=f(B, 9), traj_ref=f(B, N + 1, 9), start=torch.full((B,), -7, dtype=torch.int32, device="cuda:0"), u_guess=f(B, N, 5), x_guess=f(B, N + 1, 9))
        eng.tick_prepare(x, tick, U_prev=_dev(d["U_prev"]), glob=_dev(d["glob"]), **out, **kw)
        r = _np(out)
        r["x"], r["tick"] = x.cpu().numpy(), tick.cpu().numpy()
        return r

    tab = torch.zeros((B, N + 1, M, 3), dtype=torch.float64, device="cuda:0")
    with pytest.raises(RuntimeError, match=r"mmpc_tick_prepare_device failed \(-1\).*d_obs"):
        run(em, obs0=_dev(d["obs0"]), vel=_dev(d["vel"]), obs=tab)
    a, b = run(em), run(et, obs0=_dev(d["obs0"]), vel=_dev(d["vel"]), obs=tab)
    assert (a["tick"] == d["tick"] + 1).all()
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), key


# ---- the fleet
FN, FM = 30, 8


def _fleet(mm, B, **kw):
    from oracle import synth
    d = synth.make_batch(B, N=FN, M=FM, config_id=5, moving=True)
    par = nlp.WholeBodyParams(N=FN)
    return mm.DeviceFleet(mm, np.clip(d["x_init"], par.xlim[0], par.xlim[1]), _dev(H.straight_plan(d["traj_ref"], FN)), d["obs"], d["obs_vel"], N=FN, **kw)


def _run(fleet, T, how="run_lockstep", **kw):
    import torch
    r = getattr(fleet, how)(T, **kw)
    torch.cuda.synchronize()
    assert bool(r["all_converged"])
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in r.items()}


def _same(a, b, what):
    import torch
    for k in ("u0", "x", "iters"):
        assert torch.equal(a[k], b[k]), (what, k)


def _tensors(v):
    import torch
    if torch.is_tensor(v):
        yield v
    elif isinstance(v, dict):
        for x in v.values():
            yield from _tensors(x)
    elif isinstance(v, (list, tuple)):
        for x in v:
            yield from _tensors(x)


def _no_table(fleet, B):
    """no (B, N+1, M, 3) buffer among the fleet's tensors, buffer sets and sub-fleets"""
    for name, v in vars(fleet).items():
        for t in _tensors(v):
            assert tuple(t.shape) != (B, FN + 1, FM, 3), name
    for lo, hi, sub, _ in getattr(fleet, "_groups", []):
        _no_table(sub, hi - lo)


@pytest.mark.parametrize("fused,warm_start", [(True, "reference"), (True, "shifted"), (False, "reference")])
def test_fleet_lock_step_motion_equals_table(mm, fused, warm_start):
    B, Tn = 1024, 6
    t = _run(_fleet(mm, B, fused=fused, warm_start=warm_start), Tn)
    fm = _fleet(mm, B, fused=fused, warm_start=warm_start, obstacles="motion")
    m = _run(fm, Tn)
    _same(m, t, "lock step")
    _same(_run(fm, Tn), t, "second run on the same fleet")
    _no_table(fm, B)
    assert fm.engs[0].obs_shape(B) == (B, FM, 5)


def test_fleet_groups_and_async_in_motion_mode(mm):
    with pytest.raises(ValueError, match="obstacles must be"):
        _fleet(mm, 8, obstacles="moving")
    B, Tn = 1024, 6
    fm = _fleet(mm, B, fused=True, obstacles="motion")
    a = _run(fm, Tn)
    g = _run(fm, Tn, "run_groups", groups=3)
    _same(g, a, "groups")
    assert all(sub.motion for _, _, sub, _ in fm._groups)
    _no_table(fm, B)
    B, Tn = 256, 4
    fa = _fleet(mm, B, obstacles="motion")
    lock = _run(fa, Tn)
    asy = _run(fa, Tn, "run_async", budget=24)
    _same(asy, lock, "async")
    assert int(asy["suspended"]) >= 1, int(asy["suspended"])
    _no_table(fa, B)
    _same(lock, _run(_fleet(mm, B), Tn), "unfused lock step against the table fleet")
