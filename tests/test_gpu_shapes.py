"""GPU: shape libraries through the C ABI - handles created with specialise="cached" run the kernels of the libraries the entry
point's build() compiled (csrc/shapes/); nothing is compiled here.  References: the C oracle (1e-6, the project's standing
parity tolerance), IPOPT's termination test with independently fitted multipliers (tests/test_gpu_certificates.py's bound),
the host emulation of the same template (iteration counts), and the solve without a budget / of the whole batch / of the table
(bit for bit)."""
import copy
import sys

import numpy as np
import pytest

from oracle import nlp, coracle, synth
from cert_pool import certify
from test_slsqp_golden import cert_ok
import shape_helper as H
import tick_emu_helper as TH

pytestmark = pytest.mark.gpu
TOL = 1e-6


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(torch.device("cuda", 0))      # (a copy: the shared inputs are read-only)


def _np(r):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def _engine(mm, shape, par, B, mode=False, **kw):
    k, N, M = shape
    return mm._capi.Engine(k, N, M, par.dt, par.ulim, par.xlim, par.dulim, max_batch=B, obs_per_stage=mode, max_iter=2000, **kw)


def _solve(eng, d, obs=None, **kw):
    return _np(eng.solve_batch_device(_dev(d["x_init"]), _dev(d["traj_ref"]), _dev(d["u_ref"]), _dev(d["u_last"]),
                                      _dev(d["obs"] if obs is None else obs), **kw))


@pytest.mark.parametrize("shape", H.SHAPE_LIST, ids=H.shape_id)
def test_cached_library_runs_and_agrees(mm, shape):
    k, N, M = shape
    B = H.B_TEST
    par, d = H.inputs(shape)
    eng = _engine(mm, shape, par, B, specialise="cached")
    assert mm._capi.lib().mmpc_runs_specialised(eng._h) == 1 and eng.runs_specialised
    assert eng.lds_bytes == H.fast_lds_bytes(shape, 0)
    r, o, e = _solve(eng, d), H.oracle(shape), H.emulated(shape)
    dX, dU, ds = H.max_dev(r, o)
    print("%s: problems per CU %d, LDS %d B; vs oracle |dX| %.2e |dU| %.2e |ds| %.2e; iterations mean %.1f max %d, differing from the host emulation at %s"
          % (H.shape_id(shape), eng.problems_per_cu, eng.lds_bytes, dX, dU, ds, r["iters"].mean(), r["iters"].max(),
             np.flatnonzero(r["iters"] != e["iters"]).tolist()))
    assert (r["status"] == 0).all() and (o["status"] == 0).all()
    assert dX <= TOL and dU <= TOL and ds <= TOL
    assert np.array_equal(r["iters"], e["iters"])
    sel = np.concatenate([np.argsort(-r["iters"], kind="stable")[:4], np.arange(B)[-4:]])
    ul = np.zeros((N, par.nu))
    cs = certify([(nlp.Problem(par, d["x_init"][b], d["traj_ref"][b], d["u_ref"][b], ul, d["obs"][b]), r["X"][b], r["U"][b], r["s"][b]) for b in sel])
    assert all(cert_ok(c) for c in cs), max(c["E0"] for c in cs)


def test_defaults_stay_as_they_are(mm, monkeypatch):
    B = H.B_TEST
    # an unlisted shape without the keyword: the generic kernel, although its library is loaded in this process
    shape = (0, 12, 4)
    par, d = H.inputs(shape)
    assert _engine(mm, shape, par, B, specialise="cached").runs_specialised
    eng = _engine(mm, shape, par, B)
    assert mm._capi.lib().mmpc_runs_specialised(eng._h) == 0 and not eng.runs_specialised
    assert eng.lds_bytes == H.generic_lds_bytes(shape, 0)
    # a listed shape with specialise=True: nothing is built or loaded, and the solve is the solve without the keyword
    b = sys.modules[mm.__name__ + ".build"]
    calls = []
    monkeypatch.setattr(b, "build_shape_library", lambda *a, **k: calls.append(("build", a)))
    monkeypatch.setattr(b, "load_shape_library", lambda *a, **k: calls.append(("load", a)))
    N, M = 20, 5
    par = nlp.WholeBodyParams(N=N)
    g = synth.make_batch(B, N=N, M=M)
    x0 = nlp.clip_x_init(par, g["x_init"])
    outs = []
    for kw in (dict(), dict(specialise=True)):
        ctrl = mm.MPCWholeBody(mm.MobileManipulator(0.1), [], [], N=N, max_batch=B, n_obstacles=M, **kw)
        assert ctrl._engine.runs_specialised
        outs.append(ctrl.solve_batch(x0, g["traj_ref"], g["u_ref"], g["obs"]))
    assert not calls
    H.assert_bitwise(outs[0], outs[1], what="listed shape with specialise=True")
    assert (outs[0]["status"] == 0).all()


def test_budget_and_list_launches(mm):
    import torch
    shape = (0, 24, 6)
    k, N, M = shape
    B = H.B_TEST
    par, d = H.inputs(shape)
    eng = _engine(mm, shape, par, B, specialise="cached")
    full = _solve(eng, d)
    assert (full["status"] == 0).all() and full["iters"].max() > 10
    # list launch over a shuffled half of the rows
    rows = np.random.default_rng(3).permutation(B)[:B // 2].astype(np.int32)
    f = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device="cuda:0")
    i = lambda *s: torch.full(s, -7, dtype=torch.int32, device="cuda:0")
    out = dict(X=f(B, N + 1, 9), U=f(B, N, 5), s=f(B, N + 1), status=i(B), iters=i(B), cost=f(B), err=f(B))
    lst = _solve(eng, d, out=out, rows=(_dev(rows), _dev(np.array([len(rows)], np.int32))))
    rest = np.setdiff1d(np.arange(B), rows)
    for key in H.BIT_KEYS + ("err",):
        assert lst[key][rows].tobytes() == full[key][rows].tobytes(), key
        assert (lst[key][rest] == -7).all(), key
    # budgeted launch + continuation
    eng.set_iteration_budget(10)
    x, tr, ur, ul, ob = (_dev(d[a]) for a in ("x_init", "traj_ref", "u_ref", "u_last", "obs"))
    o = eng.solve_batch_device(x, tr, ur, ul, ob)
    nsusp = eng.suspended_count()
    assert 0 < nsusp and int((o["status"] == 3).sum()) == nsusp
    eng.resume_batch_device(x, tr, ur, ul, ob, o)
    H.assert_bitwise(_np(o), full, what="budget 10 + continuation")


def _terminal_case(shape, B):
    """inputs(shape) with the terminal reference position moved to 3 cm beside where the oracle's solve WITHOUT the equality ends -
    within reach of the short horizon, and the equality is active - and the oracle's solve of them with the equality.  The
    instances are those on which the oracle converges within 50 iterations (its terminal-equality solve gives up on about half of
    a batch at this shape and crawls on two more: a property of the reference, found out before anything runs on the GPU)."""
    par, d = H.inputs(shape, B)
    N = shape[1]
    d = {k: np.array(v) for k, v in d.items()}
    d["traj_ref"][:, N, :2] = H.oracle(shape, B)["X"][:, N, :2] + 0.03
    pt = copy.deepcopy(par); pt.terminal_xy_equality = True
    o = coracle.solve_batch(pt, d["x_init"], d["traj_ref"], d["u_ref"], d["u_last"], d["obs"], nthreads=16, max_iter=2000)
    rows = np.flatnonzero((o["status"] == 0) & (o["iters"] <= 50))
    print("terminal-equality case: %d of %d instances kept (oracle status %s, iterations %s)" % (len(rows), B, o["status"].tolist(), o["iters"].tolist()))
    assert len(rows) >= 8, o["status"]
    return par, {k: np.ascontiguousarray(v[rows]) for k, v in d.items()}, {k: v[rows] for k, v in o.items()}


def test_terminal_equality_falls_back_per_launch(mm):
    shape = (0, 12, 4)
    N = shape[1]
    par, d, o = _terminal_case(shape, H.B_TEST)
    B = d["x_init"].shape[0]
    eng = _engine(mm, shape, par, B, specialise="cached")
    L = mm._capi.lib()
    assert L.mmpc_runs_specialised(eng._h) == 1
    eng.set_terminal_xy_equality(True)
    assert L.mmpc_runs_specialised(eng._h) == 0 and eng.lds_bytes == H.generic_lds_bytes(shape, 0)
    r = _solve(eng, d)
    dX, dU, ds = H.max_dev(r, o)
    print("terminal equality on the generic kernel: |dX| %.2e |dU| %.2e |ds| %.2e" % (dX, dU, ds))
    assert (r["status"] == 0).all() and (o["status"] == 0).all()
    assert np.abs(r["X"][:, N, :2] - d["traj_ref"][:, N, :2]).max() < 1e-9
    assert dX <= TOL and dU <= TOL and ds <= TOL
    eng.set_terminal_xy_equality(False)
    assert L.mmpc_runs_specialised(eng._h) == 1 and eng.lds_bytes == H.fast_lds_bytes(shape, 0)
    # dense weights: the same per-launch fallback
    Q = np.diag([25.0, 25, 0, 0, 0, 5, 5, 5, 5]); Q[0, 1] = Q[1, 0] = 0.5
    eng.set_weights(Q=Q)
    assert L.mmpc_runs_specialised(eng._h) == 0
    eng.set_weights(Q=np.diag(np.diag(Q)))
    assert L.mmpc_runs_specialised(eng._h) == 1


def test_fleet_motion_equals_table(mm):
    import torch
    N, M, B, T = 24, 6, 32, 3
    g = synth.make_batch(B, N=N, M=M, config_id=5, moving=True)
    par = nlp.WholeBodyParams(N=N)
    res = {}
    for how in ("table", "motion"):
        fleet = mm.DeviceFleet(mm, np.clip(g["x_init"], par.xlim[0], par.xlim[1]), _dev(TH.straight_plan(g["traj_ref"], N)), g["obs"], g["obs_vel"],
                               N=N, fused=True, obstacles=how, specialise="cached")
        assert fleet.engs[0].runs_specialised and fleet.engs[0].lds_bytes == H.fast_lds_bytes((0, N, M), 2 if how == "motion" else 1)
        r = fleet.run_lockstep(T)
        torch.cuda.synchronize()
        assert bool(r["all_converged"]), how
        res[how] = {k: r[k].clone() for k in ("u0", "x", "iters")}
    for k in ("u0", "x", "iters"):
        assert torch.equal(res["table"][k], res["motion"][k]), k
