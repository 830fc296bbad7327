"""GPU (MI355X): iteration budgets and continuation on the GENERIC kernel, through the C ABI on handles created with
cfg.generic_budget (the `generic_budget` keyword of Engine, the controllers and DeviceFleet).

Three cases of tests/generic_cont_helper.py - the terminal-xy equality on a motion record, two half-space planes as written, the base
kind at (10, 2); tests/test_generic_continuation_cpu.py asserts on the host build where their cuts fall - with every budget plus one
continuation against the same handle's uninterrupted solve, exact equality of GPU against GPU.  Then what only the device has: the
budgeted list launches on a generic handle, the continuation grid that strides over more suspended instances than it has workgroups,
the stale-area refusals, the refusals a default handle keeps, the host-pointer call, and DeviceFleet.run_async at an unlisted (N, M)
without a shape library."""
import numpy as np
import pytest

import generic_cont_helper as H
import tick_emu_helper as TH
from oracle import nlp, synth

pytestmark = pytest.mark.gpu
KEYS = H.OUT_KEYS
GPU_CASES = ["wb-20-3-teq-motion", "wb-20-3-planes-aw", "base-10-2"]
UNSUPPORTED = r"failed \(-4\)"      # MMPC_E_UNSUPPORTED through Engine._chk


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(torch.device("cuda", 0))      # (a copy: the shared inputs are read-only)


def _np(r):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


class _Run:
    """a handle of the case's configuration - created with generic_budget unless told otherwise - with the case's inputs (or the rows
    `rowmap` of them) on the device"""

    def __init__(self, mm, c, rowmap=None, generic_budget=True, max_batch=None):
        import torch
        par, d = c["par"], c["d"]
        rowmap = np.arange(c["B"]) if rowmap is None else np.asarray(rowmap)
        self.c, self.B, self.N, self.nx, self.nu = c, len(rowmap), c["N"], par.nx, par.nu
        kw = dict(generic_budget=True) if generic_budget else {}
        if c["hs"] is not None:
            kw.update(halfspaces=c["hs"], as_written=c["as_written"])
        self.eng = mm._capi.Engine(c["kind_id"], c["N"], c["M"], par.dt, par.ulim, par.xlim, par.dulim, max_batch=max_batch or self.B,
                                   obs_per_stage={0: False, 1: True, 2: "motion"}[c["mode"]], max_iter=H.MAX_ITER, **kw)
        if getattr(par, "terminal_xy_equality", False):
            self.eng.set_terminal_xy_equality(True)
        assert not self.eng.runs_specialised
        self.t = [_dev(d[a][rowmap]) for a in ("x_init", "traj_ref", "u_ref", "u_last", "obs")]
        self.xg = None if c["x_guess"] is None else _dev(c["x_guess"][rowmap])
        if c["mode"] == 2:
            self.eng.set_obstacle_clock(_dev(np.ascontiguousarray(c["tick"][rowmap], np.int64)))
        self.torch = torch

    def fresh(self, B=None):
        """an output set filled with a sentinel: nothing of an earlier launch can pass for this one's"""
        f = lambda *s: self.torch.full(s, -7.0, dtype=self.torch.float64, device="cuda:0")
        i = lambda *s: self.torch.full(s, -7, dtype=self.torch.int32, device="cuda:0")
        B, N = B or self.B, self.N
        return dict(X=f(B, N + 1, self.nx), U=f(B, N, self.nu), s=f(B, N + 1), status=i(B), iters=i(B), cost=f(B), err=f(B))

    def solve(self, out=None, **kw):
        return self.eng.solve_batch_device(*self.t, x_guess=self.xg, out=self.fresh() if out is None else out, **kw)

    def resume(self, out):
        return self.eng.resume_batch_device(*self.t, out, x_guess=self.xg)


_gpu = {}


def _reference(mm, name):
    """the case's opted-in handle and its uninterrupted solve (once per case)"""
    if name not in _gpu:
        c = H.case(name)
        run = _Run(mm, c)
        ref = _np(run.solve())
        e = H.uninterrupted(name)
        print("%s: B %d, iterations gpu %s host %s; gpu - host |dX| %.2e" % (name, run.B, ref["iters"].tolist(), e["iters"].tolist(),
                                                                             np.abs(ref["X"] - e["X"]).max()))
        assert (ref["status"] == 0).all(), ref["status"]
        _gpu[name] = (c, run, ref)
    return _gpu[name]


@pytest.mark.parametrize("name", GPU_CASES)
def test_every_budget_plus_one_continuation(mm, name):
    """every budget b = 1 ... max(iters) + 1: launch, count, continue, compare with the handle's uninterrupted solve"""
    c, run, ref = _reference(mm, name)
    assert run.B == 8
    eng, it = run.eng, ref["iters"]
    top = int(it.max()) + 1
    try:
        for b in range(1, top + 1):
            eng.set_iteration_budget(b)
            out = run.solve()
            first = _np(out)
            susp = it > b
            assert eng.suspended_count() == int(susp.sum()) == int((first["status"] == 3).sum()), (name, b)
            assert (first["status"][susp] == 3).all() and (first["iters"][susp] == b).all(), (name, b)
            H.assert_bitwise(first, ref, keys=KEYS, what="%s, budget %d, rows that end within it" % (name, b), rows=~susp)
            run.resume(out)
            H.assert_bitwise(_np(out), ref, keys=KEYS, what="%s, budget %d + continuation" % (name, b))
        assert not susp.any()      # the last budget is past the end: nothing was suspended, the continuation was a no-op
    finally:
        eng.set_iteration_budget(0)
    # without a budget the opted-in handle is a default one.  Where the default handle runs the run-time-sized kernel too, the very
    # numbers; where it runs a static-LDS instantiation (MMPC_STATIC_LIST: the planes case) the same solve by another instantiation -
    # status and iteration counts equal, the point within the suite's parity tolerance
    plain = _Run(mm, c, generic_budget=False)
    p = _np(plain.solve())
    if c["hs"] is None:
        H.assert_bitwise(p, ref, keys=KEYS, what="%s, default handle against the opted-in one" % name)
    else:
        assert np.array_equal(p["status"], ref["status"]) and np.array_equal(p["iters"], ref["iters"])
        assert max(np.abs(p[k] - ref[k]).max() for k in ("X", "U", "s")) <= 1e-6
    plain.eng.close()


@pytest.mark.parametrize("name", ["base-10-2", "wb-20-3-teq-motion"])
@pytest.mark.parametrize("entry", ["rows", "list"])
def test_a_budgeted_list_launch_on_a_generic_handle(mm, name, entry):
    """mmpc_solve_rows_device and mmpc_solve_list_device with a budget on a generic handle: half of the rows, shuffled, with one index
    past the batch and a negative one.  Only listed rows are written and suspended, their count is exact; the continuation finishes
    exactly the suspended listed rows, the unlisted ones still hold the sentinel."""
    c, run, ref = _reference(mm, name)
    B = run.B
    rows = np.random.default_rng(B).permutation(B)[:(B + 1) // 2].astype(np.int32)
    lst = np.insert(np.insert(rows, len(rows) // 2, B + 3), 1, -2).astype(np.int32)
    rest = np.setdiff1d(np.arange(B), rows)
    budget = int(np.sort(ref["iters"][rows])[len(rows) // 2 - 1])      # some listed rows end within it, at least one does not
    susp = np.zeros(B, bool); susp[rows] = ref["iters"][rows] > budget
    assert susp.any() and not susp[rows].all()
    try:
        run.eng.set_iteration_budget(budget)
        out = run.solve(rows=(_dev(lst), _dev(np.array([len(lst)], np.int32))), either_family=entry == "rows")
        first = _np(out)
        assert run.eng.suspended_count() == int(susp.sum())
        assert np.array_equal(first["status"] == 3, susp) and (first["iters"][susp] == budget).all()
        run.resume(out)
        r = _np(out)
        H.assert_bitwise(r, ref, keys=KEYS, what="%s, %s launch, budget %d + continuation" % (name, entry, budget), rows=rows)
        for k in KEYS:
            assert (first[k][rest] == -7).all() and (r[k][rest] == -7).all(), k
    finally:
        run.eng.set_iteration_budget(0)


def test_the_striding_grid_keeps_instances_apart(mm):
    """600 instances (the base case tiled under a seeded permutation) and a budget of 2: every one is suspended, and the 256
    workgroups of the continuation run two or three instances each, one after the other in the same LDS block"""
    c, _, ref = _reference(mm, "base-10-2")
    n, B, budget = len(ref["iters"]), 600, 2
    rowmap = np.resize(np.arange(n), B)[np.random.default_rng(600 + n).permutation(B)]
    run = _Run(mm, c, rowmap=rowmap)
    big = {k: v[rowmap] for k, v in ref.items()}
    H.assert_bitwise(_np(run.solve()), big, keys=KEYS, what="base x 600, one launch")
    run.eng.set_iteration_budget(budget)
    out = run.solve()
    nsusp = run.eng.suspended_count()
    assert nsusp == int((big["iters"] > budget).sum()) and nsusp >= 2 * 256      # the premise: every continuation workgroup strides
    run.resume(out)
    H.assert_bitwise(_np(out), big, keys=KEYS, what="base x 600, budget %d + continuation" % budget)
    run.eng.close()


def test_stale_save_areas_are_refused(mm):
    """a continuation belongs to the budgeted launch directly before it: another B, a second continuation, a change of the budget,
    and new weights in between (the continuation re-derives them) all leave MMPC_E_UNSUPPORTED - and the outputs untouched"""
    c, _, ref = _reference(mm, "base-10-2")
    run = _Run(mm, c)
    eng = run.eng
    budget = int(np.sort(ref["iters"])[0]) - 1
    assert budget >= 1
    eng.set_iteration_budget(budget)
    # another B
    out = run.solve()
    with pytest.raises(RuntimeError, match=UNSUPPORTED):
        eng.resume_batch_device(*[t[:4].contiguous() for t in run.t], {k: v[:4].contiguous() for k, v in out.items()})
    # (the refused call cleared nothing it should not: the launch is repeated for the next refusal)
    out = run.solve()
    assert eng.suspended_count() == run.B
    run.resume(out)
    H.assert_bitwise(_np(out), ref, keys=KEYS, what="continuation")
    with pytest.raises(RuntimeError, match=UNSUPPORTED):      # a second continuation
        run.resume(out)
    out = run.solve()
    eng.set_iteration_budget(budget + 1)                      # a change of the budget
    with pytest.raises(RuntimeError, match=UNSUPPORTED):
        run.resume(out)
    out = run.solve()
    before = _np(out)
    eng.set_weights(Q=np.diag([5.0, 5, 0, 0, 0, 2]))          # setWeight in between
    with pytest.raises(RuntimeError, match=UNSUPPORTED):
        run.resume(out)
    H.assert_bitwise(_np(out), before, keys=KEYS, what="outputs after a refused continuation")
    eng.close()
    # the equality switched between a budgeted launch and its continuation: stale as well
    ct, _, reft = _reference(mm, "wb-20-3-teq-motion")
    runt = _Run(mm, ct)
    runt.eng.set_iteration_budget(2)
    out = runt.solve()
    runt.eng.set_terminal_xy_equality(False)
    with pytest.raises(RuntimeError, match=UNSUPPORTED):
        runt.resume(out)
    runt.eng.close()


def test_a_default_handle_still_refuses_the_budget(mm):
    """without cfg.generic_budget nothing changes: the budget is refused on a generic-only handle, and so are list launches through
    mmpc_solve_list_device"""
    c = H.case("base-10-2")
    run = _Run(mm, c, generic_budget=False)
    with pytest.raises(RuntimeError, match=UNSUPPORTED):
        run.eng.set_iteration_budget(4)
    lst = _dev(np.arange(run.B, dtype=np.int32))
    with pytest.raises(RuntimeError, match=UNSUPPORTED):
        run.solve(rows=(lst, _dev(np.array([run.B], np.int32))))
    run.eng.close()
    # a listed shape keeps its specialised budget, and its rows launch keeps refusing one
    d = synth.make_batch(4, N=15, M=3, kind="base", config_id=2)
    par = nlp.BaseParams(N=15)
    eng = mm._capi.Engine(1, 15, 3, par.dt, par.ulim, par.xlim, par.dulim, max_batch=4)
    assert eng.runs_specialised
    eng.set_iteration_budget(3)
    t = [_dev(d["x_init"]), _dev(d["traj_ref"]), _dev(d["u_ref"]), _dev(np.zeros((4, 15, 2))), _dev(d["obs"])]
    import torch
    out = dict(X=torch.zeros((4, 16, 6), dtype=torch.float64, device="cuda:0"), U=torch.zeros((4, 15, 2), dtype=torch.float64, device="cuda:0"),
               s=torch.zeros((4, 16), dtype=torch.float64, device="cuda:0"), status=torch.zeros(4, dtype=torch.int32, device="cuda:0"),
               iters=torch.zeros(4, dtype=torch.int32, device="cuda:0"), cost=torch.zeros(4, dtype=torch.float64, device="cuda:0"),
               err=torch.zeros(4, dtype=torch.float64, device="cuda:0"))
    with pytest.raises(RuntimeError, match=UNSUPPORTED):
        eng.solve_rows_device((_dev(np.arange(4, dtype=np.int32)), _dev(np.array([4], np.int32))), *t, out)
    eng.close()


def test_the_host_pointer_call_returns_finished_solves(mm):
    """mmpc_solve_batch with a budget on an opted-in generic handle continues the suspended rows at once: the unbudgeted results"""
    c = H.case("wb-20-3-planes-aw")
    d = c["d"]
    res = []
    for budget in (0, 3):
        run = _Run(mm, c)
        run.eng.set_iteration_budget(budget)
        res.append(run.eng.solve_batch(d["x_init"], d["traj_ref"], d["u_ref"], d["obs"]))
        if budget:
            assert run.eng.suspended_count() == int((res[0]["iters"] > budget).sum()) > 0
        run.eng.close()
    assert (res[0]["status"] == 0).all()
    H.assert_bitwise(res[1], res[0], keys=("u0", "X", "U", "s", "status", "iters", "cost"), what="mmpc_solve_batch with a budget")


def test_run_async_at_an_unlisted_shape_without_a_shape_library(mm):
    """DeviceFleet(generic_budget=True).run_async at (N, M) = (12, 2): no specialised kernel, no library - the budgets are the
    generic kernel's.  Per-robot u0, x and iters are bitwise those of run_lockstep; some robots were suspended on the way."""
    import torch
    N, M, B, T = 12, 2, 32, 4
    g = synth.make_batch(B, N=N, M=M, config_id=5, moving=True)
    par = nlp.WholeBodyParams(N=N)
    fleet = mm.DeviceFleet(mm, np.clip(g["x_init"], par.xlim[0], par.xlim[1]), _dev(TH.straight_plan(g["traj_ref"], N)), g["obs"], g["obs_vel"],
                           N=N, generic_budget=True)
    assert not fleet.engs[0].runs_specialised and fleet.engs[0].generic_budget
    a = fleet.run_lockstep(T)
    b = fleet.run_async(T, budget=6)
    torch.cuda.synchronize()
    assert all(e.generic_budget and not e.runs_specialised for e in fleet.engs) and len(fleet.engs) == 3
    assert bool(a["all_converged"]) and bool(b["all_converged"])
    assert int(b["suspended"]) > 0, "the seed and the budget are chosen so that some robot is suspended"
    for k in ("u0", "x", "iters"):
        assert torch.equal(a[k], b[k]), k
    print("run_async (12, 2): %d rounds, %d suspensions, iterations %d .. %d" % (b["rounds"], int(b["suspended"]), int(a["iters"].min()), int(a["iters"].max())))
    # the same fleet without the keyword has no budgets at this shape
    plain = mm.DeviceFleet(mm, np.clip(g["x_init"], par.xlim[0], par.xlim[1]), _dev(TH.straight_plan(g["traj_ref"], N)), g["obs"], g["obs_vel"], N=N)
    with pytest.raises(RuntimeError, match=UNSUPPORTED):
        plain.run_async(T, budget=6)
