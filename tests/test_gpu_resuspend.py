"""GPU (MI355X): re-suspendable continuations through the C ABI - mmpc_set_resume_budget, chains of budgeted continuations on both
kernel families, the carry of suspended rows across budgeted list launches, and mmpc_mission_rejoin_device against its host build.

A continuation that parks again is what no host build has: registers rebuilt from a save area are parked from a workgroup that then
strides on to the next instance in the same LDS block.  Everything is exact equality of GPU against GPU: the reference of a case is
the same handle's uninterrupted solve (tests/test_gpu_continuation.py and tests/test_gpu_generic_continuation.py hold that one to
the host builds), and a solve is the same bits wherever and however often it is cut."""
import ctypes as C

import numpy as np
import pytest

import continuation_pool as CP
import generic_cont_helper as GH
import round_emu_helper as R
import suspend_emu_helper as SH
import test_gpu_continuation as TC
import test_gpu_generic_continuation as TG

pytestmark = pytest.mark.gpu
KEYS = CP.OUT_KEYS
SPECIALISED = ["0-20-5", "0-30-8", "1-15-3", "0-20-5-motion", "lib-0-23-2"]
GENERIC = ["wb-12-2", "wb-20-3-teq-table", "base-10-2", "pose-10-2"]
UNSUPPORTED = r"failed \(-4\)"
_dev, _np = TC._dev, TC._np


class _GRun(TG._Run):
    """test_gpu_generic_continuation._Run with the iteration cap as a keyword"""

    def __init__(self, mm, c, rowmap=None, max_iter=GH.MAX_ITER):
        import torch
        par, d = c["par"], c["d"]
        rowmap = np.arange(c["B"]) if rowmap is None else np.asarray(rowmap)
        self.c, self.B, self.N, self.nx, self.nu = c, len(rowmap), c["N"], par.nx, par.nu
        kw = dict(generic_budget=True)
        if c["hs"] is not None:
            kw.update(halfspaces=c["hs"], as_written=c["as_written"])
        self.eng = mm._capi.Engine(c["kind_id"], c["N"], c["M"], par.dt, par.ulim, par.xlim, par.dulim, max_batch=self.B,
                                   obs_per_stage={0: False, 1: True, 2: "motion"}[c["mode"]], max_iter=max_iter, **kw)
        if getattr(par, "terminal_xy_equality", False):
            self.eng.set_terminal_xy_equality(True)
        assert not self.eng.runs_specialised
        self.t = [_dev(d[a][rowmap]) for a in ("x_init", "traj_ref", "u_ref", "u_last", "obs")]
        self.xg = None if c["x_guess"] is None else _dev(c["x_guess"][rowmap])
        if c["mode"] == 2:
            self.eng.set_obstacle_clock(_dev(np.ascontiguousarray(c["tick"][rowmap], np.int64)))
        self.torch = torch


def _make(mm, name, **kw):
    return TC._Run(mm, CP.case(name), **kw) if name in CP.CASES else _GRun(mm, GH.case(name), **kw)


_gpu = {}


def _reference(mm, name):
    """the case's handle and its uninterrupted solve (once per case)"""
    if name not in _gpu:
        run = _make(mm, name)
        ref = _np(run.solve())
        assert (ref["status"] == 0).all(), ref["status"]
        _gpu[name] = (run, ref)
    return _gpu[name]


def _pairs(it):
    return [(1, 1), (2, 3), (max(int(it.max()) // 2, 1), 7)]


def _chain(run, ref, b, c, what, first=None, cap=None):
    """a budgeted launch (or first(): the caller's launches, which return the output set), then continuations until nobody is
    suspended; after continuation n exactly the rows with I > b + n c are suspended, at b + n c iterations, and every other row is
    the reference's.  Returns the outputs and the number of continuations."""
    eng, it = run.eng, ref["iters"]
    out = run.solve() if first is None else first()
    n = 0
    while True:
        done = b + n * c
        r = _np(out)
        susp = it > done
        assert np.array_equal(r["status"] == 3, susp) and (r["iters"][susp] == done).all(), (what, b, c, n)
        assert eng.suspended_count() == int(susp.sum()), (what, b, c, n)
        CP.assert_bitwise(r, ref, keys=KEYS, what="%s, budget %d + %d x %d, rows that have ended" % (what, b, n, c), rows=~susp)
        if not susp.any():
            break
        run.resume(out)
        n += 1
        assert n <= int(it.max())
    # one more call: OK, and nothing changes
    run.resume(out)
    assert eng.suspended_count() == 0
    CP.assert_bitwise(_np(out), ref, keys=KEYS, what="%s, budget %d, resume budget %d, a continuation of nobody" % (what, b, c))
    return r, n


@pytest.mark.parametrize("name", SPECIALISED + GENERIC)
def test_chain_of_budgeted_continuations(mm, name):
    run, ref = _reference(mm, name)
    eng, top = run.eng, int(ref["iters"].max())
    try:
        for b, c in _pairs(ref["iters"]):
            eng.set_iteration_budget(b)
            eng.set_resume_budget(c)
            _, n = _chain(run, ref, b, c, name)
            assert n == -(-(top - b) // c), (name, b, c, n)
    finally:
        eng.set_resume_budget(0)
        eng.set_iteration_budget(0)


def test_chain_with_objective_scaling_on(mm):
    """the factor of the objective travels in the save area, through every park"""
    import torch
    run = _make(mm, "0-20-5")
    scale = torch.full((run.B,), -1.0, dtype=torch.float64, device="cuda:0")
    run.eng.set_objective_scaling(CP.G_SCALING, scale)
    ref = _np(run.solve())
    sc = scale.cpu().numpy()
    assert (ref["status"] == 0).all() and (sc < 1).any(), sc
    off = _reference(mm, "0-20-5")[1]
    assert any(ref["X"][b].tobytes() != off["X"][b].tobytes() for b in np.flatnonzero(sc < 1))
    run.eng.set_iteration_budget(2)
    run.eng.set_resume_budget(3)
    _chain(run, ref, 2, 3, "0-20-5 scaled")
    assert np.array_equal(scale.cpu().numpy(), sc)
    run.eng.close()


@pytest.mark.parametrize("name", ["0-20-5", "0-30-8"])
def test_the_striding_grid_parks_again(mm, name):
    """600 instances, budget 2, resume budget 3: at least 2 x 256 are suspended, so every workgroup of the continuation grid parks
    an instance whose registers came from a save area and strides on to the next one in the same LDS block"""
    _, ref = _reference(mm, name)
    n, B, b, c = len(ref["iters"]), 600, 2, 3
    rowmap = np.resize(np.arange(n), B)[np.random.default_rng(600 + n).permutation(B)]
    run = _make(mm, name, rowmap=rowmap)
    big = {k: v[rowmap] for k, v in ref.items()}
    run.eng.set_iteration_budget(b)
    run.eng.set_resume_budget(c)
    out = run.solve()
    nsusp = run.eng.suspended_count()
    assert nsusp == int((big["iters"] > b).sum()) and nsusp >= 2 * 256
    assert int((big["iters"] > b + c).sum()) >= 2 * 256          # ... and as many park again in the first continuation
    k = 0
    while nsusp:
        run.resume(out)
        k += 1
        nsusp = run.eng.suspended_count()
        assert nsusp == int((big["iters"] > b + k * c).sum()), k
    assert k == -(-(int(big["iters"].max()) - b) // c)
    CP.assert_bitwise(_np(out), big, keys=KEYS, what="%s x 600, budget %d, resume budget %d" % (name, b, c))
    run.eng.close()


@pytest.mark.parametrize("name", ["0-20-5", "1-15-3", "wb-12-2"])
def test_the_iteration_cap_inside_a_continuation(mm, name):
    """max_iter = b + c: the rows that need more end the first continuation with status 1 at b + c iterations, nobody is suspended,
    and the outputs are those of the same handle with that cap and no budget"""
    _, ref = _reference(mm, name)
    cap = int(np.sort(ref["iters"])[(len(ref["iters"]) - 1) // 2])      # the median: some rows end inside the continuation, some need more
    b = cap // 2
    c = cap - b
    over = ref["iters"] > b + c
    assert over.any() and (ref["iters"] > b).sum() > over.sum()
    run = _make(mm, name, max_iter=b + c)
    capped = _np(run.solve())
    assert (capped["status"][over] == 1).all() and (capped["iters"][over] == b + c).all()
    CP.assert_bitwise(capped, ref, keys=KEYS, what="%s, max_iter %d, rows that end within it" % (name, b + c), rows=~over)
    run.eng.set_iteration_budget(b)
    run.eng.set_resume_budget(c)
    out = run.solve()
    assert run.eng.suspended_count() == int((ref["iters"] > b).sum())
    run.resume(out)
    assert run.eng.suspended_count() == 0
    CP.assert_bitwise(_np(out), capped, keys=KEYS, what="%s, max_iter %d = budget + resume budget" % (name, b + c))
    run.eng.close()


def _halves(B, seed):
    rows = np.random.default_rng(seed).permutation(B).astype(np.int32)
    return rows[:B // 2], rows[B // 2:]


def _rows(lst):
    lst = np.asarray(lst, np.int32)
    return _dev(lst), _dev(np.array([len(lst)], np.int32))


@pytest.mark.parametrize("name", ["0-20-5", "wb-20-3-teq-table"])
@pytest.mark.parametrize("again", [False, True], ids=["disjoint", "a-carried-row-named-again"])
def test_list_launches_carry_the_suspended(mm, name, again):
    """list A (half the rows, shuffled, one index outside the batch) under a budget, then list B (the other half - and, in the
    variant, one row still suspended from A, which starts afresh): the handle's suspended set is the union's, every row once, and
    the chain ends with every row the reference's"""
    run, ref = _reference(mm, name)
    eng, B, it = run.eng, run.B, ref["iters"]
    A, Bl = _halves(B, 31 + B)
    b = int(np.sort(it)[B // 3])                 # a third of the rows end within it
    sa = A[it[A] > b]
    assert len(sa) >= 1 and (it[Bl] > b).any() and (it <= b).any()
    listA = np.insert(A, len(A) // 2, B + 3)
    listB = np.concatenate([Bl, sa[:1]]) if again else Bl
    c = 2
    try:
        eng.set_iteration_budget(b)
        eng.set_resume_budget(c)

        def first():
            out = run.solve(rows=_rows(listA), either_family=name in GENERIC)
            assert eng.suspended_count() == len(sa)
            run.solve(out=out, rows=_rows(listB), either_family=name in GENERIC)
            return out
        _chain(run, ref, b, c, "%s, lists A and B" % name, first=first)
    finally:
        eng.set_resume_budget(0)
        eng.set_iteration_budget(0)


@pytest.mark.parametrize("name", ["0-20-5", "wb-20-3-teq-table"])
def test_without_a_resume_budget_a_list_launch_replaces_the_suspended(mm, name):
    """today's behaviour, pinned: with c = 0 the same two launches leave only B's suspended rows resumable"""
    run, ref = _reference(mm, name)
    eng, B, it = run.eng, run.B, ref["iters"]
    A, Bl = _halves(B, 31 + B)
    b = int(np.sort(it)[B // 3])
    sa, sb = A[it[A] > b], Bl[it[Bl] > b]
    assert len(sa) and len(sb)
    try:
        eng.set_iteration_budget(b)
        out = run.solve(rows=_rows(A), either_family=name in GENERIC)
        assert eng.suspended_count() == len(sa)
        run.solve(out=out, rows=_rows(Bl), either_family=name in GENERIC)
        assert eng.suspended_count() == len(sb)
        run.resume(out)
        r = _np(out)
        CP.assert_bitwise(r, ref, keys=KEYS, what="%s, list B + continuation" % name, rows=Bl)
        assert (r["status"][sa] == 3).all() and (r["iters"][sa] == b).all()          # A's are left behind
        with pytest.raises(RuntimeError, match=UNSUPPORTED):                          # ... and a second continuation is refused
            run.resume(out)
    finally:
        eng.set_iteration_budget(0)


def test_errors(mm):
    run, ref = _reference(mm, "0-20-5")
    eng = run.eng
    L = mm._capi.lib()
    assert L.mmpc_set_resume_budget(eng._h, -1) == -1 and L.mmpc_set_resume_budget(None, 1) == -1
    with pytest.raises(RuntimeError, match=r"failed \(-1\)"):
        eng.set_resume_budget(-1)
    # a handle without budgets: the generic kernel of a default handle
    c = GH.case("base-10-2")
    par = c["par"]
    plain = mm._capi.Engine(c["kind_id"], c["N"], c["M"], par.dt, par.ulim, par.xlim, par.dulim, max_batch=8)
    with pytest.raises(RuntimeError, match=UNSUPPORTED + r".*mmpc_set_resume_budget.*generic kernel"):
        plain.set_resume_budget(1)
    plain.set_resume_budget(0)
    plain.close()
    b = max(int(ref["iters"].max()) // 2, 1)
    try:
        eng.set_iteration_budget(b)
        # c = 0: the second continuation is refused, as ever
        out = run.solve()
        run.resume(out)
        with pytest.raises(RuntimeError, match=UNSUPPORTED):
            run.resume(out)
        # c > 0: mmpc_reset between launch and continuation leaves the areas stale; so does a change of the iteration budget
        eng.set_resume_budget(1)
        out = run.solve()
        run.resume(out)
        assert eng.suspended_count() > 0
        eng.reset()
        with pytest.raises(RuntimeError, match=UNSUPPORTED):
            run.resume(out)
        out = run.solve()
        eng.set_iteration_budget(b + 1)
        with pytest.raises(RuntimeError, match=UNSUPPORTED):
            run.resume(out)
        # ... while a change of the resume budget does not: the chain goes on with the new one, to the same bits
        eng.set_iteration_budget(b)
        out = run.solve()
        run.resume(out)
        eng.set_resume_budget(5)
        while eng.suspended_count():
            run.resume(out)
        CP.assert_bitwise(_np(out), ref, keys=KEYS, what="resume budget changed inside a chain")
        # back to 0 inside a chain: the next continuation runs to the end
        out = run.solve()
        eng.set_resume_budget(1)
        run.resume(out)
        assert eng.suspended_count() > 0
        eng.set_resume_budget(0)
        run.resume(out)
        CP.assert_bitwise(_np(out), ref, keys=KEYS, what="resume budget back to 0 inside a chain")
    finally:
        eng.set_resume_budget(0)
        eng.set_iteration_budget(0)


def test_the_host_pointer_call_returns_finished_solves(mm):
    """the continuation inside mmpc_solve_batch runs to the end whatever the resume budget is"""
    c = CP.case("0-20-5")
    (k, N, M), par, d = c["shape"], c["par"], c["d"]
    eng = mm._capi.Engine(k, N, M, par.dt, par.ulim, par.xlim, par.dulim, max_batch=d["x_init"].shape[0])
    plain = eng.solve_batch(d["x_init"], d["traj_ref"], d["u_ref"], d["obs"])
    eng.reset()
    eng.set_iteration_budget(3)
    eng.set_resume_budget(1)
    cut = eng.solve_batch(d["x_init"], d["traj_ref"], d["u_ref"], d["obs"])
    assert (cut["status"] == 0).all() and cut["iters"].max() > 4
    for key in ("X", "U", "status", "iters"):
        assert np.array_equal(plain[key], cut[key]), key
    eng.close()


# ---- the rejoin kernel -------------------------------------------------------------------------------------------------------------
N_R, T_R, B_R = 20, 7, 512


def _rejoin_gpu(eng, s, set_):
    import torch
    t = {k: _dev(v) for k, v in s.items()}
    counters = torch.full((4,), -7, dtype=torch.int32, device="cuda:0")
    out = dict(U=t["U"], status=t["status"], iters=t["iters"])
    eng.mission_rejoin(t["hold"], t["solve_phase"], set_, out, t["tick"], t["phase"], t["U_last"], t["u0"], t["iters_hist"], t["status_hist"],
                       t["phase_hist"], counters)
    torch.cuda.synchronize()
    r = {k: t[k].cpu().numpy() for k in R.COMMIT_STATE}
    r["counters"] = counters.cpu().numpy()
    return r


@pytest.mark.parametrize("set_", [1, 3])
def test_rejoin_kernel_is_its_host_build(mm, set_):
    ctrl = mm.MPCWholeBody(mm.MobileManipulator(0.1), [], [], N=N_R, max_batch=B_R, n_obstacles=3, obs_per_stage=True)
    s = SH.rejoin_inputs(B_R, N_R, T_R)
    host = SH.rejoin(N_R, s, set_)
    stay = (s["hold"] == R.SUSPENDED + set_) & (s["status"] == 3)
    assert stay.sum() > 0 and host["counters"][1] == stay.sum()
    r = _rejoin_gpu(ctrl._engine, s, set_)
    for k in R.COMMIT_STATE + ("counters",):
        assert np.array_equal(r[k], host[k]), k


def test_rejoin_argument_checks(mm):
    import torch
    B, T = 256, 5
    ctrl = mm.MPCWholeBody(mm.MobileManipulator(0.1), [], [], N=N_R, max_batch=B, n_obstacles=3, obs_per_stage=True)
    eng = ctrl._engine
    L = mm._capi.lib()
    i32 = dict(dtype=torch.int32, device="cuda:0")
    f = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda:0")
    hold, sp = torch.full((B,), R.RETIRED, **i32), torch.full((B,), -1, **i32)
    arrays = dict(hold=hold, solve_phase=sp, U=f(B, N_R, 5), status=torch.zeros(B, **i32), iters=torch.zeros(B, **i32),
                  tick=torch.zeros(B, dtype=torch.int64, device="cuda:0"), phase=torch.zeros(B, **i32), U_last=f(B, N_R, 5), u0=f(B, T, 5),
                  ih=torch.zeros((B, T), **i32), sh=torch.zeros((B, T), **i32), ph=torch.zeros((B, T), **i32), cnt=torch.zeros(4, **i32))
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def rejoin(B_=B, h=eng._h, set_=0, T_=T, **a):
        g = lambda k: p(a.get(k, arrays[k]))
        return L.mmpc_mission_rejoin_device(h, B_, g("hold"), g("solve_phase"), set_, g("U"), g("status"), g("iters"), g("tick"), g("phase"),
                                            g("U_last"), g("u0"), g("ih"), g("sh"), g("ph"), T_, g("cnt"), None)

    assert rejoin() == 0 and rejoin(set_=15) == 0 and rejoin(B_=0) == 0
    for k in arrays:
        assert rejoin(**{k: None}) == -1, k
    assert rejoin(U_last=arrays["U"]) == -1 and rejoin(set_=16) == -1 and rejoin(set_=-1) == -1 and rejoin(T_=0) == -1
    assert rejoin(B_=257) == -1 and rejoin(h=None) == -1
    base = mm.MPCBase(mm.Base(0.1), [], N=15, max_batch=256)
    assert L.mmpc_mission_rejoin_device(base._engine._h, B, *([p(hold)] * 2), 0, *([p(hold)] * 10), T, p(arrays["cnt"]), None) == -4
    torch.cuda.synchronize()
    assert (hold == R.RETIRED).all() and not arrays["u0"].any() and arrays["cnt"].tolist() == [0, 0, 0, 0]
