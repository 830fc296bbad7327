"""GPU (MI355X): mmpc_set_iteration_budget / mmpc_resume_batch_device through the C ABI, cut at EVERY iteration, on the pools of
tests/continuation_pool.py - rows on which (tests/test_continuation_cpu.py asserts it on the host build) the cuts fall where the
rarely non-zero state of a suspended solve is live: the proximal term, the count of small steps, the inertia corrections of the
last two iterations, a full filter, a filter just emptied.  The device adds what no host build has: row state parked from
registers, the continuation grid of 256 workgroups that stride over the list of the suspended, mmpc_collect_suspended.

Everything is exact equality of GPU against GPU (the reference is the same handle's uninterrupted solve); that reference has to
agree with the host build in status and iteration counts and within the parity tolerance, so that iteration b of the device IS
the cut the coverage test speaks of."""
import numpy as np
import pytest

import continuation_pool as CP

pytestmark = pytest.mark.gpu
TOL = 1e-6
KEYS = CP.OUT_KEYS      # all seven outputs


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(torch.device("cuda", 0))      # (a copy: the shared inputs are read-only)


def _np(r):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


class _Run:
    """a handle of the case's shape and obstacle mode with the case's inputs (or the rows `rowmap` of them) on the device"""

    def __init__(self, mm, c, rowmap=None, max_iter=CP.MAX_ITER):
        import torch
        (k, N, M), par, d = c["shape"], c["par"], c["d"]
        rowmap = np.arange(d["x_init"].shape[0]) if rowmap is None else np.asarray(rowmap)
        self.B, self.N, self.nx, self.nu = len(rowmap), N, par.nx, par.nu
        kw = dict(specialise="cached") if c["library"] else {}
        self.eng = mm._capi.Engine(k, N, M, par.dt, par.ulim, par.xlim, par.dulim, max_batch=self.B,
                                   obs_per_stage={0: False, 1: True, 2: "motion"}[c["mode"]], max_iter=max_iter, **kw)
        assert self.eng.runs_specialised      # (a library shape: the cached library of the entry point's build, as test_gpu_shapes.py)
        self.t = [_dev(d[a][rowmap]) for a in ("x_init", "traj_ref", "u_ref", "u_last", "obs")]
        if c["mode"] == 2:
            self.eng.set_obstacle_clock(_dev(np.ascontiguousarray(c["tick"][rowmap], np.int64)))
        self.torch = torch

    def fresh(self):
        """an output set filled with a sentinel: nothing of an earlier launch can pass for this one's"""
        f = lambda *s: self.torch.full(s, -7.0, dtype=self.torch.float64, device="cuda:0")
        i = lambda *s: self.torch.full(s, -7, dtype=self.torch.int32, device="cuda:0")
        B, N = self.B, self.N
        return dict(X=f(B, N + 1, self.nx), U=f(B, N, self.nu), s=f(B, N + 1), status=i(B), iters=i(B), cost=f(B), err=f(B))

    def solve(self, out=None, **kw):
        return self.eng.solve_batch_device(*self.t, out=self.fresh() if out is None else out, **kw)

    def resume(self, out):
        return self.eng.resume_batch_device(*self.t, out)


def _sweep(run, ref, what):
    """every budget b = 1 ... max(iters) + 1: launch, look, continue, compare"""
    eng, it = run.eng, ref["iters"]
    top = int(it.max()) + 1
    try:
        for b in range(1, top + 1):
            eng.set_iteration_budget(b)
            out = run.solve()
            first = _np(out)
            susp = it > b
            assert eng.suspended_count() == int(susp.sum()), (what, b)
            assert (first["status"][susp] == 3).all() and (first["iters"][susp] == b).all(), (what, b)
            CP.assert_bitwise(first, ref, keys=KEYS, what="%s, budget %d, rows that end within it" % (what, b), rows=~susp)
            run.resume(out)
            CP.assert_bitwise(_np(out), ref, keys=KEYS, what="%s, budget %d + continuation" % (what, b))
        assert not susp.any()      # the last budget is past the end: nothing was suspended, the continuation was a no-op
    finally:
        eng.set_iteration_budget(0)
    return top


_gpu = {}


def _reference(mm, name):
    """the case's handle and its uninterrupted solve (once per case), held to the host build"""
    if name not in _gpu:
        c = CP.case(name)
        run = _Run(mm, c)
        ref = _np(run.solve())
        _gpu[name] = (c, run, ref)
    return _gpu[name]


@pytest.mark.parametrize("name", CP.CASES)
def test_reference_agrees_with_the_host_build(mm, name):
    c, run, ref = _reference(mm, name)
    e = CP.uninterrupted(name)
    dev = tuple(float(np.abs(ref[k] - e[k]).max()) for k in ("X", "U", "s"))
    print("%s: B %d, iterations gpu %s host %s; gpu - host |dX| %.2e |dU| %.2e |ds| %.2e" % ((name, run.B, ref["iters"].tolist(), e["iters"].tolist()) + dev))
    assert np.array_equal(ref["status"], e["status"]) and (ref["status"] == 0).all()
    assert np.array_equal(ref["iters"], e["iters"])
    assert max(dev) <= TOL, dev


@pytest.mark.parametrize("name", CP.CASES)
def test_every_cut_is_the_uninterrupted_solve(mm, name):
    c, run, ref = _reference(mm, name)
    n = _sweep(run, ref, name)
    print("%s: %d budgets x %d rows, %d cuts" % (name, n, run.B, int(sum((ref["iters"] > b).sum() for b in range(1, n + 1)))))


def _cap_budgets(it):
    """the first cut, the last one, and one in the middle"""
    return sorted({1, int(it.max()) // 2, int(it.max()) - 1} - {0})


@pytest.mark.parametrize("name", CP.CASES)
def test_a_cut_and_the_iteration_cap_together(mm, name):
    """max_iter = b and budget b: the cap comes first - nobody is suspended, the unconverged rows report status 1, and the outputs
    are those of the same handle without a budget"""
    c, _, ref = _reference(mm, name)
    for b in _cap_budgets(ref["iters"]):
        run = _Run(mm, c, max_iter=b)
        capped = _np(run.solve())
        over = ref["iters"] > b
        assert over.any() and (capped["status"][over] == 1).all() and (capped["iters"][over] == b).all(), (name, b)
        CP.assert_bitwise(capped, ref, keys=KEYS, what="%s, max_iter %d, rows that end within it" % (name, b), rows=~over)
        run.eng.set_iteration_budget(b)
        both = _np(run.solve())
        assert run.eng.suspended_count() == 0 and not (both["status"] == 3).any(), (name, b)
        CP.assert_bitwise(both, capped, keys=KEYS, what="%s, max_iter %d = budget" % (name, b))
        run.eng.close()


def test_every_cut_with_objective_scaling_on(mm):
    """the factor of the objective travels in the save area (scalar 10): the sweep against the uninterrupted SCALED solve"""
    import torch
    c = CP.case("0-20-5")
    run = _Run(mm, c)
    scale = torch.full((run.B,), -1.0, dtype=torch.float64, device="cuda:0")
    run.eng.set_objective_scaling(CP.G_SCALING, scale)
    ref = _np(run.solve())
    sc = scale.cpu().numpy()
    off = _reference(mm, "0-20-5")[2]
    assert (ref["status"] == 0).all() and (sc < 1).any() and (sc == 1).any(), sc
    assert any(ref["X"][b].tobytes() != off["X"][b].tobytes() for b in np.flatnonzero(sc < 1))      # another solve than the unscaled one
    _sweep(run, ref, "0-20-5 scaled")


@pytest.mark.parametrize("name", ["0-30-8", "0-20-5"])
def test_the_striding_grid_keeps_instances_apart(mm, name):
    """600 instances (the pool tiled under a seeded permutation) and a budget of 2: every one is suspended, and the 256
    workgroups of the continuation run two or three instances each, one after the other - in the same LDS block, with the gain
    block and the correction scratch of each instance's own row.  Every row has to be bitwise its row of the small batch."""
    c, _, ref = _reference(mm, name)
    n, B, budget = len(ref["iters"]), 600, 2
    rowmap = np.resize(np.arange(n), B)[np.random.default_rng(600 + n).permutation(B)]
    run = _Run(mm, c, rowmap=rowmap)
    big = {k: v[rowmap] for k, v in ref.items()}
    full = _np(run.solve())
    CP.assert_bitwise(full, big, keys=KEYS, what="%s x 600, one launch" % name)
    run.eng.set_iteration_budget(budget)
    out = run.solve()
    nsusp = run.eng.suspended_count()
    assert nsusp == int((big["iters"] > budget).sum()) and nsusp >= 2 * 256      # the premise: every continuation workgroup strides
    run.resume(out)
    CP.assert_bitwise(_np(out), big, keys=KEYS, what="%s x 600, budget %d + continuation" % (name, budget))


@pytest.mark.parametrize("name", CP.CASES)
def test_a_list_launch_with_a_budget(mm, name):
    """mmpc_solve_list_device with a budget (mmpc_collect_suspended_list): half of the rows, shuffled, and one index outside the
    batch.  Only listed rows are suspended, their count is exact; after the continuation the listed rows are the reference's and
    the others still hold the sentinel."""
    c, run, ref = _reference(mm, name)
    B = run.B
    rows = np.random.default_rng(B).permutation(B)[:(B + 1) // 2].astype(np.int32)
    lst = np.insert(rows, len(rows) // 2, B + 3).astype(np.int32)
    rest = np.setdiff1d(np.arange(B), rows)
    budget = int(np.sort(ref["iters"][rows])[len(rows) // 2 - 1])      # some listed rows end within it, at least one does not
    susp = np.zeros(B, bool); susp[rows] = ref["iters"][rows] > budget
    assert susp.any() and not susp[rows].all()
    try:
        run.eng.set_iteration_budget(budget)
        out = run.solve(rows=(_dev(lst), _dev(np.array([len(lst)], np.int32))))
        first = _np(out)
        assert run.eng.suspended_count() == int(susp.sum())
        assert np.array_equal(first["status"] == 3, susp) and (first["iters"][susp] == budget).all()
        run.resume(out)
        r = _np(out)
        CP.assert_bitwise(r, ref, keys=KEYS, what="%s, list launch, budget %d + continuation" % (name, budget), rows=rows)
        for k in KEYS:
            assert (first[k][rest] == -7).all() and (r[k][rest] == -7).all(), k
    finally:
        run.eng.set_iteration_budget(0)
