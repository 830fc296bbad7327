"""GPU (MI355X): what an instance of the persistent plain launch (mmpc_set_persistent_grid) starts on - the LDS block, the gain
block, the correction scratch and the registers its predecessor on the same workgroup left - on the rows of
tests/continuation_pool.py: solves that leave rare state behind (a proximal term, a count of small steps, inertia corrections, a
full filter, a second-order correction), in every obstacle mode (static record, table, motion record + tick word), on the four
listed shapes and two shape libraries (gains in global memory, the fully unrolled roll-out).
tests/test_gpu_persistent_launch.py covers the launch form itself on easy rows of three listed shapes in mode 0; this file is
about the predecessor.  tests/test_stale_state_cpu.py asks the same of the host builds, where the slab is the test's to fill.

Everything goes through the C ABI, into output sets pre-filled with the sentinel -7, and is compared bit for bit - all seven
outputs - with the same handle's launch at persistent_grid -1 (one workgroup per instance: no predecessor).  That reference has to
agree with the host build of the case in status and iteration counts and within the parity tolerance, so that the predecessors on
the device ARE the rare-state solves tests/test_continuation_cpu.py speaks of.

A row that differs names a pair: the row and its predecessor in launch order - at grid 1 the row before it."""
import numpy as np
import pytest

import continuation_pool as CP
import scaling_helper as SH

pytestmark = pytest.mark.gpu
TOL = 1e-6               # GPU against host build: the tolerance of tests/test_gpu_continuation.py
KEYS = CP.OUT_KEYS       # all seven outputs
NAN_CASES = ["0-20-5-table", "1-15-3-motion", "lib-0-23-2"]
WARM_CASES = ["0-20-5", "0-30-8", "1-15-3-motion", "lib-0-23-2"]
SCALED_CASES = ["0-30-8", "1-15-3-motion", "lib-0-23-2"]
BIG_CASES = ["0-20-5-table", "0-20-5-motion"]
BIG_B, BIG_GRID = 600, 64


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(torch.device("cuda", 0))      # (a copy: the shared inputs are read-only)


class _Run:
    """a handle of the case's shape and obstacle mode; solve() takes the rows of the case it is to run, in launch order"""

    def __init__(self, mm, c, max_batch=None, max_iter=CP.MAX_ITER):
        import torch
        self.torch, self.c = torch, c
        (k, N, M), par = c["shape"], c["par"]
        self.n = c["d"]["x_init"].shape[0]
        self.max_batch, self.N, self.nx, self.nu = int(max_batch or self.n), N, par.nx, par.nu
        kw = dict(specialise="cached") if c["library"] else {}
        self.eng = mm._capi.Engine(k, N, M, par.dt, par.ulim, par.xlim, par.dulim, max_batch=self.max_batch,
                                   obs_per_stage={0: False, 1: True, 2: "motion"}[c["mode"]], max_iter=max_iter, **kw)
        assert self.eng.runs_specialised      # (a library shape: the cached library of the entry point's build, as test_gpu_shapes.py)

    def inputs(self, rowmap=None, x_init=None):
        """the device tensors of the rows `rowmap` (default: the pool in its order); on a motion handle the obstacle clock as well"""
        c, d = self.c, self.c["d"]
        rowmap = np.arange(self.n) if rowmap is None else np.asarray(rowmap)
        t = [_dev((d[a] if a != "x_init" or x_init is None else x_init)[rowmap]) for a in ("x_init", "traj_ref", "u_ref", "u_last", "obs")]
        if c["mode"] == 2:
            tick = np.zeros(self.max_batch, np.int64)
            tick[:len(rowmap)] = c["tick"][rowmap]
            self.eng.set_obstacle_clock(_dev(tick))
        return t

    def fresh(self, B):
        """an output set filled with a sentinel: a row that no workgroup wrote cannot pass"""
        f = lambda *s: self.torch.full(s, -7.0, dtype=self.torch.float64, device="cuda:0")
        i = lambda *s: self.torch.full(s, -7, dtype=self.torch.int32, device="cuda:0")
        N = self.N
        return dict(X=f(B, N + 1, self.nx), U=f(B, N, self.nu), s=f(B, N + 1), status=i(B), iters=i(B), cost=f(B), err=f(B))

    def launch(self, t, grid, stream=None, **kw):
        """one launch with `grid`, not waited for"""
        out = self.fresh(t[0].shape[0])
        self.eng.set_persistent_grid(grid)
        self.eng.solve_batch_device(*t, out=out, stream=stream, **kw)
        return out

    def solve(self, grid, rowmap=None, t=None, **kw):
        out = self.launch(self.inputs(rowmap) if t is None else t, grid, **kw)
        self.torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}


def _assert_bitwise(new, old, what, rows=None, keys=KEYS):
    for k in keys:
        a, b = new[k], old[k]
        if rows is not None:
            a, b = a[rows], b[rows]
        a = np.ascontiguousarray(a).reshape(len(a), -1)
        b = np.ascontiguousarray(b).reshape(len(b), -1)
        same = (a.view(np.uint8) == b.view(np.uint8)).all(axis=1)
        assert same.all(), "%s: %s differs in rows %s (positions in launch order)" % (what, k, np.nonzero(~same)[0].tolist())


_gpu = {}


def _reference(mm, name):
    """the case's handle and its launch with one workgroup per instance (once per case), held to the host build"""
    if name not in _gpu:
        c = CP.case(name)
        run = _Run(mm, c)
        ref = run.solve(-1)
        e = CP.uninterrupted(name)
        dev = tuple(float(np.abs(ref[k] - e[k]).max()) for k in ("X", "U", "s"))
        print("%s: B %d, iterations gpu %s host %s; gpu - host |dX| %.2e |dU| %.2e |ds| %.2e" % ((name, run.n, ref["iters"].tolist(), e["iters"].tolist()) + dev))
        assert np.array_equal(ref["status"], e["status"]) and (ref["status"] == 0).all(), name
        assert np.array_equal(ref["iters"], e["iters"]), name
        assert max(dev) <= TOL, (name, dev)
        _gpu[name] = (c, run, ref)
    return _gpu[name]


@pytest.mark.parametrize("name", CP.CASES)
def test_every_case_behind_its_pool_predecessors(mm, name):
    """grid 1: one workgroup solves the whole pool in its order; 2 and 3: which rows share a workgroup is the ticket's business"""
    c, run, ref = _reference(mm, name)
    for grid in (1, 2, 3):
        _assert_bitwise(run.solve(grid), ref, "%s, grid %d" % (name, grid))


@pytest.mark.parametrize("name", CP.CASES)
def test_every_row_behind_several_predecessors(mm, name):
    """grid 1 with the rows reversed and under two seeded permutations (same handle, permuted input tensors)"""
    c, run, ref = _reference(mm, name)
    n = run.n
    maps = [("reversed", np.arange(n)[::-1])] + [("permutation %d" % s, np.random.default_rng(1000 * s + n).permutation(n)) for s in (1, 2)]
    before = {b: set() for b in range(n)}
    for what, rowmap in maps:
        for i in range(1, n):
            before[int(rowmap[i])].add(int(rowmap[i - 1]))
        new = run.solve(1, rowmap)
        _assert_bitwise(new, {k: v[rowmap] for k, v in ref.items()}, "%s, grid 1, %s %s" % (name, what, rowmap.tolist()))
    assert sum(len(v) >= 2 for v in before.values()) >= n - 2      # (all but a row or two - those that come first - have run behind two others)


@pytest.mark.parametrize("name", CP.CASES)
def test_predecessors_stopped_at_the_iteration_cap(mm, name):
    """max_iter at the median iteration count of the pool: the rows above it leave mid-solve, with their state live"""
    c, _, ref = _reference(mm, name)
    cap = int(np.median(ref["iters"]))
    run = _Run(mm, c, max_iter=cap)
    try:
        old = run.solve(-1)
        assert (old["status"] == 1).any() and (old["status"] == 0).any(), (name, cap, old["status"].tolist())
        assert set(old["status"].tolist()) <= {0, 1} and (old["iters"][old["status"] == 1] == cap).all()
        _assert_bitwise(old, ref, "%s, max_iter %d, rows that end within it" % (name, cap), rows=old["status"] == 0)
        for grid in (1, 2):
            _assert_bitwise(run.solve(grid), old, "%s, max_iter %d, grid %d" % (name, cap, grid))
    finally:
        run.eng.close()


@pytest.mark.parametrize("name", NAN_CASES)
def test_a_nan_instance_in_the_middle(mm, name):
    """the worst predecessor in the table mode, the motion mode and a library kernel: its successors are the rows of the clean batch"""
    c, run, ref = _reference(mm, name)
    mid = run.n // 2
    others = np.array([b for b in range(run.n) if b != mid])
    x_init = np.array(c["d"]["x_init"])
    x_init[mid, 0] = np.nan
    t = run.inputs(x_init=x_init)
    for grid in (-1, 2, 1):      # (grid 1: every later row runs behind the NaN one on the same workgroup)
        new = run.solve(grid, t=t)
        assert new["status"][mid] == 2, (name, grid, new["status"].tolist())
        _assert_bitwise(new, ref, "%s, grid %d, rows behind and beside the NaN instance (row %d)" % (name, grid, mid), rows=others)


def _shifted(U):
    return np.ascontiguousarray(np.concatenate([U[:, 1:], U[:, -1:]], axis=1))


@pytest.mark.parametrize("name", WARM_CASES)
def test_warm_start(mm, name):
    """mmpc_set_warm_start: U guess = the optimum shifted one stage, X guess = the optimum, mu_init = 0.1 - another start point, another
    barrier schedule, and (asserted on the host build) other iteration counts than the cold solve"""
    c, run, ref = _reference(mm, name)
    e = CP.uninterrupted(name)
    host = CP.warm(name, _shifted(e["U"]), e["X"], 0.1)
    assert (host["iters"] != e["iters"]).any(), (name, host["iters"].tolist())
    t = run.inputs()
    xg = _dev(ref["X"])
    try:
        run.eng.set_warm_start(_dev(_shifted(ref["U"])), mu_init=0.1)
        old = run.solve(-1, t=t, x_guess=xg)
        print("%s: iterations cold %s warm %s (host build, its own optimum as the guess: %s)" % (name, ref["iters"].tolist(), old["iters"].tolist(), host["iters"].tolist()))
        assert set(old["status"].tolist()) <= {0, 1} and (old["iters"] > 0).all()
        assert (old["iters"] != ref["iters"]).any()
        for grid in (1, 2):
            _assert_bitwise(run.solve(grid, t=t, x_guess=xg), old, "%s, warm start, grid %d" % (name, grid))
    finally:
        run.eng.set_warm_start(None, mu_init=1.0)
    _assert_bitwise(run.solve(2), ref, "%s, grid 2 after the warm start is off again" % name)


def scaling_bound(name):
    """nlp_scaling_max_gradient of a case: half way between the two smallest objective gradients of the pool (numpy), so that one row
    keeps the factor 1 and the others scale - held to the host build (tests/emu_scaling, generic kernel; the objective and so the
    factor do not see the obstacles: the static part of the case's obstacle input stands in for every mode)"""
    c = CP.case(name)
    d = dict(c["d"])
    d["obs"] = np.ascontiguousarray(d["obs"][:, 0] if c["mode"] == 1 else d["obs"][..., :3])
    g = np.sort(SH.sigma_numpy(c["par"], d)[1])
    G = 0.5 * (g[0] + g[1])
    assert g[0] < G < g[1]
    host = SH.solve(c["par"], d, G, fast=False, max_iter=1)["scale"]
    assert (host < 1).sum() >= 2 and (host == 1).sum() >= 1, (name, host.tolist())
    return G, host


@pytest.mark.parametrize("name", SCALED_CASES)
def test_objective_scaling_on(mm, name):
    """an instance that scales its weights rewrites the constants block in LDS; its successor may or may not scale"""
    import torch
    c, run, ref = _reference(mm, name)
    G, host = scaling_bound(name)
    scale = torch.full((run.max_batch,), -7.0, dtype=torch.float64, device="cuda:0")
    t = run.inputs()

    def solve(grid):
        scale.fill_(-7.0)
        r = run.solve(grid, t=t)
        r["scale"] = scale.cpu().numpy()
        return r
    try:
        run.eng.set_objective_scaling(G, scale)
        old = solve(-1)
        sc = old["scale"]
        print("%s: max gradient %.6g, factors %s" % (name, G, sc.tolist()))
        assert (sc < 1).sum() >= 2 and (sc == 1).sum() >= 1, sc
        # (device and host build each hold the factor to numpy's within 1e-13: tests/test_gpu_scaling.py, tests/test_scaling_cpu.py)
        assert np.array_equal(sc == 1, host == 1) and np.abs(sc / host - 1).max() <= 2e-13
        assert set(old["status"].tolist()) <= {0, 1}
        for grid in (1, 2):
            _assert_bitwise(solve(grid), old, "%s, objective scaling, grid %d" % (name, grid), keys=KEYS + ("scale",))
    finally:
        run.eng.set_objective_scaling(0.0)
    _assert_bitwise(run.solve(2), ref, "%s, grid 2 after the option is off again" % name)


def test_batch_sizes_in_turn_on_one_handle(mm):
    """B = 16, 5, 16 at grid 2: the ticket ends at B + grid - 1 before it goes back to 0, a value that changes with B"""
    c = CP.case("0-20-5")
    run = _Run(mm, c, max_batch=16)
    n = run.n
    maps = {16: np.resize(np.arange(n), 16), 5: np.arange(n)[-5:]}
    try:
        old = {B: run.solve(-1, m) for B, m in maps.items()}
        for B in (16, 5):
            assert (old[B]["status"] == 0).all()
        for i, B in enumerate((16, 5, 16)):
            _assert_bitwise(run.solve(2, maps[B]), old[B], "launch %d: B = %d, grid 2" % (i, B))
    finally:
        run.eng.close()


_big = {}


def _big_run(mm, name):
    """the pool tiled to 600 rows under a seeded permutation, as test_the_striding_grid_keeps_instances_apart: handle, device
    inputs, and the rows of the small reference it has to reproduce"""
    if name not in _big:
        c, _, ref = _reference(mm, name)
        n = len(ref["iters"])
        rowmap = np.resize(np.arange(n), BIG_B)[np.random.default_rng(BIG_B + n).permutation(BIG_B)]
        run = _Run(mm, c, max_batch=BIG_B)
        _big[name] = (run, run.inputs(rowmap), {k: v[rowmap] for k, v in ref.items()})
    return _big[name]


@pytest.mark.parametrize("name", BIG_CASES)
def test_launch_orders_in_the_table_and_the_motion_mode(mm, name):
    """600 rows on 64 workgroups (about ten solves deep) in batch order, history order (the second launch sorts by the first one's
    iteration counts) and key order - in the motion mode the key kernel of the record, in front of a persistent launch"""
    run, t, big = _big_run(mm, name)
    try:
        run.eng.set_schedule_hint(0)
        _assert_bitwise(run.solve(-1, t=t), big, "%s x 600, one workgroup per instance" % name)
        _assert_bitwise(run.solve(BIG_GRID, t=t), big, "%s x 600, grid 64, batch order" % name)
        for mode, launches in ((1, 3), (2, 2)):
            run.eng.set_schedule_hint(mode)
            for i in range(launches):
                _assert_bitwise(run.solve(BIG_GRID, t=t), big, "%s x 600, grid 64, schedule hint %d, launch %d" % (name, mode, i))
    finally:
        run.eng.set_schedule_hint(1)


def test_two_handles_on_two_streams(mm):
    """two 600-row batches of different cases, back to back on two streams without a synchronise in between, twice: the tickets are
    per handle, and neither launch may starve the other's reset"""
    import torch
    runs = [_big_run(mm, name) for name in BIG_CASES]
    streams = [torch.cuda.Stream(device=0) for _ in runs]
    torch.cuda.synchronize()
    outs = []
    for rnd in range(2):
        for (run, t, _), st in zip(runs, streams):
            with torch.cuda.stream(st):      # (the sentinel fill of the output set goes to the launch's own stream)
                outs.append(run.launch(t, BIG_GRID, stream=st.cuda_stream))
    torch.cuda.synchronize()
    for i, out in enumerate(outs):
        name, big = BIG_CASES[i % 2], runs[i % 2][2]
        _assert_bitwise({k: v.cpu().numpy() for k, v in out.items()}, big, "%s x 600, round %d, beside the other handle" % (name, i // 2))
