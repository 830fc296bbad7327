"""The instances of the continuation tests (tests/test_continuation_cpu.py, tests/test_gpu_continuation.py), shared by both.
TEST ONLY: numpy, the generators and the host builds of the kernels; never used by the product package.

A solve cut into launches keeps, besides its point, ten scalars (emu_helper.SCALARS).  One that is dropped or restored wrongly
changes nothing unless the cut falls where it is non-zero - and on an ordinary instance prox, nsmall, delta_last and delta_prev
are zero and the filter is far from full at every iteration.  The pools below are the rows of seeded generator batches (and the
five recorded stragglers of tests/golden/c5_tail_cases.npz) on which the host build, cut at EVERY iteration, parks each of those
states non-trivially; test_continuation_cpu.py asserts that (a condition of the pool, not a measurement), so that a sweep of the
same rows over every cut on the GPU cuts where the rare state is live.

A pool is generator arguments plus row indices (at most 16 rows); a case is a pool in one obstacle mode on one host build:
  the four listed shapes                         tests/emu            static record; (0,30,8): the golden per-stage table
  (0,20,5) and (1,15,3) as table / motion twins  tests/emu_motion     the pool's obstacles moving (the generator's velocities),
                                                                      as a per-stage table and as motion record + non-zero tick
  two shape libraries                            tests/emu_shapes     (0,23,2): gains in global memory; (0,12,4): gains in LDS
"""
import ctypes as C
import os

import numpy as np

import emu_helper
import motion_helper
import shape_helper
from oracle import nlp, synth

_HERE = os.path.dirname(os.path.abspath(__file__))

# ---- the pools: (generator arguments, rows), ... per shape ------------------------------------------------------------------------
# Rows with the state named behind them at some cut of the host build (found by tracing the whole batch at a budget of 1).
POOLS = {
    # prox > 0: 62 ... 187; a full filter: 4 ... 34 (and 66); nsmall, delta_last, delta_prev: most of them
    (0, 20, 5): [(dict(B=192, config_id=3), [62, 66, 100, 124, 137, 150, 165, 187, 4, 8, 10, 11, 34])],
    # prox > 0: 12 ... 57; a full filter: 26 ... 107 (and 37, 57)
    (0, 20, 3): [(dict(B=128, config_id=4), [12, 17, 24, 37, 57, 26, 41, 48, 78, 107])],
    (0, 30, 8): "golden",          # all five rows of c5_tail_cases.npz
    # config 2: nsmall > 0 on 865, 1522, 2744; delta_last, delta_prev > 0 on 199, 424, 463 (and 1522, 1892, 2744); a full filter on
    # 1892, the only one of 3000.  config 7: prox > 0 on 1979, the only one of 3000; nsmall > 0 on all three
    (1, 15, 3): [(dict(B=3000, config_id=2), [865, 1522, 2744, 199, 424, 463, 1892]), (dict(B=3000, config_id=7), [1979, 1557, 1634])],
}
# the twins take their own rows of the same batches: with the obstacles moving the solves are other solves
TWIN_POOLS = {
    # prox > 0: 20 ... 168; a full filter: 11 ... 60 (and 115, 168)
    (0, 20, 5): [(dict(B=192, config_id=3), [20, 63, 100, 115, 124, 137, 165, 168, 11, 22, 50, 60])],
    # config 2: nsmall > 0 on 563, 2113, 2688; a full filter on 563, 1892.  config 7: prox > 0 on 612, 1979; nsmall > 0 on all three
    (1, 15, 3): [(dict(B=3000, config_id=2), [563, 2113, 2688, 1892, 92, 127]), (dict(B=3000, config_id=7), [612, 1979, 2024])],
}
# two shapes of shape_helper.SHAPE_LIST, rows of shape_helper.inputs(shape, B=192).  (0,23,2): gains in global memory (the first slim
# horizon); prox > 0 on all but row 30, a full filter on 30, 118, 121, 134, 140, 190.  (0,12,4): gains in LDS; the short horizon
# parks no prox, no nsmall and no full filter on any of the 192 rows - delta_last, delta_prev > 0 on 24, 65, 116, 136, all there are
LIBRARY_POOLS = {
    (0, 23, 2): (192, [12, 62, 70, 118, 121, 134, 140, 190, 30]),
    (0, 12, 4): (192, [24, 65, 116, 136, 0, 1, 2, 3]),
}
LIBRARY_SHAPES = list(LIBRARY_POOLS)
assert all(s in shape_helper.SHAPE_LIST for s in LIBRARY_SHAPES)

G_SCALING = 100.0      # nlp_scaling_max_gradient of the objective-scaling case, (0,20,5)

CASES = ["0-20-5", "0-20-3", "0-30-8", "1-15-3", "0-20-5-table", "0-20-5-motion", "1-15-3-table", "1-15-3-motion",
         "lib-0-23-2", "lib-0-12-4"]
COVERED = [c for c in CASES if c != "lib-0-12-4"]      # the cases whose pool has to reach every rare state


def par_of(kind, N):
    return nlp.BaseParams(N=N) if kind == 1 else nlp.WholeBodyParams(N=N)


def pool_rows(shape, segments, moving=False):
    """the rows of a pool, in the pool's order: dict(x_init [clipped], traj_ref, u_ref, u_last = 0, obs[, obs_vel], row = the
    generator's row index)"""
    k, N, M = shape
    par = par_of(k, N)
    parts = []
    for args, rows in segments:
        d = synth.make_batch(args["B"], N=N, M=M, kind="base" if k == 1 else "wholebody", config_id=args["config_id"], moving=moving)
        parts.append({key: v[np.asarray(rows)] for key, v in d.items()})
        parts[-1]["row"] = np.asarray(rows, np.int64)
    d = {key: np.ascontiguousarray(np.concatenate([p[key] for p in parts])) for key in parts[0]}
    if k == 0:
        d["x_init"] = nlp.clip_x_init(par, d["x_init"])
    d["u_last"] = np.zeros((d["x_init"].shape[0], N, par.nu))
    return par, d


def golden_rows():
    z = np.load(os.path.join(_HERE, "golden", "c5_tail_cases.npz"))
    return par_of(0, 30), dict(x_init=z["x"], traj_ref=z["loc"], u_ref=np.zeros_like(z["ul"]), u_last=z["ul"], obs=z["obs"])


def twin_ticks(row):
    """per-instance ticks, none of them 0 (small ones and counts beyond 2^31, motion_helper.TICKS), by the generator's row index:
    a row is the same instance in whichever pool it stands"""
    nz = motion_helper.TICKS[motion_helper.TICKS != 0]
    return nz[np.asarray(row) % len(nz)].astype(np.int64)


def moving_twins(par, d):
    """the motion record of a pool whose obstacles move (the way motion_helper.motion_inputs builds it: velocities scaled per
    instance, the obstacles where the generator put them at the instance's tick) and the per-stage table it stands for"""
    tick = twin_ticks(d["row"])
    rec = motion_helper.scale_velocities(motion_helper.record(d["obs"], d["obs_vel"]), tick, par.dt)
    rec[..., :2] -= rec[..., 3:] * (tick.astype(np.float64) * par.dt)[:, None, None]
    rec = np.ascontiguousarray(rec)
    return rec, tick, motion_helper.table_twin(rec, tick, par.N, par.dt)


_cases = {}


def case(name):
    """dict(name, shape, mode [0 static, 1 table, 2 motion], par, d [x_init, traj_ref, u_ref, u_last, obs], tick [mode 2], backend,
    library).  Built once and shared: read-only."""
    if name in _cases:
        return _cases[name]
    tick, library = None, False
    if name.startswith("lib-"):
        shape = tuple(int(v) for v in name.split("-")[1:])
        B, rows = LIBRARY_POOLS[shape]
        par, d = shape_helper.inputs(shape, B)
        d = {k: np.ascontiguousarray(v[np.asarray(rows)]) for k, v in d.items()}
        mode, backend, library = 0, "shape", True
    elif name.endswith(("-table", "-motion")):
        shape = tuple(int(v) for v in name.split("-")[:3])
        par, d = pool_rows(shape, TWIN_POOLS[shape], moving=True)
        rec, tick, tab = moving_twins(par, d)
        mode = 2 if name.endswith("-motion") else 1
        d["obs"] = rec if mode == 2 else tab
        d.pop("obs_vel")
        assert (tick != 0).all() and (np.abs(rec[..., 3:]).max(axis=(1, 2)) > 0).all()      # every instance's obstacles do move
        if mode == 1:
            tick = None
        backend = "motion"
    else:
        shape = tuple(int(v) for v in name.split("-"))
        if POOLS[shape] == "golden":
            par, d = golden_rows()
            mode = 1
        else:
            par, d = pool_rows(shape, POOLS[shape])
            mode = 0
        backend = "emu"
    d = {k: np.ascontiguousarray(v, float) for k, v in d.items() if k != "row"}
    for v in d.values():
        v.setflags(write=False)
    B, (k, N, M) = d["x_init"].shape[0], shape
    assert B <= 16 and d["obs"].shape == {0: (B, M, 3), 1: (B, N + 1, M, 3), 2: (B, M, 5)}[mode]
    _cases[name] = dict(name=name, shape=shape, mode=mode, par=par, d=d, tick=tick, backend=backend, library=library)
    return _cases[name]


# ---- the host builds -------------------------------------------------------------------------------------------------------------
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_p = lambda a: a.ctypes.data_as(_dp) if a is not None else None
_i = lambda a: a.ctypes.data_as(_ip)
MAX_ITER = 2000
OUT_KEYS = ("X", "U", "s", "status", "iters", "cost", "err")


class HostRun:
    """One case bound to its host build: launch(budget, resume) runs one launch - uninterrupted (0, 0), budgeted (b, 0) or a
    continuation (0 or b, 1) - on this object's output arrays `out` and save areas `state`."""

    def __init__(self, c):
        self.c = c
        par, d, (k, N, M) = c["par"], c["d"], c["shape"]
        B = self.B = d["x_init"].shape[0]
        if c["backend"] == "emu":
            self._run = emu_helper.FastRun(par, d["x_init"], d["traj_ref"], d["u_ref"], d["u_last"], d["obs"], max_iter=MAX_ITER)
            self.out, self.state, self.scal_offset = self._run.out, self._run.state, self._run.scal_offset
            self.launch = self._run.launch
            return
        self.prm = emu_helper.make_params(par, M, False, max_iter=MAX_ITER)
        self.prm.obs_per_stage = c["mode"]
        if c["backend"] == "motion":
            L = C.CDLL(motion_helper.build())
            self.fn, sd = L.mmpc_emum_solve_fast, L.mmpc_emum_fast_state_doubles(k, N, M)
            self.scal_offset = emu_helper.fast_state_scal_offset(k, N)      # (one constant per (kind, N), whatever the mode)
        else:
            L = shape_helper.lib(c["shape"])
            self.fn, sd = L.mmpc_emush_solve_fast, L.mmpc_emush_fast_state_doubles()
            self.scal_offset = L.mmpc_emush_fast_state_scal_offset()
        assert 0 < self.scal_offset and self.scal_offset + len(emu_helper.SCALARS) <= sd
        self.state = np.full((B, sd), np.nan)
        self.out = dict(X=np.zeros((B, N + 1, par.nx)), U=np.zeros((B, N, par.nu)), s=np.zeros((B, N + 1)), status=np.zeros(B, np.int32),
                        iters=np.zeros(B, np.int32), cost=np.zeros(B), err=np.zeros(B))
        self.tick = None if c["tick"] is None else np.ascontiguousarray(c["tick"], np.int64)

    def launch(self, budget=0, resume=0):
        d, o, k = self.c["d"], self.out, self.c["shape"][0]
        tp = self.tick.ctypes.data_as(C.POINTER(C.c_longlong)) if self.tick is not None else None
        rc = self.fn(k, C.byref(self.prm), self.B, _p(d["x_init"]), _p(d["traj_ref"]), _p(d["u_ref"]), _p(d["u_last"]), _p(d["obs"]), tp,
                     _p(o["X"]), _p(o["U"]), _p(o["s"]), _i(o["status"]), _i(o["iters"]), _p(o["cost"]), _p(o["err"]), 0, int(budget),
                     _p(self.state), int(resume))
        assert rc == 0
        return o

    def snapshot(self):
        return {k: v.copy() for k, v in self.out.items()}


_ref, _chain = {}, {}


def uninterrupted(name):
    """the case's solve in one launch on its host build (once per case; read-only)"""
    if name not in _ref:
        r = HostRun(case(name))
        r.launch(0, 0)
        _ref[name] = r.snapshot()
    return _ref[name]


def warm(name, u_guess, x_guess, mu_init):
    """the case's solve in one launch on its host build from a warm start (mmpc_set_warm_start + the X guess of the launch): U
    guess (B, N, nu), X guess (B, N+1, nx), initial barrier parameter"""
    c = case(name)
    par, d, (k, N, M) = c["par"], c["d"], c["shape"]
    u_guess, x_guess = np.ascontiguousarray(u_guess, float), np.ascontiguousarray(x_guess, float)
    assert u_guess.shape == d["u_last"].shape and x_guess.shape == d["traj_ref"].shape
    if c["backend"] == "emu":
        return emu_helper.solve_batch(par, d["x_init"], d["traj_ref"], d["u_ref"], d["u_last"], d["obs"], x_guess=x_guess, u_guess=u_guess,
                                      fast=True, mu_init=mu_init, max_iter=MAX_ITER)
    r = HostRun(c)
    r.prm.mu_init, r.prm.u_guess = float(mu_init), u_guess.ctypes.data
    fn = C.CDLL(motion_helper.build()).mmpc_emum_solve_fast_guess if c["backend"] == "motion" else shape_helper.lib(c["shape"]).mmpc_emush_solve_fast_guess
    o = r.out
    tp = r.tick.ctypes.data_as(C.POINTER(C.c_longlong)) if r.tick is not None else None
    rc = fn(k, C.byref(r.prm), r.B, _p(d["x_init"]), _p(d["traj_ref"]), _p(d["u_ref"]), _p(d["u_last"]), _p(d["obs"]), tp, _p(o["X"]), _p(o["U"]),
            _p(o["s"]), _i(o["status"]), _i(o["iters"]), _p(o["cost"]), _p(o["err"]), 0, 0, None, 0, _p(x_guess))
    assert rc == 0
    return r.snapshot()


def chain(name):
    """the case cut at every iteration on its host build: (outputs, scal[l, b, :] = emu_helper.SCALARS parked after launch l - NaN
    where instance b was not suspended -, launches, areas[l] = the save areas after launch l); once per case"""
    if name not in _chain:
        r = HostRun(case(name))
        scal, launches, areas = emu_helper.trace_chain(r.launch, r.out["status"], r.state, r.scal_offset, budget=1)
        _chain[name] = (r.snapshot(), scal, launches, areas)
    return _chain[name]


def cut_once(name, budget):
    """a launch with `budget`, then one continuation WITHOUT a budget - what the C ABI runs: (outputs after the first launch,
    outputs after the continuation, save areas after the first launch)"""
    r = HostRun(case(name))
    r.launch(budget, 0)
    first, areas = r.snapshot(), r.state.copy()
    if (first["status"] == 3).any():
        r.launch(0, 1)
    return first, r.snapshot(), areas


def coverage(scal):
    """what the cuts of a chain reach, over all rows: dict of booleans / counts from scal[l, b, :]"""
    S = {n: scal[:, :, i] for i, n in enumerate(emu_helper.SCALARS)}
    with np.errstate(invalid="ignore"):
        drop = (S["nfilt"][1:] < S["nfilt"][:-1])          # (NaN compares false: both cuts exist)
        return dict(prox=int((S["prox"] > 0).sum()), nsmall=int((S["nsmall"] > 0).sum()), delta_last=int((S["delta_last"] > 0).sum()),
                    delta_prev=int((S["delta_prev"] > 0).sum()), filter_full=int((S["nfilt"] == emu_helper.fcap()).sum()),
                    filter_drop=int(drop.sum()), filt_init=sorted(set(S["filt_init"][np.isfinite(S["filt_init"])].astype(int).tolist())),
                    distinct_mu=max((len(set(S["mu"][np.isfinite(S["mu"][:, b]), b].tolist())) for b in range(scal.shape[1])), default=0))


def assert_bitwise(a, b, keys=OUT_KEYS, what="", rows=None):
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if rows is not None:
            x, y = x[rows], y[rows]
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), "%s: %s differs (max |diff| %g)" % (what, k, np.abs(x.astype(float) - y.astype(float)).max())
