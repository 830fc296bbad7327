"""CPU: the objective scaling (mmpc_set_objective_scaling; IPOPT's nlp_scaling_method = gradient-based) of both solver kernels in
the host emulation (tests/emu_scaling/mmpc_emu_scaling.cpp): the factor against numpy, the solve against the C oracle's solve of
the instance with its weights times the factor, and - bit for bit - against the emulation's own solve of that twin."""
import numpy as np
import pytest

import emu_helper
import scaling_helper as sh

G = sh.G_IPOPT
CASES = [("fast",) + c for c in sh.FAST] + [("generic",) + c for c in sh.GENERIC]
_cache = {}


def _case(case):
    """inputs (built once, never changed), the solve with the option on and the one with it off"""
    if case not in _cache:
        fast = case[0] == "fast"
        par, d, sig = (sh.fast_inputs if fast else sh.generic_inputs)(*case[1:])
        _cache[case] = dict(par=par, d=d, sig=sig, fast=fast, on=sh.solve(par, d, G, fast=fast), off=sh.solve(par, d, 0.0, fast=fast))
    return _cache[case]


@pytest.mark.parametrize("case", CASES, ids=str)
def test_factor_equals_numpy(case):
    c = _case(case)
    assert np.abs(c["on"]["scale"] / c["sig"] - 1).max() <= 1e-13
    assert ((c["on"]["scale"] == 1) == (c["sig"] == 1)).all()
    assert (c["off"]["scale"] == -1).all()      # off: nothing is written


@pytest.mark.parametrize("case", CASES, ids=str)
def test_parity_with_the_oracle_on_scaled_weights(case):
    """the tolerances of tests/test_emu_kernel.py (_cmp); cost against the oracle's scaled cost / sigma"""
    c = _case(case)
    e = c["on"]
    o = sh.oracle_scaled(c["par"], c["d"], c["sig"])
    print("iters emu", e["iters"], "oracle", o["iters"], "dX %.2e dU %.2e ds %.2e" % (np.abs(o["X"] - e["X"]).max(), np.abs(o["U"] - e["U"]).max(), np.abs(o["s"] - e["s"]).max()))
    assert (o["status"] == 0).all() and (e["status"] == 0).all()
    assert (np.abs(o["iters"] - e["iters"]) <= 2).mean() > 0.8
    assert np.abs(o["X"] - e["X"]).max() < 1e-6 and np.abs(o["U"] - e["U"]).max() < 1e-6 and np.abs(o["s"] - e["s"]).max() < 1e-6
    assert np.abs(e["cost"] / (o["cost"] / c["sig"]) - 1).max() <= 1e-9


@pytest.mark.parametrize("shape", sh.FAST, ids=str)
@pytest.mark.parametrize("fast", [True, False], ids=["fast", "generic"])
def test_twin_bitwise(shape, fast):
    """diagonal weights: instance b with the option on = instance b alone with the option off and Q, P, R, W, S x sigma_b"""
    c = _case(("fast",) + shape)
    par, d = c["par"], c["d"]
    on = c["on"] if fast else sh.solve(par, d, G)
    assert np.abs(on["scale"] / c["sig"] - 1).max() <= 1e-13
    changed = 0
    for b in range(d["x_init"].shape[0]):
        sg = on["scale"][b]
        tw = sh.solve(sh.scaled_par(par, sg), sh.instance(d, b), 0.0, fast=fast)
        sh.assert_bitwise({k: on[k][b:b + 1] for k in sh.BIT_KEYS}, tw, what="instance %d" % b)
        assert abs(on["cost"][b] / (tw["cost"][0] / sg) - 1) <= 1e-12
        changed += int(on["iters"][b] != c["off"]["iters"][b]) if fast else 0
    if fast:
        assert changed > 0      # the scaled solve is another solve than the unscaled one


@pytest.mark.parametrize("case", CASES, ids=str)
def test_factor_one_is_the_unscaled_solve_bitwise(case):
    """max_gradient = 1e30: the gradient phase runs, every factor is 1, and the outputs are those of the option off"""
    c = _case(case)
    r = sh.solve(c["par"], c["d"], 1e30, fast=c["fast"])
    assert (r["scale"] == 1).all()
    sh.assert_bitwise(r, c["off"], keys=sh.BIT_KEYS + ("cost",), what="sigma = 1")


@pytest.mark.parametrize("case", CASES, ids=str)
def test_reverse_lane_order(case):
    c = _case(case)
    r = sh.solve(c["par"], c["d"], G, fast=c["fast"], reverse=True)
    sh.assert_bitwise(r, c["on"], keys=sh.BIT_KEYS + ("cost", "scale"), what="reversed lanes")


@pytest.mark.parametrize("shape,budget", [((0, 20, 5), 7), ((1, 15, 3), 3)], ids=str)
def test_budgeted_and_resumed_equals_uninterrupted(shape, budget):
    c = _case(("fast",) + shape)
    r = sh.solve(c["par"], c["d"], G, fast=True, budget=budget)
    assert r["launches"] == 2 and (c["on"]["iters"] > budget).sum() >= 8
    sh.assert_bitwise(r, c["on"], keys=sh.BIT_KEYS + ("cost", "scale"), what="budget %d" % budget)


def test_layout_unchanged():
    """every *_lds_doubles of this library equals the existing emulation's for the same arguments"""
    import ctypes as C
    lib = C.CDLL(emu_helper.build())
    for kind, N, M in sh.FAST:
        for mode in (0, 1, 2):
            assert sh.fast_lds_doubles(kind, N, M, mode) == lib.mmpc_emu_fast_lds_doubles(kind, N, M, mode) > 0
    for kind in (0, 1, 2):
        for N, M in ((6, 2), (5, 1), (20, 5), (30, 8), (49, 0), (35, 16)):
            for mode in (0, 1, 2):
                for nhs, nq in ((0, 0), (6, 0), (6, 6)) if kind == 0 else ((0, 0),):
                    assert sh.lds_doubles(kind, N, M, mode, nhs, nq) == lib.mmpc_emu_lds_doubles(kind, N, M, mode, nhs, nq) > 0
    for kind, N, M in ((0, 20, 5), (0, 20, 3), (1, 15, 3)):
        assert C.CDLL(sh.build()).mmpc_emus_fast_state_doubles(kind, N, M) == lib.mmpc_emu_fast_state_doubles(kind, N, M) > 0


# ---- the gradient term by term: one-hot instances (sh.onehot_inputs), one iteration - the factor is written before the first
ONEHOT = ([(kern,) + s + (False,) for s in sh.ONEHOT_SHAPES for kern in ("fast", "generic")]
          + [("generic",) + s + (True,) for s in sh.ONEHOT_DENSE] + [("generic", "pose", 6, 2, False), ("generic", "pose", 6, 2, True)])
_onehot = {}


def onehot_case(kind, N, M, dense, variant):
    """inputs of a one-hot case (built once, never changed; the builder asserts the hot value against numpy)"""
    key = (kind, N, M, dense, variant)
    if key not in _onehot:
        _onehot[key] = sh.onehot_inputs(kind, N, M, variant, dense)
    return _onehot[key]


def onehot_assert(scale, status, sig):
    print("instances %d, mismatches %d, max |scale / sigma - 1| %.3g" % (len(sig), int((np.abs(scale / sig - 1) > 1e-13).sum()), np.abs(scale / sig - 1).max()))
    assert (status == 1).all()          # one iteration: nobody converges, and nobody fails
    assert np.abs(scale / sig - 1).max() <= 1e-13
    assert ((scale == 1) == (sig == 1)).all()


# (the pose-reference kind has no state entries to cover, sh.onehot_entries: no "xguess" case)
@pytest.mark.parametrize("case,variant", [(c, v) for c in ONEHOT for v in sh.ONEHOT_VARIANTS if not (c[1] == "pose" and v == "xguess")], ids=str)
def test_onehot_factor(case, variant):
    """every entry of grad f(w0) decides the factor of one instance: a missed entry gives sigma = 1, a wrong one another factor"""
    kern, kind, N, M, dense = case
    par, d, sig, g = onehot_case(kind, N, M, dense, variant)
    r = sh.solve(par, d, G, fast=kern == "fast", max_iter=1)
    onehot_assert(r["scale"], r["status"], sig)


# ---- full solves whose factor another term than Q (x0 - x_ref_k) decides (sh.decider_inputs)
DECIDERS = [(name,) + s for s in sh.DECIDER_SHAPES for name in sh.DECIDERS]
_decider = {}


def decider_case(case):
    if case not in _decider:
        par, d, sig = sh.decider_inputs(*case)
        fast = case[1] in (0, 1)
        _decider[case] = dict(par=par, d=d, sig=sig, fast=fast, on=sh.solve(par, d, G, fast=fast), off=sh.solve(par, d, 0.0, fast=fast))
    return _decider[case]


@pytest.mark.parametrize("case", DECIDERS, ids=str)
def test_decider_factor_and_oracle(case):
    """the assertions of test_factor_equals_numpy and test_parity_with_the_oracle_on_scaled_weights, unchanged"""
    c = decider_case(case)
    e = c["on"]
    assert np.abs(e["scale"] / c["sig"] - 1).max() <= 1e-13
    assert ((e["scale"] == 1) == (c["sig"] == 1)).all()
    o = sh.oracle_scaled(c["par"], c["d"], c["sig"])
    print("iters emu", e["iters"], "oracle", o["iters"], "dX %.2e dU %.2e ds %.2e" % (np.abs(o["X"] - e["X"]).max(), np.abs(o["U"] - e["U"]).max(), np.abs(o["s"] - e["s"]).max()))
    assert (o["status"] == 0).all() and (e["status"] == 0).all()
    assert (np.abs(o["iters"] - e["iters"]) <= 2).mean() > 0.8
    assert np.abs(o["X"] - e["X"]).max() < 1e-6 and np.abs(o["U"] - e["U"]).max() < 1e-6 and np.abs(o["s"] - e["s"]).max() < 1e-6
    assert np.abs(e["cost"] / (o["cost"] / c["sig"]) - 1).max() <= 1e-9


# the specialised shapes on both kernels, the ("wb", 6, 2) cases on the generic one (which scales its own copy of R2 + W2)
DECIDER_TWINS = [(kern, c) for c in DECIDERS for kern in ("fast", "generic") if kern == "generic" or c[1] in (0, 1)]


@pytest.mark.parametrize("kern,case", DECIDER_TWINS, ids=str)
def test_decider_twin_bitwise(kern, case):
    """instance b with the option on = instance b alone (its guesses too) with the option off and Q, P, R, W, S x sigma_b"""
    c = decider_case(case)
    par, d, fast = c["par"], c["d"], kern == "fast"
    on, off = (c["on"], c["off"]) if fast == c["fast"] else (sh.solve(par, d, G), sh.solve(par, d, 0.0))
    assert np.abs(on["scale"] / c["sig"] - 1).max() <= 1e-13
    changed = 0
    for b in range(d["x_init"].shape[0]):
        sg = on["scale"][b]
        tw = sh.solve(sh.scaled_par(par, sg), sh.instance(d, b), 0.0, fast=fast)
        sh.assert_bitwise({k: on[k][b:b + 1] for k in sh.BIT_KEYS}, tw, what="instance %d" % b)
        assert abs(on["cost"][b] / (tw["cost"][0] / sg) - 1) <= 1e-12
        changed += int(on["X"][b].tobytes() != off["X"][b].tobytes())
    # the scaled solve is another solve than the unscaled one (in its iterates: these short solves keep their iteration counts)
    assert changed >= (c["sig"] < 1).sum() > 0


DECIDER_BUDGET = (("W", 0, 20, 3), 4)


def test_decider_budgeted_and_resumed_with_a_guess():
    """the factor travels through the save area together with a guess: the continuation does not form it again"""
    case, budget = DECIDER_BUDGET
    c = decider_case(case)
    r = sh.solve(c["par"], c["d"], G, fast=True, budget=budget)
    assert r["launches"] == 2 and (c["on"]["iters"] > budget).all()
    sh.assert_bitwise(r, c["on"], keys=sh.BIT_KEYS + ("cost", "scale"), what="budget %d" % budget)


# ---- receding horizon: the factor at ticks >= 1 (the tick kernel's host build feeds the emulation, as DeviceFleet(fused=True) does)
@pytest.mark.parametrize("warm_start", ["shifted", "reference"])
def test_fleet_ticks_factor(warm_start):
    """every tick's factor is numpy's at that tick's own starting point - u_last = the previous optimum, and the shifted guess and
    its roll-out when there are some; the shifted run has a tick whose factor the guess decides; its last tick equals its twin"""
    import tick_emu_helper as H
    par, x, glob, obs0, vel = sh.fleet_plan()
    B, N, M, Tn = (sh.FLEET[k] for k in "BNMT")
    tick = np.zeros(B, np.int64)
    prev, decided = None, 0
    for t in range(Tn):
        warm = warm_start == "shifted" and prev is not None
        want = ("x_in", "traj_ref", "obs") + (("u_guess", "x_guess") if warm else ())
        p = H.prepare(N, M, par.dt, par.xlim, x, tick, U_prev=prev, glob=glob, obs0=obs0, vel=vel, want=want)
        x, tick = p["x"], p["tick"]
        d = sh.tick_inputs(p["x_in"], p["traj_ref"], p["obs"], prev if prev is not None else np.zeros((B, N, 5)), p.get("u_guess"), p.get("x_guess"))
        sig = sh.sigma_numpy(par, d)[0]
        r = sh.solve(par, d, G, fast=True, mu_init=0.1 if warm else 1.0)
        print("tick", t, "sigma", np.round(sig, 4), "iters", r["iters"])
        assert (r["status"] == 0).all()
        assert np.abs(r["scale"] / sig - 1).max() <= 1e-13 and ((r["scale"] == 1) == (sig == 1)).all()
        if t >= 1:
            assert np.abs(d["u_last"]).max() > 0.1
        if warm:
            decided += int(sh.guess_decides(par, d).sum())
        prev = r["U"]
    if warm_start == "shifted":
        assert decided > 0          # otherwise nothing here sees which point the factor was formed at
        for b in range(B):
            sg = r["scale"][b]
            tw = sh.solve(sh.scaled_par(par, sg), sh.instance(d, b), 0.0, fast=True, mu_init=0.1)
            sh.assert_bitwise({k: r[k][b:b + 1] for k in sh.BIT_KEYS}, tw, what="tick %d, instance %d" % (t, b))
