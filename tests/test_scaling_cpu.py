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
