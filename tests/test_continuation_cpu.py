"""CPU (host build of the kernel source): a solve cut into launches of at most `budget` iterations - suspended, state
written to the save area, resumed - runs exactly the iterations of the uninterrupted solve: bitwise equal outputs.

Below the two cases on ordinary instances: every case of tests/continuation_pool.py - the four listed shapes, the table and
motion twins, two shape libraries - cut at EVERY iteration, in both forms (a chain of launches of one iteration each; one
budgeted launch plus one continuation without a budget, what the C ABI runs; the save areas of the two compared word for word),
and the condition that makes the sweep worth its time: the pools' cuts fall where prox, nsmall, delta_last, delta_prev are
non-zero, the filter is full, the filter has just been emptied, and the barrier parameter has changed several times."""
import numpy as np
import pytest

import continuation_pool as CP
import emu_helper
import scaling_helper
from oracle import nlp, synth


@pytest.mark.parametrize("kind,N,M,cid,budget", [("wholebody", 20, 5, 3, 7), ("base", 15, 3, 2, 3)])
def test_budgeted_launches_equal_the_uninterrupted_solve(kind, N, M, cid, budget):
    B = 6
    d = synth.make_batch(B, N=N, M=M, kind=kind, config_id=cid)
    par = nlp.WholeBodyParams(N=N) if kind == "wholebody" else nlp.BaseParams(N=N)
    xi = nlp.clip_x_init(par, d["x_init"]) if kind == "wholebody" else d["x_init"]
    ul = np.zeros((B, N, par.nu))
    ref = emu_helper.solve_batch(par, xi, d["traj_ref"], d["u_ref"], ul, d["obs"], fast=True, max_iter=2000)
    cut, launches = emu_helper.solve_fast_budgeted(par, xi, d["traj_ref"], d["u_ref"], ul, d["obs"], budget, max_iter=2000)
    assert (ref["status"] == 0).all() and (cut["status"] == 0).all()
    assert launches == int(np.ceil(ref["iters"].max() / budget)) or launches == int(np.ceil((ref["iters"].max() + 1) / budget))
    for k in ("X", "U", "s", "iters", "cost", "err"):
        assert np.array_equal(ref[k], cut[k]), k


def test_the_scalars_are_read_where_the_kernel_writes_them():
    """the offset of the scalars comes from the kernel's constants; what is read there is what the park code wrote: scalar 4 is
    the iteration count of the cut, on every case"""
    assert emu_helper.SCALARS[4] == "it" and len(emu_helper.SCALARS) == 10
    for name in CP.CASES:
        scal = CP.chain(name)[1]
        it = scal[:, :, 4]
        for l in range(scal.shape[0]):
            parked = np.isfinite(it[l])
            assert parked.any() and (it[l][parked] == l + 1).all(), (name, l)
            assert np.isfinite(scal[l][parked]).all() and (scal[l][parked][:, 0] > 0).all(), (name, l)      # mu > 0
    # the helper of emu_helper on its own gives the trace of the pool module
    c = CP.case("1-15-3")
    d = c["d"]
    out, scal, launches = emu_helper.solve_fast_chain(c["par"], d["x_init"], d["traj_ref"], d["u_ref"], d["u_last"], d["obs"], max_iter=CP.MAX_ITER)
    ref = CP.chain("1-15-3")
    assert launches == ref[2] and scal.tobytes() == ref[1].tobytes()
    CP.assert_bitwise(out, ref[0], what="solve_fast_chain")


@pytest.mark.parametrize("name", CP.CASES)
def test_cut_at_every_iteration_in_a_chain(name):
    """(a) launches of ONE iteration each, every one again with the budget: bitwise the uninterrupted solve"""
    ref = CP.uninterrupted(name)
    out, scal, launches, _ = CP.chain(name)
    assert (ref["status"] == 0).all(), ref["status"]
    assert launches == max(1, int(ref["iters"].max()))
    # instance b is suspended after launch l exactly while l + 1 < its iteration count
    assert np.array_equal(np.isfinite(scal[:, :, 4]), np.arange(1, scal.shape[0] + 1)[:, None] < ref["iters"][None, :])
    CP.assert_bitwise(out, ref, what="%s, chain of budget 1" % name)


@pytest.mark.parametrize("name", CP.CASES)
def test_every_budget_plus_one_continuation(name):
    """(b) for every budget b from 1 to the largest iteration count: a launch with the budget, then ONE continuation without a
    budget - bitwise the uninterrupted solve; after the first launch exactly the rows with more than b iterations are suspended,
    at iteration b, and the others are final.
    And the save area does not depend on how the solve got there: what one launch of b iterations parks is, word for word, what
    the chain parks after b launches of one iteration - b - 1 continuations, each from the area the launch before it wrote.  So
    a word that is saved or restored wrongly shows at the next cut even where it does not (yet) change the path of the solve:
    the sixteenth entry of a full filter, th_min, the row state of every lane."""
    ref = CP.uninterrupted(name)
    areas = CP.chain(name)[3]
    for b in range(1, int(ref["iters"].max()) + 1):
        first, final, area = CP.cut_once(name, b)
        susp = ref["iters"] > b
        if susp.any():
            assert area[susp].tobytes() == areas[b - 1][susp].tobytes(), "%s: the save areas at cut %d differ on rows %s" % (
                name, b, [r for r in np.flatnonzero(susp) if area[r].tobytes() != areas[b - 1][r].tobytes()])
        assert np.array_equal(first["status"] == 3, susp), (name, b)
        assert (first["iters"][susp] == b).all(), (name, b)
        CP.assert_bitwise(first, ref, what="%s, budget %d, rows that end within it" % (name, b), rows=~susp)
        CP.assert_bitwise(final, ref, what="%s, budget %d + continuation" % (name, b))


RARE = ("prox", "nsmall", "delta_last", "delta_prev", "filter_full", "filter_drop")
# States a pool does not reach within the batches it is drawn from, by name, with the search made.
# "filt_init_0", every case: filt_init = 0 at a cut is not reachable on any shape.  The flag is 0 before the first iteration and
# from a change of mu (behind the park point of that iteration) to the filter's set-up of the same iteration, which sets it to 1
# before `it` is counted up; a launch parks only after at least one iteration of its own, so a parked solve always holds 1.  Traced
# to confirm, every cut of: make_batch(192, N=20, M=5, config_id=3), make_batch(128, N=20, M=3, config_id=4), the base kind's
# make_batch(3000, N=15, M=3, config_id=2 and 7) - each static and with moving obstacles - and the five c5_tail_cases rows: 1 at
# every one.  (A continuation that lost the flag would empty a filter that holds entries, which the bitwise sweeps see.)
UNREACHED = {name: ("filt_init_0",) for name in CP.COVERED}


@pytest.mark.parametrize("name", CP.COVERED)
def test_the_pool_cuts_where_the_rare_state_is(name):
    """(d) a condition of the pool: at some cut of the chain (over the union of the pool's rows) each of prox > 0, nsmall > 0,
    delta_last > 0, delta_prev > 0, a full filter, a filter smaller than at the cut before (a reset, or a new mu), the values of
    filt_init that a cut can see (UNREACHED), and at least five distinct mu on one row"""
    cov = CP.coverage(CP.chain(name)[1])
    print(name, cov)
    for key in RARE:
        assert key not in UNREACHED.get(name, ())
        assert cov[key] > 0, (name, key, cov)
    assert cov["filt_init"] == ([1] if "filt_init_0" in UNREACHED.get(name, ()) else [0, 1]), (name, cov)
    assert cov["distinct_mu"] >= 5, (name, cov)


def test_the_scaled_pool_has_a_scaled_row_and_keeps_its_factor_over_a_cut():
    """at nlp_scaling_max_gradient = 100 the (0,20,5) pool has scaled and unscaled rows (the numpy factor and the host build's);
    with the option on, every budget plus one continuation is bitwise the uninterrupted scaled solve (scalar 10 of the save area)"""
    c = CP.case("0-20-5")
    sig, _ = scaling_helper.sigma_numpy(c["par"], c["d"], CP.G_SCALING)
    assert (sig < 1).any() and (sig == 1).any(), sig
    ref = scaling_helper.solve(c["par"], c["d"], max_gradient=CP.G_SCALING, fast=True, max_iter=CP.MAX_ITER)
    assert ((ref["scale"] < 1) == (sig < 1)).all() and np.abs(ref["scale"] / sig - 1).max() <= 1e-13
    assert (ref["status"] == 0).all()
    off = CP.uninterrupted("0-20-5")
    assert any(ref["X"][b].tobytes() != off["X"][b].tobytes() for b in np.flatnonzero(sig < 1))      # another solve than the unscaled one
    for b in range(1, int(ref["iters"].max()) + 1):
        cut = scaling_helper.solve(c["par"], c["d"], max_gradient=CP.G_SCALING, fast=True, budget=b, max_iter=CP.MAX_ITER)
        CP.assert_bitwise(cut, ref, what="scaled, budget %d + continuation" % b)
        assert cut["launches"] == (2 if (ref["iters"] > b).any() else 1)
