"""CPU (host build of the kernel source, tests/emu_generic_cont): the GENERIC kernel's iteration budget and continuation - the
CONT = true instantiations of mmpc_solve_one, what a handle created with cfg.generic_budget runs.

Every case of tests/generic_cont_helper.py - the smallest shapes on which each word the generic kernel carries over an iteration is
live: static obstacles, the terminal-xy equality on a per-stage table and on its motion twin, two half-space planes as written and
as intended, dense weights, the base kind, the pose-reference kind with an X guess, objective scaling - is cut at EVERY iteration, in
the two forms of tests/test_continuation_cpu.py: a chain of launches of one iteration each, and for every budget one budgeted launch
plus one continuation without a budget (what the C ABI runs), the save areas of the two compared word for word.  And the conditions
that keep the sweep from passing vacuously: over the union of a case's rows some cut falls where each rare state is live."""
import subprocess
import os

import numpy as np
import pytest

import generic_cont_helper as H


@pytest.mark.parametrize("name", H.CASES)
def test_budget_zero_on_the_cont_instantiation_is_the_plain_kernel(name):
    """the uninterrupted solve on the CONT = true instantiation (no budget) equals the CONT = false one bitwise"""
    a, b = H.uninterrupted(name, cont=1), H.uninterrupted(name, cont=0)
    assert (b["status"] == 0).all(), b["status"]
    H.assert_bitwise(a, b, what="%s, CONT = true without a budget against CONT = false" % name)
    if H.case(name)["max_gradient"] > 0:
        assert a["scale"].tobytes() == b["scale"].tobytes()


@pytest.mark.parametrize("name", H.CASES)
def test_cut_at_every_iteration_in_a_chain(name):
    """(a) launches of ONE iteration each, every one again with the budget: bitwise the uninterrupted solve"""
    ref = H.uninterrupted(name)
    out, scal, launches, _, _ = H.chain(name)
    assert (ref["status"] == 0).all(), ref["status"]
    assert launches == max(1, int(ref["iters"].max()))
    # instance b is suspended after launch l exactly while l + 1 < its iteration count, and parks iteration l + 1
    parked = np.isfinite(scal[:, :, 4])
    assert np.array_equal(parked, np.arange(1, scal.shape[0] + 1)[:, None] < ref["iters"][None, :])
    for l in range(scal.shape[0]):
        assert (scal[l, parked[l], 4] == l + 1).all() and (scal[l, parked[l], 0] > 0).all(), (name, l)
    H.assert_bitwise(out, ref, what="%s, chain of budget 1" % name)
    if H.case(name)["max_gradient"] > 0:
        assert out["scale"].tobytes() == ref["scale"].tobytes()       # (scale_out gets the factor again at every continuation)


@pytest.mark.parametrize("name", H.CASES)
def test_every_budget_plus_one_continuation(name):
    """(b) for every budget b from 1 to the largest iteration count: a launch with the budget, then ONE continuation without a
    budget - bitwise the uninterrupted solve; after the first launch exactly the rows with more than b iterations are suspended,
    at iteration b, and the others are final.  The save area after one launch of b iterations is, word for word, the area the chain
    holds after b launches of one iteration: a word that is saved or restored wrongly shows at the next cut even where it does
    not (yet) change the path of the solve."""
    ref = H.uninterrupted(name)
    areas = H.chain(name)[3]
    for b in range(1, int(ref["iters"].max()) + 1):
        first, final, area = H.cut_once(name, b)
        susp = ref["iters"] > b
        if susp.any():
            assert np.isfinite(area[susp]).all(), (name, b)
            assert area[susp].tobytes() == areas[b - 1][susp].tobytes(), "%s: the save areas at cut %d differ on rows %s" % (
                name, b, [r for r in np.flatnonzero(susp) if area[r].tobytes() != areas[b - 1][r].tobytes()])
        assert np.array_equal(first["status"] == 3, susp), (name, b)
        assert (first["iters"][susp] == b).all(), (name, b)
        H.assert_bitwise(first, ref, what="%s, budget %d, rows that end within it" % (name, b), rows=~susp)
        H.assert_bitwise(final, ref, what="%s, budget %d + continuation" % (name, b))


RARE = ("prox", "nsmall", "delta_last", "delta_prev", "filter_full", "filter_drop")
# States a case's rows do not reach, by name, with the search made; structural zeros of the kernel are named the same way.
#  * the equality cases - prox, nsmall, delta_last, delta_prev: pinned to zero by the kernel under the terminal equality (`!teq` guards
#    mmpc_prox_update and the start of the inertia correction; the second rung there is Gauss-Newton, no delta_w): structural.
#  * "wb-12-2" - a full filter: none of make_batch(1536, N=12, M=2, config_id=3) parks one (8 to 25 iterations a row; the filter
#    is emptied at every change of mu and never collects 16 entries in between), every cut of every row traced.
#  * "base-10-2" - prox, nsmall, delta_last, delta_prev, a full filter: none of make_batch(3000, N=10, M=2, kind="base", config_id=2)
#    and none of the same with config_id=7 parks any of them (six or seven iterations a row, no crawling step, no lost pivot), every
#    cut of every row traced.  The base kind's park / resume code is the whole-body kind's (one template); those words are cut live on
#    the other cases.
UNREACHED = {
    "wb-20-3-teq-table": ("prox", "nsmall", "delta_last", "delta_prev"),
    "wb-20-3-teq-motion": ("prox", "nsmall", "delta_last", "delta_prev"),
    "wb-12-2": ("filter_full",),
    "base-10-2": ("prox", "nsmall", "delta_last", "delta_prev", "filter_full"),
}


@pytest.mark.parametrize("name", H.CASES)
def test_the_rows_cut_where_the_rare_state_is(name):
    """a condition of the rows: at some cut of the chain (over the union of the case's rows) each of prox > 0, nsmall > 0,
    delta_last > 0, delta_prev > 0, a full filter, a filter smaller than at the cut before, at least five distinct mu on one row;
    on the equality cases non-zero terminal multipliers; on the as-written case a non-zero border-variable word; on the scaled case
    a factor below 1 (and a row with factor 1) - or the state is named in UNREACHED, where the kernel must then indeed not reach it"""
    _, scal, _, areas, layout = H.chain(name)
    cov = H.coverage(scal, areas, layout)
    print(name, cov)
    for key in RARE:
        if key in UNREACHED.get(name, ()):
            assert cov[key] == 0, (name, key, "listed as unreached, but reached: take it off the list", cov)
        else:
            assert cov[key] > 0, (name, key, cov)
    assert cov["distinct_mu"] >= 5, (name, cov)
    c = H.case(name)
    if name in H.EQUALITY_CASES:
        assert cov["nueq"] > 0, (name, cov)
    else:
        assert cov["nueq"] == 0, (name, cov)
    if c["as_written"]:
        assert cov["border"] > 0, (name, cov)
    if c["max_gradient"] > 0:
        assert cov["sigma_lt1"] > 0 and cov["sigma_eq1"] > 0, (name, cov)
        sig = H.uninterrupted(name)["scale"]
        assert (sig < 1).any() and (sig == 1).any(), sig
    else:
        assert cov["sigma_lt1"] == 0


def test_the_motion_twin_is_the_table_case():
    """the two equality cases are one problem in two obstacle modes: bitwise equal solves (so the motion case cuts the same states)"""
    H.assert_bitwise(H.uninterrupted("wb-20-3-teq-motion"), H.uninterrupted("wb-20-3-teq-table"), what="motion twin against its table")
    assert (H.case("wb-20-3-teq-motion")["tick"] != 0).all()


def test_save_area_size_documented_in_the_header():
    """include/mmpc.h documents the generic save area per instance with the figure for (whole-body, 30, 8): 26 264 bytes"""
    spec = dict(kind="wholebody", N=30, M=8, gen=dict(B=1, config_id=5), rows=[0])
    r = H.HostRun(H.make_case(spec))
    N, nx, nu, R = 30, 9, 5, r.R
    assert R == 2 * nu + 2 * nx + 8 + 4
    assert 8 * r.layout["total"] == 8 * (2 * (N + 1) * nx + N * nu + (N + 1) + 2 * (N + 1) * R + 64) == 26264
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "mmpc.h")).read()
    assert "26 264 bytes" in hdr and "generic_budget" in hdr


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """the same translation unit as a stand-alone program (its own main) built with -fsanitize=address,undefined: a (12, 2) batch
    uninterrupted and as a chain of one-iteration launches, bitwise equal, no report on an access of the park / resume code"""
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "gcont_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wno-unknown-pragmas",
                           "-ffp-contract=off", "-DMMPC_EMUG_MAIN", "-o", exe, os.path.join(here, "emu_generic_cont", "mmpc_emu_gcont.cpp")],
                          stderr=subprocess.DEVNULL)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "bitwise equal" in p.stdout, (p.stdout, p.stderr[-2000:])
    assert "AddressSanitizer" not in p.stderr, p.stderr[-2000:]
