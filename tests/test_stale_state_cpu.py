"""CPU (host builds of the kernel source): no solve reads what it has not written.

On the device a workgroup starts on another workgroup's LDS, and under the persistent plain launch (mmpc_set_persistent_grid) an
instance starts on its predecessor's slab, gain block, correction scratch and registers.  The host builds used to give every
instance a fresh slab of NaN, which is blind exactly where a stale read is most likely to hide: the max / min reductions and most
guards are comparisons, and a NaN on one side of `x > y ? x : y` is silently dropped.  Their lane state is static and simply
carried over from the previous solve of the process.

Here both are the test's (tests/emu_common/mmpc_emu_poison.h through tests/poison_helper.py): the blocks start as the predecessor
left them (`keep`, in pool order and reversed), as seeded finite noise, +-1e300, +-inf, 0 or a denormal, and the lane state is
overwritten with a byte pattern at the entry of every solve, continuations included.  Every output - and scale_out, and the save
areas of a chain - has to be bit for bit what the NaN slab gives.  A difference is a read of a word the solve did not initialise:
a bug of the kernel source, on every launch form.  tests/test_gpu_persistent_reuse.py asks the same of the device."""
import ctypes as C

import numpy as np
import pytest

import continuation_pool as CP
import emu_helper
import generic_cont_helper as GH
import manipulate_emu_helper as MAH
import mission_emu_helper as MIH
import motion_helper
import poison_helper as PH
import scaling_helper as SH
import shape_helper
import tick_emu_helper as TH
from oracle import nlp, synth

# what an uninterrupted solve is put through: every fill (keep: the predecessor in pool order), keep behind the successor
# instead, and the four lane patterns on the default slab
VARIANTS = [(m, -1, False) for m in PH.MODES[1:]] + [("keep", -1, True)] + [("nan", p, False) for p in PH.LANE_PATTERNS]
VARIANT_IDS = ["%s%s%s" % (m, "-reversed" if r else "", "" if p < 0 else "-lane-%02X" % p) for m, p, r in VARIANTS]
CHAIN_LANES = (0x43, 0xFF)      # the budget-1 chains: seeded noise in every block and one of these in the lane state


def _bitwise(a, b, keys, what):
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), \
            "%s: %s differs in rows %s" % (what, k, np.flatnonzero((x != y).reshape(len(x), -1).any(axis=1) | (np.isnan(x) != np.isnan(y)).reshape(len(x), -1).any(axis=1)).tolist())


def _flip(v):
    return None if v is None else np.ascontiguousarray(v[::-1])


# ---- the solver cases: name -> (host library, solve(reversed) -> outputs, keys) -------------------------------------------------
def _pool_lib(c):
    return {"emu": lambda: C.CDLL(emu_helper.build()), "motion": lambda: C.CDLL(motion_helper.build()),
            "shape": lambda: shape_helper.lib(c["shape"])}[c["backend"]]()


def _pool_case(c, rev):
    """the pool's case, or the same rows in reversed order"""
    return dict(c, d={k: _flip(v) for k, v in c["d"].items()}, tick=_flip(c["tick"])) if rev else c


def _pool_specialised(name):
    c = CP.case(name)

    def solve(rev=False):
        r = CP.HostRun(_pool_case(c, rev))
        r.launch(0, 0)
        return r.snapshot()
    return _pool_lib(c), solve, CP.OUT_KEYS


def _pool_generic(name):
    """the generic kernel on the pool's rows, on the same host library"""
    c = CP.case(name)

    def solve(rev=False):
        cc = _pool_case(c, rev)
        par, d = cc["par"], cc["d"]
        if cc["backend"] == "emu":
            return emu_helper.solve_batch(par, d["x_init"], d["traj_ref"], d["u_ref"], d["u_last"], d["obs"], max_iter=CP.MAX_ITER)
        if cc["backend"] == "motion":
            return motion_helper.solve(par, d["x_init"], d["traj_ref"], d["u_ref"], d["u_last"], d["obs"], tick=cc["tick"], mode=cc["mode"],
                                       max_iter=CP.MAX_ITER)
        return shape_helper.solve(cc["shape"], par, d, fast=False, max_iter=CP.MAX_ITER)
    return _pool_lib(c), solve, CP.OUT_KEYS


def _terminal_xy_inputs():
    """tests/test_emu_kernel.py, test_emu_terminal_xy_equality"""
    d = synth.make_batch(6)
    par = nlp.WholeBodyParams()
    par.terminal_xy_equality = True
    x0 = np.clip(d["x_init"], par.xlim[0], par.xlim[1])
    d["traj_ref"][:, :, :2] = x0[:, None, :2] + 0.5 * (d["traj_ref"][:, :, :2] - x0[:, None, :2])
    return par, dict(x_init=d["x_init"], traj_ref=d["traj_ref"], u_ref=d["u_ref"], u_last=np.zeros((6, 20, 5)), obs=d["obs"]), {}


def _halfspace_inputs():
    """tests/test_emu_kernel.py, test_emu_halfspace_obstacles_c1: the demo's two planes, the second start beside them.  (Four rows:
    the two starts twice, so that under `keep` each of them runs behind the other one.)"""
    import test_emu_kernel
    d, hs = test_emu_kernel._c1_inputs()
    d = {k: np.concatenate([v, v]) for k, v in d.items()}
    return nlp.WholeBodyParams(), dict(d, u_last=np.zeros((4, 20, 5))), dict(hs=hs)


def _pose_inputs():
    """tests/test_emu_kernel.py, test_emu_pose_reference_controller"""
    x0, ref, obs = emu_helper.pose_batch(6, 10)
    return nlp.pose_ref_params(N=10), dict(x_init=x0, traj_ref=ref, u_ref=np.zeros((6, 10, 5)), u_last=np.zeros((6, 10, 5)), obs=obs), {}


_EXTRA = {"terminal-xy": _terminal_xy_inputs, "half-space": _halfspace_inputs, "pose-reference": _pose_inputs}
_extra_inputs = {}


def _extra(name):
    """the generic kernel's configurations that no pool has, on tests/emu"""
    if name not in _extra_inputs:
        _extra_inputs[name] = _EXTRA[name]()
    par, d, kw = _extra_inputs[name]

    def solve(rev=False):
        dd = {k: _flip(v) for k, v in d.items()} if rev else d
        return emu_helper.solve_batch(par, dd["x_init"], dd["traj_ref"], dd["u_ref"], dd["u_last"], dd["obs"], **kw)
    return C.CDLL(emu_helper.build()), solve, CP.OUT_KEYS


SCALING_CASES = [("fast",) + c for c in SH.FAST] + [("generic",) + c for c in SH.GENERIC]      # those of tests/test_scaling_cpu.py
_scaling_inputs = {}


def _scaling(case):
    """objective scaling ON (both branches of the factor in every batch: scaling_helper.check_both_branches), scale_out compared"""
    if case not in _scaling_inputs:
        _scaling_inputs[case] = (SH.fast_inputs if case[0] == "fast" else SH.generic_inputs)(*case[1:])
    par, d, sig = _scaling_inputs[case]

    def solve(rev=False):
        dd = {k: _flip(v) for k, v in d.items()} if rev else d
        r = SH.solve(par, dd, SH.G_IPOPT, fast=case[0] == "fast", max_iter=CP.MAX_ITER)
        assert ((r["scale"] < 1).sum() >= 2 and (r["scale"] == 1).any())
        return r
    return C.CDLL(SH.build()), solve, CP.OUT_KEYS + ("scale",)


def _gcont(name):
    """the CONT = true instantiation of the generic kernel, uninterrupted; the save areas are not written (and must stay as they are)"""
    c = GH.case(name)

    def solve(rev=False):
        cc = dict(c, d={k: _flip(v) for k, v in c["d"].items()}, x_guess=_flip(c["x_guess"]), tick=_flip(c["tick"])) if rev else c
        r = GH.HostRun(cc)
        r.launch(1, 0, 0)
        out = r.snapshot()
        out["areas"] = r.state.copy()
        return out
    return C.CDLL(GH.build()), solve, GH.OUT_KEYS + ("scale", "areas")


SOLVER_CASES = ([("specialised", n) for n in CP.CASES] + [("generic", n) for n in CP.CASES] + [("extra", n) for n in _EXTRA] +
                [("scaling", c) for c in SCALING_CASES] + [("generic-cont", n) for n in GH.CASES])
_BUILDERS = {"specialised": _pool_specialised, "generic": _pool_generic, "extra": _extra, "scaling": _scaling, "generic-cont": _gcont}
_nan_ref = {}


def _solver(case):
    """(library, solve, keys, the NaN-slab result in the case's own order) - the reference is computed once and never changed"""
    lib, solve, keys = _BUILDERS[case[0]](case[1])
    if case not in _nan_ref:
        with PH.poisoned(lib):
            _nan_ref[case] = solve()
        assert len(_nan_ref[case]["iters"]) >= 2 and (_nan_ref[case]["iters"] > 0).all()      # every row has a predecessor or a successor, and runs
    return lib, solve, keys, _nan_ref[case]


def _case_id(case):
    return "%s-%s" % (case[0], case[1] if isinstance(case[1], str) else "-".join(str(v) for v in case[1]))


@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("case", SOLVER_CASES, ids=_case_id)
def test_uninterrupted_solve_does_not_see_what_it_starts_on(case, variant):
    mode, lane, rev = variant
    lib, solve, keys, ref = _solver(case)
    with PH.poisoned(lib, mode, lane):
        out = solve(rev)
    if rev:
        out = {k: np.asarray(out[k])[::-1] for k in keys}
    _bitwise(out, ref, keys, "%s, %s" % (_case_id(case), VARIANT_IDS[VARIANTS.index(variant)]))


def test_the_setting_reaches_the_solve():
    """the harness itself: with the blocks under the test's control a solve can be told what its slab held (the sanitized builds
    rely on the same blocks) - `keep` hands instance b + 1 the very block of instance b, and the default is back afterwards"""
    lib = PH._lib(emu_helper.build())
    a = np.zeros(64)
    for mode, check in (("noise", lambda v: (np.abs(v) <= 1e3).all() and len(set(v.tolist())) == 64), ("+1e300", lambda v: (v == 1e300).all()),
                        ("-1e300", lambda v: (v == -1e300).all()), ("+inf", lambda v: (v == np.inf).all()), ("-inf", lambda v: (v == -np.inf).all()),
                        ("0", lambda v: (v == 0).all() and not np.signbit(v).any()), ("1e-310", lambda v: (v == 1e-310).all() and (v > 0).all()),
                        ("nan", lambda v: np.isnan(v).all()), ("keep", lambda v: np.isnan(v).all())):
        with PH.poisoned(lib, mode):
            assert check(PH.fill(lib, a.copy())), mode
    with PH.poisoned(lib, "noise", seed=5):
        n1 = PH.fill(lib, a.copy())
    with PH.poisoned(lib, "noise", seed=5):
        n2 = PH.fill(lib, a.copy())
    with PH.poisoned(lib, "noise", seed=6):
        n3 = PH.fill(lib, a.copy())
    assert n1.tobytes() == n2.tobytes() != n3.tobytes()
    assert np.isnan(PH.fill(lib, a.copy())).all()      # outside `poisoned`: the default
    assert lib.mmpc_emu_poison_set(len(PH.MODES), 0, -1) != 0 and lib.mmpc_emu_poison_set(0, 0, 256) != 0


# ---- budget-1 chains: a resume rebuilds every live register from the save area and the launch arguments --------------------------
def _suspended(scal):
    return np.isfinite(scal[:, :, 4])      # (scalar 4: the iteration count of the cut - NaN where the row was not suspended)


def _assert_areas(areas, ref_areas, susp, what):
    """the save areas after every launch, on the rows suspended then, word for word - but for the words the park code never writes
    (NaN in the reference chain, whose areas start as NaN; here they start as noise)"""
    assert len(areas) == len(ref_areas)
    for l, (a, r) in enumerate(zip(areas, ref_areas)):
        written = ~np.isnan(r[susp[l]])
        assert written.any() and a[susp[l]][written].tobytes() == r[susp[l]][written].tobytes(), "%s: the save areas after launch %d differ" % (what, l)


@pytest.mark.parametrize("lane", CHAIN_LANES, ids=lambda p: "lane-%02X" % p)
@pytest.mark.parametrize("name", CP.CASES)
def test_specialised_chain_of_one_iteration_launches(name, lane):
    ref = CP.uninterrupted(name)
    _, scal, launches, ref_areas = CP.chain(name)
    c = CP.case(name)
    lib = _pool_lib(c)
    with PH.poisoned(lib, "noise", lane):
        r = CP.HostRun(c)
        PH.fill(lib, r.state)
        s2, l2, areas = emu_helper.trace_chain(r.launch, r.out["status"], r.state, r.scal_offset, budget=1)
    assert l2 == launches and s2.tobytes() == scal.tobytes()
    CP.assert_bitwise(r.out, ref, what="%s, noise + lane %02X, cut at every iteration" % (name, lane))
    _assert_areas(areas, ref_areas, _suspended(scal), name)


@pytest.mark.parametrize("lane", CHAIN_LANES, ids=lambda p: "lane-%02X" % p)
@pytest.mark.parametrize("name", GH.CASES)
def test_generic_chain_of_one_iteration_launches(name, lane):
    ref = GH.uninterrupted(name)
    _, scal, launches, ref_areas, _ = GH.chain(name)
    c = GH.case(name)
    lib = C.CDLL(GH.build())
    susp = _suspended(scal)
    with PH.poisoned(lib, "noise", lane):
        r = GH.HostRun(c)
        PH.fill(lib, r.state)
        areas = []
        for l in range(launches):
            r.launch(1, 1, int(l > 0))
            assert np.array_equal(r.out["status"] == 3, susp[l] if l < len(susp) else np.zeros(c["B"], bool)), (name, l)
            if l < launches - 1:
                areas.append(r.state.copy())
    GH.assert_bitwise(r.snapshot(), ref, keys=GH.OUT_KEYS + ("scale",), what="%s, noise + lane %02X, cut at every iteration" % (name, lane))
    _assert_areas(areas, ref_areas, susp, name)


# ---- the fleet kernels: one slab per robot -------------------------------------------------------------------------------------------
def _xlim(N):
    return np.asarray(nlp.WholeBodyParams(N=N).xlim, float)


def _tick():
    d = TH.fleet_inputs()
    return TH.build(), lambda: TH.prepare(30, 8, 0.1, _xlim(30), **d)


def _mission():
    d, _ = MIH.branch_inputs(512, 20, 3, 31)
    return MIH.build(), lambda: MIH.prepare(20, 3, 0.1, _xlim(20), **d)


def _manipulate():
    d, _ = MAH.branch_inputs(448, 20, 3, 21)
    return MAH.build(), lambda: MAH.prepare(20, 3, 0.1, _xlim(20), **d)


_FLEET = {"tick": _tick, "mission": _mission, "manipulate": _manipulate}
_fleet = {}


@pytest.mark.parametrize("mode", PH.MODES[1:])
@pytest.mark.parametrize("kernel", list(_FLEET))
def test_fleet_kernels_do_not_see_what_they_start_on(kernel, mode):
    """the seeded inputs of tests/test_fleet_{tick,mission,manipulate}_cpu.py: every array the harness returns"""
    if kernel not in _fleet:
        lib, run = _FLEET[kernel]()
        with PH.poisoned(lib):
            _fleet[kernel] = (lib, run, run())
    lib, run, ref = _fleet[kernel]
    with PH.poisoned(lib, mode):
        out = run()
    assert sorted(out) == sorted(ref) and len(ref) >= 6
    _bitwise(out, ref, sorted(ref), "fleet %s kernel, %s" % (kernel, mode))
