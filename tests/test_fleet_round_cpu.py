"""CPU: the glue of a mission under iteration budgets (csrc/mmpc_round.h) built for the host (g++ -DMMPC_EMU -ffp-contract=off,
tests/round_emu): the mission and manipulate kernels per robot under a hold word against the existing host builds of the batch
kernels, the commit kernel against a numpy definition, the protocol of DeviceFleet.run_mission(budget=...) end to end on the CPU
oracle, and the resource usage of the three kernels' gfx950 code objects.

Bounds.  The round kernels call mmpc_mission_one / mmpc_manipulate_one unchanged and the commit kernel copies, so everything is
compared bitwise.  The protocol test rests on the claim the driver rests on: robots do not interact, so a robot's sequence of solves
is the lock step's whatever the budget and the number of handle sets."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import coracle, nlp

import manipulate_emu_helper as MANH
import mission_emu_helper as MH
import round_emu_helper as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, M, DT, NGLOB, NPLAN = 20, 3, 0.1, 31, 21
KEYS = ("x_in", "traj_ref", "start", "obs")
FAR = 10 ** 9


def _xlim():
    return np.asarray(nlp.WholeBodyParams(N=N).xlim, float)


# ---- the references, computed once: the existing host builds on the shared inputs, without and with the advance ----------------
@functools.lru_cache(maxsize=None)
def _mission():
    d, branch = MH.branch_inputs(512, N, M, NGLOB)
    xlim = _xlim()
    return d, branch, MH.prepare(N, M, DT, xlim, **dict(d, U_prev=None)), MH.prepare(N, M, DT, xlim, **d)


@functools.lru_cache(maxsize=None)
def _manipulate():
    d, branch = MANH.branch_inputs(448, N, M, NPLAN)
    xlim = _xlim()
    return d, branch, MANH.prepare(N, M, DT, xlim, **dict(d, U_prev=None)), MANH.prepare(N, M, DT, xlim, **d)


def _mission_round(d, hold, tick_limit, **kw):
    return R.mission_round(N, M, DT, _xlim(), d["x"], d["tick"], d["phase"], d["U_prev"], hold, tick_limit, d["glob"], d["obs0"], d["vel"], **kw)


def _manipulate_round(d, hold, tick_limit, **kw):
    return R.manipulate_round(N, M, DT, _xlim(), d["x"], d["tick"], d["phase"], d["pose"], d["nplan"], d["U_prev"], hold, tick_limit,
                              plan=d["plan"], obs0=d["obs0"], vel=d["vel"], **kw)


def _listed(r):
    """the rows in the lists of a call, per solve phase, and the sentinel beyond the counts"""
    if "lists" in r:
        rows = {}
        for p in range(3):
            n = int(r["counts"][p])
            assert (r["lists"][p, n:] == -7).all(), p
            rows[p] = np.sort(r["lists"][p, :n])
        return rows
    n = int(r["counts"][0])
    assert (r["list"][n:] == -7).all()
    return {4: np.sort(r["list"][:n])}


def _check_hold(r, hold_in, sp_in=-1):
    """LISTED exactly on the listed rows, with the list's phase as solve_phase; everything else as it came in"""
    B = r["hold"].shape[0]
    exp_h, exp_s = np.array(hold_in, np.int32), np.full(B, sp_in, np.int32) if np.isscalar(sp_in) else np.array(sp_in, np.int32)
    for p, rows in _listed(r).items():
        exp_h[rows], exp_s[rows] = R.LISTED, p
    assert np.array_equal(r["hold"], exp_h) and np.array_equal(r["solve_phase"], exp_s)


STATE = {"mission": ("x", "tick", "phase"), "manipulate": ("x", "tick", "phase", "plan", "qgoal", "ik_status")}


@pytest.mark.parametrize("kind", ["mission", "manipulate"])
@pytest.mark.parametrize("hold", [R.NEW, R.READY], ids=["all_new", "all_ready"])
def test_round_kernel_is_the_batch_kernel_on_new_and_ready_robots(mm, kind, hold):
    d, _, ref_new, ref_adv = _mission() if kind == "mission" else _manipulate()
    ref = ref_new if hold == R.NEW else ref_adv
    B = d["x"].shape[0]
    for reverse in (False, True):
        r = (_mission_round if kind == "mission" else _manipulate_round)(d, np.full(B, hold, np.int32), FAR, reverse=reverse)
        for k in KEYS + STATE[kind] + ("counts",):
            assert np.array_equal(r[k], ref[k]), k
        got, want = _listed(r), _listed(ref)
        assert all(np.array_equal(got[p], want[p]) for p in want) and sum(len(v) for v in want.values()) >= 100
        _check_hold(r, np.full(B, hold, np.int32))
    assert not np.array_equal(ref_new["x"], ref_adv["x"])            # (the two references differ: the advance is tested)


@pytest.mark.parametrize("kind", ["mission", "manipulate"])
def test_mixed_holds_skip_and_process_per_robot(mm, kind):
    d, _, ref_new, ref_adv = _mission() if kind == "mission" else _manipulate()
    B = d["x"].shape[0]
    hold = np.array(R.MIXED, np.int32)[np.arange(B) % len(R.MIXED)]
    sp_in = (100 + np.arange(B)).astype(np.int32)
    new, ready = hold == R.NEW, hold == R.READY
    skip = ~(new | ready)
    assert all((hold == R.SUSPENDED + s).sum() >= 30 for s in range(4)) and new.sum() >= 60 and ready.sum() >= 120
    for reverse in (False, True):
        r = (_mission_round if kind == "mission" else _manipulate_round)(d, hold, FAR, solve_phase=sp_in, reverse=reverse)
        # a skipped robot: every row as found
        for k in KEYS:
            assert (r[k][skip] == -7).all(), k
        for k in STATE[kind]:
            found = d[k] if k in d and d[k] is not None else np.full_like(r[k], -7)
            assert np.array_equal(r[k][skip], found[skip]), k
        assert np.array_equal(r["hold"][skip], hold[skip]) and np.array_equal(r["solve_phase"][skip], sp_in[skip])
        # a processed robot: its rows of the all-NEW / all-READY call
        for k in KEYS + STATE[kind]:
            assert np.array_equal(r[k][new], ref_new[k][new]) and np.array_equal(r[k][ready], ref_adv[k][ready]), k
        after = np.where(new, ref_new["phase"], ref_adv["phase"])
        got = _listed(r)
        if kind == "mission":
            for p in range(3):
                assert np.array_equal(got[p], np.flatnonzero(~skip & (after == p))), p
            assert r["counts"][3] == (~skip & (after >= 3)).sum()
        else:
            assert np.array_equal(got[4], np.flatnonzero(~skip & (after == 4)))
            assert r["counts"][1] == (~skip & (after == 5)).sum()
        _check_hold(r, hold, sp_in)


def test_mission_round_retires_at_the_tick_limit(mm):
    d, branch, _, _ = _mission()
    B = d["x"].shape[0]
    xlim = _xlim()
    L = 37
    # every other cycle of the branches is at its last tick; the others have four to go
    last = (np.arange(B) // len(MH.BRANCHES)) % 2 == 0
    d = dict(d, tick=np.where(last, L - 1, L - 5).astype(np.int64))
    bare = MH.prepare(N, M, DT, xlim, **d, want=())                  # the output-less call at the end of run_mission
    full = MH.prepare(N, M, DT, xlim, **d)
    frozen = d["phase"] >= 3
    retire = last & ~frozen
    assert all((retire & (branch == k)).sum() >= 8 for k in range(len(MH.BRANCHES)) if MH.BRANCHES[k] != "done")
    assert (frozen & last).sum() >= 8
    for reverse in (False, True):
        r = _mission_round(d, np.full(B, R.READY, np.int32), L, reverse=reverse)
        for k in ("x", "tick", "phase"):
            assert np.array_equal(r[k][retire], bare[k][retire]) and np.array_equal(r[k][~retire], full[k][~retire]), k
        assert np.array_equal(r["tick"][retire], np.full(int(retire.sum()), L)) and not np.array_equal(r["x"][retire], d["x"][retire])
        for k in KEYS:
            assert (r[k][retire] == -7).all() and np.array_equal(r[k][~retire], full[k][~retire]), k
        got = _listed(r)
        for p in range(3):
            assert np.array_equal(got[p], np.flatnonzero(~last & (full["phase"] == p))), p
        assert r["counts"][3] == (~retire & (full["phase"] >= 3)).sum()
        exp = np.full(B, R.READY, np.int32)
        exp[retire] = np.where(bare["phase"][retire] == 3, R.RETIRED_AT_DONE, R.RETIRED)
        exp[~last & (full["phase"] < 3)] = R.LISTED
        assert np.array_equal(r["hold"], exp)
        assert (exp == R.RETIRED_AT_DONE).sum() >= 24 and (r["solve_phase"][retire] == -1).all()


def test_manipulate_round_retires_at_the_tick_limit(mm):
    d, branch, _, _ = _manipulate()
    B = d["x"].shape[0]
    xlim = _xlim()
    L = 37
    last = (np.arange(B) // len(MANH.BRANCHES)) % 2 == 0
    d = dict(d, tick=np.where(last, L - 1, L - 5).astype(np.int64))
    bare = MANH.prepare(N, M, DT, xlim, **d, want=())
    full = MANH.prepare(N, M, DT, xlim, **d)
    retire = last & (d["phase"] == MANH.MANIPULATE)       # (a robot at 'move finish' was advanced by the mission round: it is solved)
    assert (retire & (bare["phase"] == 4)).sum() >= 8 and (retire & (bare["phase"] == 5)).sum() >= 8
    for reverse in (False, True):
        r = _manipulate_round(d, np.full(B, R.READY, np.int32), L, reverse=reverse)
        for k in STATE["manipulate"]:
            assert np.array_equal(r[k][retire], bare[k][retire]) and np.array_equal(r[k][~retire], full[k][~retire]), k
        assert np.array_equal(r["tick"][retire], np.full(int(retire.sum()), L))
        for k in KEYS:
            assert (r[k][retire] == -7).all() and np.array_equal(r[k][~retire], full[k][~retire]), k
        assert np.array_equal(_listed(r)[4], np.flatnonzero(~retire & (full["phase"] == 4)))
        assert r["counts"][1] == (~retire & (full["phase"] == 5)).sum()
        exp = np.full(B, R.READY, np.int32)
        exp[retire] = R.RETIRED
        exp[~retire & (full["phase"] == 4)] = R.LISTED
        assert np.array_equal(r["hold"], exp)


def test_retiring_into_move_finish_makes_the_lock_steps_transition(mm):
    """The corner: the retiring advance of the mission round takes a robot to 'move finish'.  The lock step's two output-less calls
    leave it in 'manipulate' (or 'manipulate finish') with its IK answer and plan; so do the two round kernels."""
    d, branch, _, _ = _mission()
    B = d["x"].shape[0]
    xlim = _xlim()
    L = 12
    d = dict(d, tick=np.full(B, L - 1, np.int64))
    rng = np.random.default_rng(8)
    psi, reach = d["x"][:, 2], rng.uniform(0.3, 0.7, B)
    pose = np.stack([d["x"][:, 0] + reach * np.cos(psi), d["x"][:, 1] + reach * np.sin(psi), rng.uniform(1.0, 1.6, B), psi], axis=1)
    one = MH.prepare(N, M, DT, xlim, **d, want=())
    two = MANH.prepare(N, M, DT, xlim, one["x"], one["tick"], one["phase"], pose, NPLAN, U_prev=d["U_prev"], obs0=d["obs0"], vel=d["vel"], want=())
    corner = (d["phase"] < 3) & (one["phase"] == 3)
    assert corner.sum() >= 100 and (two["phase"][corner] >= 4).all() and (two["ik_status"][corner] >= 0).all()
    for reverse in (False, True):
        a = _mission_round(d, np.full(B, R.READY, np.int32), L, reverse=reverse)
        assert (a["hold"][corner] == R.RETIRED_AT_DONE).all() and (a["hold"][~corner & (d["phase"] < 3)] == R.RETIRED).all()
        b = R.manipulate_round(N, M, DT, xlim, a["x"], a["tick"], a["phase"], pose, NPLAN, d["U_prev"], a["hold"], L, obs0=d["obs0"], vel=d["vel"],
                               reverse=reverse)
        for k in STATE["manipulate"]:
            assert np.array_equal(b[k], two[k]), k
        assert (b["hold"][d["phase"] < 3] == R.RETIRED).all()
        for k in KEYS:
            assert (b[k][corner] == -7).all(), k
        assert not np.isin(np.flatnonzero(corner), _listed(b)[4]).any()
        # (the robots that came in at 'move finish' are READY and not at their limit by the manipulate round's rule: listed, if live)
        assert np.array_equal(_listed(b)[4], np.flatnonzero((d["phase"] == 3) & (two["phase"] == 4)))


@pytest.mark.parametrize("rejoin", [0, 1])
@pytest.mark.parametrize("set_", [1, 3])
def test_commit_kernel_against_numpy_definition(mm, set_, rejoin):
    T = 7
    s = R.commit_inputs(512, N, T)
    mine = s["hold"] == (R.SUSPENDED + set_ if rejoin else R.LISTED)
    for st in range(4):
        assert (mine & (s["status"] == st) & (s["tick"] < T)).sum() >= 4 and (mine & (s["status"] == st) & (s["tick"] >= T)).sum() >= 1, st
    ref = R.commit_reference(s, set_, rejoin)
    for reverse in (False, True):
        r = R.commit(N, s, set_, rejoin, reverse=reverse)
        for k in R.COMMIT_STATE + ("counters",):
            assert np.array_equal(r[k], ref[k]), k
    # what the definition says, in the test's own words: nobody else is written, a suspended robot keeps U_last and its histories
    for k in R.COMMIT_STATE:
        assert np.array_equal(ref[k][~mine], s[k][~mine]), k
    susp = mine & (s["status"] == 3) if not rejoin else np.zeros(512, bool)
    assert (ref["hold"][susp] == R.SUSPENDED + set_).all() and (ref["U_last"][susp] == -7).all() and (ref["u0"][susp] == -7).all()
    done = mine & ~susp
    assert (ref["hold"][done] == R.READY).all() and np.array_equal(ref["U_last"][done], s["U"][done]) and (ref["solve_phase"][mine] == -1).all()
    assert ref["counters"][0] == done.sum() and ref["counters"][1] == susp.sum() and ref["counters"][2] == (done & (s["status"] != 0)).sum()
    assert (susp.sum() > 0) == (rejoin == 0) and 0 < ref["counters"][3] < 512


# ---- the protocol end to end on the CPU oracle ----------------------------------------------------------------------------------
class _Fleet:
    """4 robots of the mission fleet, the host kernels and the CPU oracle per phase handle (the settings of tests/oracle_engine.py).
    The oracle is deterministic, so a solve is remembered by its inputs: the async runs replay the lock step's solves and pay only
    for one whose inputs differ - which then shows in the comparison."""

    def __init__(self, mm, B=4, seed=5):
        F = MH.mission_fleet(mm, 16, N, DT, seed=seed)
        self.B = B
        self.F = {k: np.ascontiguousarray(v[:B]) for k, v in F.items()}
        self.xlim = _xlim()
        self.par = []
        for p in range(4):
            par = nlp.WholeBodyParams(N=N, dt=DT)
            par.terminal_xy_equality = p >= 1
            if p >= 2:
                par.Q = par.P = np.diag([5., 5, 5, 0, 0, 1, 1, 1, 1] if p == 2 else [500., 500, 500, 0, 0, 1, 1, 1, 1])
            self.par.append(par)
        self.memo = {}
        self.zero_u = np.zeros((1, N, 5))

    def solve(self, p, x_in, traj, ul, obs):
        key = (p, x_in.tobytes(), traj.tobytes(), ul.tobytes(), obs.tobytes())
        if key not in self.memo:
            r = coracle.solve_batch(self.par[min(p, 3)], x_in[None], traj[None], self.zero_u, ul[None], obs[None], tol=1e-8, max_iter=200)
            self.memo[key] = (r["U"][0].copy(), int(r["iters"][0]), int(r["status"][0]))
        return self.memo[key]

    def lockstep(self, T, manip):
        F, B, xlim = self.F, self.B, self.xlim
        x, tick, phase = F["x0"].copy(), np.zeros(B, np.int64), np.zeros(B, np.int32)
        plan, qgoal, iks = np.zeros((B, NPLAN, 9)), np.zeros((B, 3)), np.full(B, -1, np.int32)
        U, prev = np.zeros((B, N, 5)), None
        h = dict(u0=np.zeros((B, T, 5)), iters=np.zeros((B, T), np.int32), status=np.zeros((B, T), np.int32), phase=np.zeros((B, T), np.int32))

        def glue(want):
            nonlocal x, tick, phase, plan, qgoal, iks
            a = MH.prepare(N, M, DT, xlim, x, tick, phase, prev, F["glob"], F["obs0"], F["vel"], want=want)
            x, tick, phase = a["x"], a["tick"], a["phase"]
            rows = [(p, a["lists"][p, :a["counts"][p]]) for p in range(3)]
            if manip:
                b = MANH.prepare(N, M, DT, xlim, x, tick, phase, F["pose"], NPLAN, prev, plan, F["obs0"], F["vel"], want=want)
                x, tick, phase, plan = b["x"], b["tick"], b["phase"], b["plan"]
                tr = b["ik_status"] != -7
                qgoal[tr], iks[tr] = b["qgoal"][tr], b["ik_status"][tr]
                lst = b["list"][:b["counts"][0]]
                for k in want:
                    a[k][lst] = b[k][lst]
                rows.append((4, lst))
            return a, rows

        for t in range(T):
            a, rows = glue(KEYS)
            ul = prev if prev is not None else np.zeros((B, N, 5))
            new = U.copy()
            for p, lst in rows:
                for b in lst:
                    new[b], it, st = self.solve(p, a["x_in"][b], a["traj_ref"][b], ul[b], a["obs"][b])
                    h["u0"][b, t], h["iters"][b, t], h["status"][b, t] = new[b, 0], it, st
            U = prev = new
            h["phase"][:, t] = phase
        glue(())
        h.update(x=x, final_phase=phase, plan=plan, qgoal=qgoal, ik_status=iks)
        return h

    def rounds(self, T, manip, budget, sets):
        F, B, xlim = self.F, self.B, self.xlim
        x, tick, phase = F["x0"].copy(), np.zeros(B, np.int64), np.zeros(B, np.int32)
        plan, qgoal, iks = np.zeros((B, NPLAN, 9)), np.zeros((B, 3)), np.full(B, -1, np.int32)
        buf = dict(x_in=np.zeros((B, 9)), traj_ref=np.zeros((B, N + 1, 9)), start=np.zeros(B, np.int32), obs=np.zeros((B, N + 1, M, 3)))
        s = dict(hold=np.zeros(B, np.int32), solve_phase=np.full(B, -1, np.int32), U=np.zeros((B, N, 5)), status=np.zeros(B, np.int32),
                 iters=np.zeros(B, np.int32), U_last=np.zeros((B, N, 5)), u0=np.zeros((B, T, 5)), iters_hist=np.zeros((B, T), np.int32),
                 status_hist=np.zeros((B, T), np.int32), phase_hist=np.full((B, T), -1, np.int32))
        flight = {}
        r = nsusp = 0

        def commit(k, rejoin):
            s.update(tick=tick, phase=phase)
            c = R.commit(N, s, k, rejoin)
            s.update({key: c[key] for key in R.COMMIT_STATE})
            return c["counters"]

        while True:
            k = r % sets
            if k in flight:
                for b, (Ub, it, st) in flight.pop(k):
                    s["U"][b], s["iters"][b], s["status"][b] = Ub, it, st
                commit(k, 1)
            a = R.mission_round(N, M, DT, xlim, x, tick, phase, s["U_last"], s["hold"], T, F["glob"], F["obs0"], F["vel"],
                                solve_phase=s["solve_phase"], init=buf)
            x, tick, phase = a["x"], a["tick"], a["phase"]
            rows = [(p, a["lists"][p, :a["counts"][p]]) for p in range(3)]
            if manip:
                a = R.manipulate_round(N, M, DT, xlim, x, tick, phase, F["pose"], NPLAN, s["U_last"], a["hold"], T, plan=plan, obs0=F["obs0"],
                                       vel=F["vel"], solve_phase=a["solve_phase"], qgoal=qgoal, ik_status=iks, init={k_: a[k_] for k_ in KEYS})
                x, tick, phase, plan, qgoal, iks = a["x"], a["tick"], a["phase"], a["plan"], a["qgoal"], a["ik_status"]
                rows.append((4, a["list"][:a["counts"][0]]))
            buf = {k_: a[k_] for k_ in KEYS}
            s.update(hold=a["hold"], solve_phase=a["solve_phase"])
            held = []
            for p, lst in rows:
                for b in lst:
                    assert s["hold"][b] == R.LISTED and s["solve_phase"][b] == p
                    Ub, it, st = self.solve(p, buf["x_in"][b], buf["traj_ref"][b], s["U_last"][b], buf["obs"][b])
                    if it <= budget:
                        s["U"][b], s["iters"][b], s["status"][b] = Ub, it, st
                    else:        # (what a suspended solve leaves in its rows is nobody's business)
                        s["U"][b], s["iters"][b], s["status"][b] = np.nan, budget, 3
                        held.append((b, (Ub, it, st)))
            cnt = commit(k, 0)
            assert cnt[1] == len(held)
            nsusp += len(held)
            flight[k] = held
            r += 1
            if r >= T and cnt[3] == 0:
                break
            assert r < (sets + 2) * T + 8
        ph = np.where(s["phase_hist"] < 0, phase[:, None], s["phase_hist"])
        return dict(u0=s["u0"], iters=s["iters_hist"], status=s["status_hist"], phase=ph, x=x, final_phase=phase, plan=plan, qgoal=qgoal,
                    ik_status=iks, rounds=r, suspended=nsusp, hold=s["hold"])


@functools.lru_cache(maxsize=None)
def _fleet(mm):
    return _Fleet(mm)


@pytest.mark.parametrize("manip", [False, True], ids=["mission", "manipulate"])
def test_protocol_end_to_end_on_the_cpu_oracle(mm, manip):
    fl = _fleet(mm)
    T = 220 if manip else 200
    lock = fl.lockstep(T, manip)
    solved = (lock["phase"] < 3) | (lock["phase"] == 4)
    phases = [p for p in (0, 1, 2, 4) if (lock["phase"] == p).any()]
    assert phases == ([0, 1, 2, 4] if manip else [0, 1, 2]) and (lock["final_phase"] == (5 if manip else 3)).all()
    peak = {p: int(lock["iters"][lock["phase"] == p].max()) for p in phases}
    b1 = min(peak.values()) - 1
    print("solves %d, max iterations per phase %s, budgets %d, 1, %d" % (solved.sum(), peak, b1, 10 ** 6))
    assert b1 >= lock["iters"][solved].min()
    for p in phases:
        it = lock["iters"][lock["phase"] == p]
        assert (it > b1).any() and (it <= b1).any(), (p, b1)
    keys = ("u0", "iters", "status", "phase", "x", "final_phase") + (("plan", "qgoal", "ik_status") if manip else ())
    for budget in (b1, 1, 10 ** 6):
        for sets in (2, 3):
            a = fl.rounds(T, manip, budget, sets)
            print("budget %d, sets %d: %d rounds, %d suspended" % (budget, sets, a["rounds"], a["suspended"]))
            for k in keys:
                assert np.array_equal(a[k], lock[k]), (budget, sets, k)
            assert a["suspended"] == (lock["iters"][solved] > budget).sum()
            assert np.isin(a["hold"], (R.READY, R.RETIRED)).all()
            if budget == 10 ** 6:
                assert a["rounds"] == T + 1 or (a["rounds"] == T and not solved[:, -1].any())


# ---- resources ------------------------------------------------------------------------------------------------------------------
def test_round_kernels_use_no_scratch_on_gfx950(mm):
    """The three kernels cross-compiled for gfx950, as the compiler reports them: no scratch; the round kernels' LDS is the tick
    kernel's slots and the spare counters of a retiring call."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = "hipcc"
    src = os.path.join(ROOT, "tests", "round_emu", "mmpc_round_probe.hip")
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage", src], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    lds_doubles = MH.C.CDLL(MH.build()).mmpc_mission_emu_lds_doubles()
    for name, lds in (("mmpc_mission_round_probe_kernel", 8 * lds_doubles), ("mmpc_manipulate_round_probe_kernel", 8 * lds_doubles),
                      ("mmpc_commit_probe_kernel", 0)):
        m = re.search(r"Function Name: " + name + r"(.*?)LDS Size \[bytes/block\]: (\d+)", p.stderr, re.S)
        assert m, p.stderr[-2000:]
        get = lambda key: int(re.search(re.escape(key) + r": (\d+)", m.group(1)).group(1))
        usage = "%s: VGPRs %d, SGPRs %d, occupancy %d waves/SIMD, scratch %d B/lane, LDS %s B" % (
            name, get("VGPRs"), get("SGPRs"), get("Occupancy [waves/SIMD]"), get("ScratchSize [bytes/lane]"), m.group(2))
        print(usage)
        assert get("ScratchSize [bytes/lane]") == 0, usage
        # (the four spare counters and their alignment: at most 32 bytes on top of the tick kernel's slots; the commit kernel: none)
        assert lds <= int(m.group(2)) <= (lds + 32 if lds else 0), usage
