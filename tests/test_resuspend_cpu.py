"""CPU: re-suspendable continuations - the bookkeeping of a handle's list of suspended instances (csrc/mmpc_suspend.h) and the rejoin
of a mission round (mmpc_rejoin_robot, csrc/mmpc_round.h) on their host build against numpy definitions; chains of budgeted
continuations on the host builds of both kernel families; and the fleet protocol with a resume budget on the CPU oracle.

Everything here is exact: lists are compared as sets with exact counts, save areas word for word, results bit for bit."""
import numpy as np
import pytest

import continuation_pool as CP
import emu_helper
import generic_cont_helper as GH
import round_emu_helper as R
import suspend_emu_helper as SH
import test_fleet_round_cpu as FR

B = 512


def _statuses(seed):
    """512 rows, a third of them suspended"""
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([0, 1, 2, 3, 3], np.int32), B)


def _as_set(lst, n):
    assert 0 <= n <= B and (lst[n:] == -7).all()
    got = lst[:n].tolist()
    assert len(set(got)) == n, "a row is in the list twice"
    return set(got)


# ---- list bookkeeping -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reverse", [False, True])
def test_collect_keeps_its_behaviour(reverse):
    st = _statuses(1)
    lst, n = SH.collect(st, reverse)
    assert _as_set(lst, n) == set(np.flatnonzero(st == 3).tolist())
    rng = np.random.default_rng(2)
    named = np.concatenate([rng.permutation(B)[:200], [-1, B, B + 7, 1 << 30]]).astype(np.int32)
    rng.shuffle(named)
    lst, n = SH.collect_listed(st, named, reverse)
    assert _as_set(lst, n) == {int(b) for b in named if 0 <= b < B and st[b] == 3}
    # a row named twice is entered twice: the list launch's behaviour as it is, pinned
    lst, n = SH.collect_listed(st, np.repeat(np.flatnonzero(st == 3)[:5], 2), reverse)
    assert n == 10


@pytest.mark.parametrize("reverse", [False, True])
def test_compact_by_status(reverse):
    st0 = _statuses(3)
    S = np.random.default_rng(4).permutation(np.flatnonzero(st0 == 3)).astype(np.int32)
    assert len(S) > 100
    # a continuation ends some of them
    st = st0.copy()
    st[S[::3]] = 0
    st[S[1::7]] = 1
    lst, n = SH.compact(st, S, reverse)
    assert _as_set(lst, n) == SH.merge_reference(st, S, []) == set(S.tolist()) & set(np.flatnonzero(st == 3).tolist())
    assert 0 < n < len(S)
    # nobody left, and an empty list
    assert SH.compact(np.zeros(B, np.int32), S, reverse)[1] == 0 and SH.compact(st, [], reverse)[1] == 0
    # an entry outside the batch (the list is device memory) is dropped
    lst, n = SH.compact(st, np.concatenate([S, [-3, B]]), reverse)
    assert _as_set(lst, n) == SH.merge_reference(st, S, [])


@pytest.mark.parametrize("reverse", [False, True])
def test_merge_carries_the_suspended_and_appends_the_listed_once(reverse):
    rng = np.random.default_rng(5)
    st = _statuses(6)
    stamp = np.zeros(B, np.int32)
    gen = 0
    rows = rng.permutation(B)
    A, Bl = rows[:B // 2], rows[B // 2:]
    # launch A into an empty S: duplicates, indices outside the batch
    listA = np.concatenate([A, A[:40], [-1, B, B + 100]]).astype(np.int32)
    rng.shuffle(listA)
    gen += 1
    lst, n = SH.merge(st, None, listA, stamp, gen, reverse)
    S = lst[:n].copy()
    assert _as_set(lst, n) == SH.merge_reference(st, None, listA) and n == (st[A] == 3).sum()
    # launch B: the other half, plus rows still suspended from A (named again: they start afresh - some end, some are suspended
    # again), plus duplicates; meanwhile nothing else happened to S
    again = S[:30]
    st2 = st.copy()
    st2[again[:10]] = 0                      # the new solve of a carried row ended: it leaves S
    st2[Bl[:50]] = rng.choice(np.array([0, 3], np.int32), 50)
    listB = np.concatenate([Bl, again, Bl[:25], [B]]).astype(np.int32)
    rng.shuffle(listB)
    gen += 1
    lst, n = SH.merge(st2, S, listB, stamp, gen, reverse)
    want = SH.merge_reference(st2, S, listB)
    assert _as_set(lst, n) == want and n == len(want)
    assert set(again[10:].tolist()) <= want and not set(again[:10].tolist()) & want
    S2 = lst[:n].copy()
    # an empty list keeps S (compacted); an empty S and an empty list give nothing
    gen += 1
    st3 = st2.copy()
    st3[S2[::2]] = 0
    lst, n = SH.merge(st3, S2, [], stamp, gen, reverse)
    assert _as_set(lst, n) == SH.merge_reference(st3, S2, []) and n == len(S2) - len(S2[::2])
    gen += 1
    assert SH.merge(st3, [], [], stamp, gen, reverse)[1] == 0
    # the same list twice in a row: the stamps of the merge before do not hide anybody
    gen += 1
    lst, n = SH.merge(st, None, listA, stamp, gen, reverse)
    assert _as_set(lst, n) == SH.merge_reference(st, None, listA)


# ---- rejoin -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("set_", [1, 3])
def test_rejoin_kernel_against_numpy_definition(set_):
    N, T = 20, 7
    s = SH.rejoin_inputs(B, N, T)
    mine = s["hold"] == R.SUSPENDED + set_
    for st in range(4):
        assert (mine & (s["status"] == st) & (s["tick"] < T)).sum() >= 2 and (mine & (s["status"] == st) & (s["tick"] >= T)).sum() >= 1, st
    ref = SH.rejoin_reference(s, set_)
    for reverse in (False, True):
        r = SH.rejoin(N, s, set_, reverse=reverse)
        for k in R.COMMIT_STATE + ("counters",):
            assert np.array_equal(r[k], ref[k]), (k, reverse)
    # the definition in the test's own words: nobody else is written; status 3 stays suspended and nothing of it is written
    stay = mine & (s["status"] == 3)
    for k in R.COMMIT_STATE:
        assert np.array_equal(ref[k][~mine | stay], s[k][~mine | stay]), k
    done = mine & ~stay
    assert (ref["hold"][done] == R.READY).all() and np.array_equal(ref["U_last"][done], s["U"][done]) and (ref["solve_phase"][done] == -1).all()
    assert ref["counters"].tolist()[:3] == [done.sum(), stay.sum(), (done & (s["status"] != 0)).sum()] and stay.sum() > 0
    assert 0 < ref["counters"][3] < B
    # every other status is the commit's rejoin, exactly
    s2 = {k: v.copy() for k, v in s.items()}
    s2["status"][stay] = 1
    a, c = SH.rejoin(N, s2, set_), R.commit(N, s2, set_, 1)
    for k in R.COMMIT_STATE + ("counters",):
        assert np.array_equal(a[k], c[k]), k


# ---- chains of budgeted continuations on the host builds ------------------------------------------------------------------------
def _pairs(it_max):
    return [(1, 2), (3, 7), (max(it_max // 2, 1), 1)]


def _chain_check(name, launch, out, state, ref, areas, what):
    """launch(budget, resume) on (out, state): a budgeted launch, then budgeted continuations; after continuation n the save areas of
    the rows still suspended are those of the budget-1 chain at iteration b + n c (areas[b + n c - 1]), and the end is `ref`."""
    it = ref["iters"]
    for b, c in _pairs(int(it.max())):
        state[:] = np.nan
        launch(b, 0)
        n = 0
        while True:
            done = b + n * c
            susp = out["status"] == 3
            assert np.array_equal(susp, it > done), (what, b, c, n)
            if not susp.any():
                break
            assert (out["iters"][susp] == done).all()
            assert state[susp].tobytes() == areas[done - 1][susp].tobytes(), (what, b, c, n)
            launch(c, 1)
            n += 1
        assert n == -(-(int(it.max()) - b) // c) if it.max() > b else n == 0
        for k in CP.OUT_KEYS:
            assert out[k].tobytes() == ref[k].tobytes(), (what, b, c, k)


@pytest.mark.parametrize("name", ["0-20-5", "0-30-8", "1-15-3-motion"])
def test_specialised_chain_of_budgeted_continuations(name):
    ref = CP.uninterrupted(name)
    _, _, _, areas = CP.chain(name)
    r = CP.HostRun(CP.case(name))
    _chain_check(name, r.launch, r.out, r.state, ref, areas, name)


@pytest.mark.parametrize("name", ["wb-12-2", "wb-20-3-teq-table", "pose-10-2"])
def test_generic_chain_of_budgeted_continuations(name):
    ref = GH.uninterrupted(name)
    _, _, _, areas, _ = GH.chain(name)
    r = GH.HostRun(GH.case(name))
    # (the chain's areas hold NaN where a row was not suspended after that launch; only suspended rows are compared)
    _chain_check(name, lambda b, res: r.launch(1, b, res), r.out, r.state, ref, areas, name)


# ---- the protocol with a resume budget on the CPU oracle -------------------------------------------------------------------------
def _rounds(fl, T, manip, budget, c, sets, max_iter=200):
    """test_fleet_round_cpu._Fleet.rounds with a resume budget: the rejoin in place of the rejoining commit; a continuation adds c
    iterations to a held solve, which comes back finished or still suspended and is then carried on its set"""
    N, M, DT, NPLAN, KEYS = FR.N, FR.M, FR.DT, FR.NPLAN, FR.KEYS
    F, nB, xlim = fl.F, fl.B, fl.xlim
    x, tick, phase = F["x0"].copy(), np.zeros(nB, np.int64), np.zeros(nB, np.int32)
    plan, qgoal, iks = np.zeros((nB, NPLAN, 9)), np.zeros((nB, 3)), np.full(nB, -1, np.int32)
    buf = dict(x_in=np.zeros((nB, 9)), traj_ref=np.zeros((nB, N + 1, 9)), start=np.zeros(nB, np.int32), obs=np.zeros((nB, N + 1, M, 3)))
    s = dict(hold=np.zeros(nB, np.int32), solve_phase=np.full(nB, -1, np.int32), U=np.zeros((nB, N, 5)), status=np.zeros(nB, np.int32),
             iters=np.zeros(nB, np.int32), U_last=np.zeros((nB, N, 5)), u0=np.zeros((nB, T, 5)), iters_hist=np.zeros((nB, T), np.int32),
             status_hist=np.zeros((nB, T), np.int32), phase_hist=np.full((nB, T), -1, np.int32))
    flight = {}
    r = nsusp = nagain = 0
    cap = (sets + 2) * T + 8 + T * sets * -(-max_iter // c)
    while True:
        k = r % sets
        if k in flight:
            carried = []
            for b, (Ub, it, st), done in flight.pop(k):
                done += c                                     # the continuation queued at the end of the set's last round
                if it <= done:
                    s["U"][b], s["iters"][b], s["status"][b] = Ub, it, st
                else:
                    s["U"][b], s["iters"][b], s["status"][b] = np.nan, done, 3
                    carried.append((b, (Ub, it, st), done))
            s.update(tick=tick, phase=phase)
            rj = SH.rejoin(N, s, k, reverse=bool(r & 1))
            s.update({key: rj[key] for key in R.COMMIT_STATE})
            assert rj["counters"][1] == len(carried) and all(s["hold"][b] == R.SUSPENDED + k for b, _, _ in carried)
            nagain += len(carried)
            flight[k] = carried
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
        held = flight.get(k, [])
        new = 0
        for p, lst in rows:
            for b in lst:
                assert s["hold"][b] == R.LISTED and s["solve_phase"][b] == p and all(b != h[0] for h in held)
                Ub, it, st = fl.solve(p, buf["x_in"][b], buf["traj_ref"][b], s["U_last"][b], buf["obs"][b])
                if it <= budget:
                    s["U"][b], s["iters"][b], s["status"][b] = Ub, it, st
                else:
                    s["U"][b], s["iters"][b], s["status"][b] = np.nan, budget, 3
                    held.append((b, (Ub, it, st), budget))
                    new += 1
        s.update(tick=tick, phase=phase)
        cm = R.commit(N, s, k, 0)
        s.update({key: cm[key] for key in R.COMMIT_STATE})
        assert cm["counters"][1] == new
        nsusp += new
        flight[k] = held
        r += 1
        if r >= T and cm["counters"][3] == 0:
            break
        assert r < cap
    ph = np.where(s["phase_hist"] < 0, phase[:, None], s["phase_hist"])
    return dict(u0=s["u0"], iters=s["iters_hist"], status=s["status_hist"], phase=ph, x=x, final_phase=phase, plan=plan, qgoal=qgoal,
                ik_status=iks, rounds=r, suspended=nsusp, resuspended=nagain, hold=s["hold"])


@pytest.mark.parametrize("manip", [False, True], ids=["mission", "manipulate"])
def test_protocol_with_a_resume_budget_on_the_cpu_oracle(mm, manip):
    fl = FR._fleet(mm)
    T = 220 if manip else 200
    lock = fl.lockstep(T, manip)
    solved = (lock["phase"] < 3) | (lock["phase"] == 4)
    phases = [p for p in (0, 1, 2, 4) if (lock["phase"] == p).any()]
    b1 = min(int(lock["iters"][lock["phase"] == p].max()) for p in phases) - 1
    keys = ("u0", "iters", "status", "phase", "x", "final_phase") + (("plan", "qgoal", "ik_status") if manip else ())
    it = lock["iters"][solved].astype(np.int64)
    for budget, c in ((max(b1 - 3, 1), 1), (b1, 3), (1, 7)):
        want = int((-(-(it[it > budget] - budget) // c) - 1).sum())
        assert want > 0
        for sets in (2, 3):
            a = _rounds(fl, T, manip, budget, c, sets)
            print("budget %d, resume budget %d, sets %d: %d rounds, %d suspended, %d suspended again" % (budget, c, sets, a["rounds"], a["suspended"],
                                                                                                        a["resuspended"]))
            for k in keys:
                assert np.array_equal(a[k], lock[k]), (budget, c, sets, k)
            assert a["suspended"] == (it > budget).sum() and a["resuspended"] == want
            assert np.isin(a["hold"], (R.READY, R.RETIRED)).all()
