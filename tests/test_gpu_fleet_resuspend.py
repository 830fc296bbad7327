"""GPU (MI355X): DeviceFleet.run_mission(budget=b, sets=k, resume_budget=c) - missions whose continuations are suspended again -
against the same fleet's lock step.

The governing claim is the one of tests/test_gpu_fleet_round.py: robots do not interact and a solve is the same bits wherever it is
cut, so every number a robot produces is bit for bit the lock step's.  b is that file's budget minus 3 and c = 1: the longest solve of
every phase then comes back still suspended at least three times.  The counts are exact: `suspended` is the number of solves with
I > b iterations, `resuspended` the sum over them of ceil((I - b) / c) - 1."""
import time

import numpy as np
import pytest

import mission_emu_helper as MH
import test_gpu_fleet_round as FR

pytestmark = pytest.mark.gpu
N, DT = FR.N, FR.DT
T_MISSION, T_MANIP = FR.T_MISSION, FR.T_MANIP
_np, _same = FR._np, FR._same


@pytest.fixture(scope="module")
def mission(mm):
    import torch
    F = MH.mission_fleet(mm, 16, N, DT)
    fleet = FR._fleet(mm, F, 16)
    lock = _np(fleet.run_mission(T_MISSION))
    torch.cuda.synchronize()
    return dict(F=F, fleet=fleet, lock=lock, budget=max(FR._budget(lock, False) - 3, 1))


@pytest.fixture(scope="module")
def manipulate(mm):
    import torch
    F = MH.mission_fleet(mm, 16, N, DT)
    fleet = FR._fleet(mm, F, 8)
    man = dict(pose=F["pose"][:8], t_manipulate=2)
    lock = _np(fleet.run_mission(T_MANIP, manipulate=man))
    torch.cuda.synchronize()
    return dict(F=F, fleet=fleet, man=man, lock=lock, budget=max(FR._budget(lock, True) - 3, 1))


def _again(lock, b, c):
    it = lock["iters"][FR._solved(lock)].astype(np.int64)
    return int((-(-(it[it > b] - b) // c) - 1).sum())


def _check(a, lock, b, c, keys, what, seconds):
    solved = FR._solved(lock)
    print("%s: budget %d, resume budget %d, %d rounds, %d of %d solves suspended, %d times again, %.1f s" % (
        what, b, c, a["rounds"], a["suspended"], solved.sum(), a["resuspended"], seconds))
    _same(a, lock, keys, what)
    assert bool(a["all_converged"]) == bool(lock["all_converged"])
    assert a["suspended"] == (lock["iters"][solved] > b).sum()
    assert a["resuspended"] == _again(lock, b, c) and a["resuspended"] > 0
    # by construction: the longest solve of every phase comes back still suspended at least three times
    for p in np.unique(lock["phase"][solved]):
        assert -(-(int(lock["iters"][lock["phase"] == p].max()) - b) // c) - 1 >= 3, p


def _run(fleet, T, **kw):
    import torch
    t0 = time.perf_counter()
    a = _np(fleet.run_mission(T, **kw))
    torch.cuda.synchronize()
    return a, time.perf_counter() - t0


@pytest.mark.parametrize("sets", [2, 3])
def test_mission_with_a_resume_budget_is_the_lock_step_per_robot(mm, mission, sets):
    lock, b = mission["lock"], mission["budget"]
    assert (lock["final_phase"] == 3).all() and bool(lock["all_converged"])
    a, dt = _run(mission["fleet"], T_MISSION, budget=b, sets=sets, resume_budget=1)
    _check(a, lock, b, 1, FR.KEYS_E2E, "mission, sets %d" % sets, dt)


@pytest.mark.parametrize("sets", [2, 3])
def test_manipulate_mission_with_a_resume_budget_is_the_lock_step_per_robot(mm, manipulate, sets):
    lock, b = manipulate["lock"], manipulate["budget"]
    assert (lock["final_phase"] == 5).all() and (lock["ik_status"] == 0).all()
    a, dt = _run(manipulate["fleet"], T_MANIP, manipulate=manipulate["man"], budget=b, sets=sets, resume_budget=1)
    _check(a, lock, b, 1, FR.KEYS_MAN, "manipulate, sets %d" % sets, dt)


def test_shifted_warm_start_with_a_resume_budget(mm, manipulate):
    """a solve launched cold in round 0 is carried past the round that sets mu_0 = 0.1 on its handle: its barrier parameter and its
    point are the save area's"""
    fleet, man = manipulate["fleet"], manipulate["man"]
    lock, _ = _run(fleet, T_MANIP, manipulate=man, warm_start="shifted")
    assert not np.array_equal(lock["iters"], manipulate["lock"]["iters"])
    b = max(FR._budget(lock, True) - 3, 1)
    a, dt = _run(fleet, T_MANIP, manipulate=man, warm_start="shifted", budget=b, sets=2, resume_budget=1)
    _check(a, lock, b, 1, FR.KEYS_MAN, "shifted", dt)
    # the handles are back at the reference protocol, without a resume budget
    again, _ = _run(fleet, T_MANIP, manipulate=man, budget=manipulate["budget"] + 3, sets=2)
    _same(again, manipulate["lock"], FR.KEYS_MAN, "after shifted")
    assert again["resuspended"] == 0


def test_motion_mode_with_a_resume_budget(mm, mission):
    lock, b = mission["lock"], mission["budget"]
    a, dt = _run(FR._fleet(mm, mission["F"], 16, obstacles="motion"), T_MISSION, budget=b, sets=2, resume_budget=1)
    _check(a, lock, b, 1, FR.KEYS_E2E, "motion", dt)


def test_resume_budget_0_is_the_call_without_it(mm, mission):
    lock, b = mission["lock"], mission["budget"] + 3
    plain, _ = _run(mission["fleet"], T_MISSION, budget=b, sets=2)
    zero, _ = _run(mission["fleet"], T_MISSION, budget=b, sets=2, resume_budget=0)
    _same(zero, plain, FR.KEYS_E2E + ("rounds", "suspended", "resuspended"), "resume_budget=0")
    _same(zero, lock, FR.KEYS_E2E, "resume_budget=0 against the lock step")
    assert zero["resuspended"] == 0 and zero["suspended"] > 0


def test_argument_errors(mm, mission):
    fleet = mission["fleet"]
    with pytest.raises(ValueError, match="resume_budget"):
        fleet.run_mission(2, resume_budget=4)
    with pytest.raises(ValueError, match="resume_budget"):
        fleet.run_mission(2, budget=10, resume_budget=-1)
