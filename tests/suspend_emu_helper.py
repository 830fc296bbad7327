"""ctypes driver for the host build of the bookkeeping of re-suspendable continuations (tests/suspend_emu/mmpc_suspend_emu.cpp: the
per-entry logic of a handle's list of suspended instances, csrc/mmpc_suspend.h, and the rejoin of a mission round, csrc/mmpc_round.h),
with the numpy definitions the CPU and the GPU tests share.  TEST ONLY: never used by the product package."""
import ctypes as C
import os
import subprocess

import numpy as np

import round_emu_helper as R
import tick_emu_helper as TH

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "suspend_emu", "mmpc_suspend_emu.cpp")
_CSRC = os.path.join(_HERE, "..", "mobile-manipulator-mpc_amd", "csrc")
_DEPS = [_SRC, os.path.join(_HERE, "emu_common", "mmpc_emu_poison.h"), os.path.join(_HERE, "..", "include", "mmpc.h")] + \
        [os.path.join(_CSRC, f) for f in ("mmpc_suspend.h", "mmpc_round.h", "mmpc_mission.h", "mmpc_manipulate.h", "mmpc_ik.h", "mmpc_tick.h",
                                          "mmpc_core.h", "mmpc_tile.h")]

_p = TH._p
_ip = lambda a: _p(a, C.c_int)


def build():
    out = os.path.join(_HERE, "suspend_emu", "_build", "libmmpc_suspend_emu.so")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in _DEPS):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        tmp = out + ".tmp.%d" % os.getpid()
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", tmp, _SRC])
        os.replace(tmp, out)
    return out


def _i32(a):
    return np.ascontiguousarray(a, np.int32)


def collect(status, reverse=False):
    """mmpc_collect_suspended on the host: the list (B,) - entries beyond the count at the sentinel -7 - and the count"""
    lib = C.CDLL(build())
    status = _i32(status)
    B = len(status)
    lst, cnt = np.full(B, -7, np.int32), np.full(1, -7, np.int32)
    assert lib.mmpc_suspend_emu_collect(B, _ip(status), _ip(lst), _ip(cnt), int(reverse)) == 0
    return lst, int(cnt[0])


def collect_listed(status, in_list, reverse=False):
    """mmpc_collect_suspended_list on the host (duplicates of the caller's list are entered as often as they are named, as ever)"""
    lib = C.CDLL(build())
    status, in_list = _i32(status), _i32(in_list)
    B = len(status)
    lst, cnt = np.full(max(B, len(in_list), 1), -7, np.int32), np.full(1, -7, np.int32)
    assert lib.mmpc_suspend_emu_collect_listed(B, _ip(in_list), len(in_list), _ip(status), _ip(lst), _ip(cnt), int(reverse)) == 0
    return lst, int(cnt[0])


def compact(status, S, reverse=False):
    """the compaction after a continuation under a resume budget: the entries of S whose status is still 3"""
    lib = C.CDLL(build())
    status, S = _i32(status), _i32(S)
    B = len(status)
    lst, cnt = np.full(B, -7, np.int32), np.full(1, -7, np.int32)
    assert lib.mmpc_suspend_emu_compact(B, _ip(S), len(S), _ip(status), _ip(lst), _ip(cnt), None, 0, int(reverse)) == 0
    return lst, int(cnt[0])


def merge(status, S, listed, stamp, gen, reverse=False):
    """the merge of a budgeted list launch under a resume budget (S None: nothing carried - the append alone).  `stamp` (B,) int32 is
    the handle's duplicate guard and is updated in place; gen the merge's number."""
    lib = C.CDLL(build())
    status, listed = _i32(status), _i32(listed)
    B = len(status)
    assert stamp.dtype == np.int32 and stamp.shape == (B,) and stamp.flags.c_contiguous
    lst, cnt = np.full(B, -7, np.int32), np.zeros(1, np.int32)
    if S is not None:
        S = _i32(S)
        assert lib.mmpc_suspend_emu_compact(B, _ip(S), len(S), _ip(status), _ip(lst), _ip(cnt), _ip(stamp), int(gen), int(reverse)) == 0
    assert lib.mmpc_suspend_emu_append(B, _ip(listed), len(listed), _ip(status), _ip(lst), _ip(cnt), _ip(stamp), int(gen), int(reverse)) == 0
    return lst, int(cnt[0])


def merge_reference(status, S, listed):
    """S := {b in S : status[b] == 3} united with {b listed : status[b] == 3}, indices outside the batch skipped - as a set"""
    B = len(status)
    ok = lambda b: 0 <= b < B and status[b] == 3
    return {int(b) for b in (() if S is None else S) if ok(b)} | {int(b) for b in listed if ok(b)}


def rejoin(N, s, set, reverse=False):
    """The rejoin kernel on the host, on the state dict `s` of round_emu_helper.commit_inputs; nothing of `s` is modified: the
    arrays the kernel may write (round_emu_helper.COMMIT_STATE) come back as copies, with "counters" (4,)."""
    lib = C.CDLL(build())
    r = {k: np.array(s[k], order="C") for k in R.COMMIT_STATE}
    B, T = r["hold"].shape[0], r["u0"].shape[1]
    counters = np.full(4, -7, np.int32)
    rc = lib.mmpc_suspend_emu_rejoin(C.c_int(N), C.c_int(B), _ip(r["hold"]), _ip(r["solve_phase"]), C.c_int(set), _p(s["U"]), _ip(s["status"]),
                                     _ip(s["iters"]), _p(s["tick"], C.c_longlong), _ip(s["phase"]), _p(r["U_last"]), _p(r["u0"]),
                                     _ip(r["iters_hist"]), _ip(r["status_hist"]), _ip(r["phase_hist"]), C.c_int(T), _ip(counters),
                                     C.c_int(int(reverse)))
    assert rc == 0
    r["counters"] = counters
    return r


def rejoin_reference(s, set):
    """mmpc_mission_rejoin_device in numpy (include/mmpc.h), robot by robot"""
    r = {k: np.array(s[k]) for k in R.COMMIT_STATE}
    B, T = r["hold"].shape[0], r["u0"].shape[1]
    cnt = np.zeros(4, np.int32)
    for b in range(B):
        if int(s["hold"][b]) == R.SUSPENDED + set:
            st = int(s["status"][b])
            if st == 3:
                cnt[1] += 1                   # stays suspended: nothing of it is written
            else:
                r["U_last"][b] = s["U"][b]
                t = int(s["tick"][b])
                if 0 <= t < T:
                    r["u0"][b, t] = s["U"][b, 0]
                    r["iters_hist"][b, t], r["status_hist"][b, t], r["phase_hist"][b, t] = s["iters"][b], st, s["phase"][b]
                r["hold"][b] = R.READY
                r["solve_phase"][b] = -1
                cnt[0] += 1
                cnt[2] += st != 0
        h = int(r["hold"][b])
        cnt[3] += h in (R.NEW, R.LISTED) or h >= R.SUSPENDED or (h == R.READY and int(s["phase"][b]) in (0, 1, 2, 4))
    r["counters"] = cnt
    return r


def rejoin_inputs(B=512, N=20, T=7, seed=23):
    """round_emu_helper.commit_inputs with the mixed hold codes of round_emu_helper.MIXED cycled over the robots (status and tick
    cycle at other periods, so every code meets every status inside and outside the history) and solve_phase at a value per robot:
    a robot that stays suspended keeps it"""
    s = R.commit_inputs(B, N, T, seed)
    s["hold"] = np.array(R.MIXED, np.int32)[np.arange(B) % len(R.MIXED)]
    s["status"] = ((np.arange(B) // len(R.MIXED)) % 4).astype(np.int32)
    s["tick"] = ((np.arange(B) // (4 * len(R.MIXED))) % (T + 2)).astype(np.int64)
    s["solve_phase"] = (100 + np.arange(B)).astype(np.int32)
    return s
