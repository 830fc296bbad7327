"""Wall time of a fleet mission under iteration budgets (DeviceFleet.run_mission(budget=..., sets=...)) against the lock step, on the
fleet of tools/fleet_mission_probe.py (B = 8192, N = 20, M = 3, tests/mission_emu_helper.py:mission_fleet), with and without the
manipulate phase; writes profiles/fleet_mission_async.txt.

  python tools/fleet_mission_async_probe.py [--parent DIR] [--ticks T] [--robots B] [--rounds R] [--budgets 32,48,96] [--sets 2,3,4]
                                            [--phases both|mission|manipulate] [--resume-budget 256,512,1024] [--out FILE]
      R rounds alternating the variants in rotating order, host clock around a run that ends in a synchronise, best and spread of each:
        1. run_mission on a default fleet, parent commit (--parent DIR: a checkout of the parent commit with its library built);
        2. the same on this build.  Condition: outputs bit for bit equal and this build's best within the parent's best plus this
           build's own spread;
        3. a generic_budget=True fleet, budget 0: the comparator of every run under a budget;
        4. that fleet with every budget x every number of handle sets: wall time, rounds, suspensions, outputs against variant 3,
           and the time line of the last round by the round's lists (stream events through on_round);
        5. --resume-budget: every budget x sets again with each resume budget c (run_mission(..., resume_budget=c): a continuation gives
           a solve at most c further iterations and parks it again), with the count of re-suspensions; same comparison, same time line.
           (profiles/fleet_mission_resuspend.txt: --budgets 96 --sets 3,4 --resume-budget 256,512,1024 --phases manipulate)
"""
import argparse
import importlib.util
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, M = 20, 3
KEYS = ("u0", "iters", "status", "phase", "counts", "x", "final_phase")
KEYS_MAN = KEYS + ("mcounts", "qgoal", "ik_status", "plan")


def load_parent(path):
    pkg = os.path.join(path, "mobile-manipulator-mpc_amd")
    spec = importlib.util.spec_from_file_location("mmpc_parent", os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["mmpc_parent"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent"); ap.add_argument("--ticks", type=int, default=240); ap.add_argument("--robots", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=3); ap.add_argument("--budgets", default="32,48,96"); ap.add_argument("--sets", default="2,3,4")
    ap.add_argument("--phases", default="both", choices=("both", "mission", "manipulate"))
    ap.add_argument("--resume-budget", default="", help="resume budgets of variant 5 (default: none)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fleet_mission_async.txt"))
    ap.add_argument("--commit", help="label of the code measured, for the report (default: git rev-parse HEAD)")
    args = ap.parse_args()
    import torch
    import mmpc_loader
    import mission_emu_helper as H
    T, B = args.ticks, args.robots
    budgets, setss = [int(v) for v in args.budgets.split(",") if v], [int(v) for v in args.sets.split(",") if v]
    resumes = [int(v) for v in args.resume_budget.split(",") if v]
    mm = mmpc_loader.load()
    F = H.mission_fleet(mm, B, N, 0.1)
    mk = lambda pkg, **kw: pkg.DeviceFleet(pkg, F["x0"], F["glob"], F["obs0"], F["vel"], N=N, **kw)
    default, generic = mk(mm), mk(mm, generic_budget=True)
    pfleet = mk(load_parent(args.parent)) if args.parent else None
    try:
        commit = args.commit or subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL, text=True).strip()
    except Exception:
        commit = "working tree (no git metadata)"
    lines = ["fleet mission under iteration budgets: B = %d, N = %d, M = %d, T = %d ticks; %s; taken on top of commit %s; %d round(s) alternating the variants, "
             "host clock around a run that ends in a synchronise" % (B, N, M, T, torch.cuda.get_device_name(0), commit, args.rounds)]
    rc = 0
    for manip in ([False, True] if args.phases == "both" else [args.phases == "manipulate"]):
        kw = dict(manipulate=dict(pose=F["pose"], t_manipulate=2.0)) if manip else {}
        keys = KEYS_MAN if manip else KEYS
        stamps = {}

        def under_budget(b, k, c=0):
            ev = []

            def on_round(r, s):
                e = torch.cuda.Event(enable_timing=True); e.record()
                ev.append((e, s["counts"].clone(), s["mcounts"].clone() if manip else None, s["counters"].clone()))
            e0 = torch.cuda.Event(enable_timing=True); e0.record()
            res = generic.run_mission(T, budget=b, sets=k, on_round=on_round, **(dict(resume_budget=c) if c else {}), **kw)
            stamps[(b, k, c)] = (e0, ev)
            return res

        variants = {}
        if pfleet is not None:
            variants["1 default fleet, parent commit"] = lambda: pfleet.run_mission(T, **kw)
        variants["2 default fleet, this build"] = lambda: default.run_mission(T, **kw)
        variants["3 generic_budget fleet, budget 0"] = lambda: generic.run_mission(T, **kw)
        for b in budgets:
            for k in setss:
                variants["4 budget %3d, sets %d" % (b, k)] = (lambda b=b, k=k: under_budget(b, k))
        for b in budgets:
            for k in setss:
                for c in resumes:
                    variants["5 budget %3d, sets %d, resume %4d" % (b, k, c)] = (lambda b=b, k=k, c=c: under_budget(b, k, c))
        times = {k: [] for k in variants}; last = {}
        full = T
        T = min(full, 4)                             # warm-up: handles, buffers, save areas, code objects - a few ticks are enough
        for name, fn in variants.items():
            fn(); torch.cuda.synchronize()
            print("warm-up done: %s" % name, flush=True)
        T = full
        names = list(variants)
        for i in range(args.rounds):                 # (the order rotates: a variant's place in the round is not its property)
            for name in names[i % len(names):] + names[:i % len(names)]:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                last[name] = variants[name]()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3)
                print("%s: %.2f ms" % (name, times[name][-1]), flush=True)
        ref = last["3 generic_budget fleet, budget 0"]
        ph = ref["phase"]
        solved = (ph < 3) | (ph == 4)
        nsolve = int(solved.sum())
        lines += ["", "== %s the manipulate phase: %d solves in a run, iterations mean %.1f, max %d; solves over 32 / 48 / 96 iterations: %d / %d / %d; "
                  "every solve converged: %s" % ("with" if manip else "without", nsolve, float(ref["iters"][solved].double().mean()), int(ref["iters"].max()),
                                                 int((ref["iters"] > 32).sum()), int((ref["iters"] > 48).sum()), int((ref["iters"] > 96).sum()),
                                                 bool(ref["all_converged"]))]
        for name, v in times.items():
            r = last[name]
            extra = ""
            if name.startswith(("4", "5")):
                same = all(bool(torch.equal(r[k], ref[k])) for k in keys)
                extra = "  rounds %4d  suspended %7d%s  outputs bitwise those of variant 3: %s" % (
                    r["rounds"], r["suspended"], "  again %7d" % r["resuspended"] if name.startswith("5") else "", same)
                rc |= 0 if same else 1
            lines.append("  %-38s best %9.2f ms  spread %8.2f ms  (%s)  %8.0f solves/s%s" % (
                name, min(v), max(v) - min(v), " ".join("%.2f" % t for t in v), nsolve / (min(v) * 1e-3), extra))
        if pfleet is not None:
            rp, r2 = last["1 default fleet, parent commit"], last["2 default fleet, this build"]
            same = all(bool(torch.equal(r2[k], rp[k])) for k in keys)
            p, m = times["1 default fleet, parent commit"], times["2 default fleet, this build"]
            ok = same and min(m) <= min(p) + (max(m) - min(m))
            lines.append("  run_mission on a default fleet, this build against the parent commit: %s bit for bit equal: %s; this build's best within the "
                         "parent's best + this build's own spread: %s" % (", ".join(keys), same, "met" if ok else "MISSED"))
            rc |= 0 if ok else 1
        lines.append("  time line of the last round of each run under a budget (per block of rounds: mean robots listed in move / approach / rotate"
                     "%s, mean suspended per round, mean live after the round, ms per round between stream events):" % (" / manipulate" if manip else ""))
        for (b, k, c), (e0, ev) in stamps.items():
            per = np.array([a.elapsed_time(c) for a, c in zip([e0] + [e[0] for e in ev[:-1]], [e[0] for e in ev])])
            cnt = torch.stack([e[1] for e in ev]).double().cpu().numpy()[:, :3]
            if manip:
                cnt = np.concatenate([cnt, torch.stack([e[2] for e in ev]).double().cpu().numpy()[:, :1]], axis=1)
            ctr = torch.stack([e[3] for e in ev]).double().cpu().numpy()
            R = len(ev)
            step = max(1, (R + 11) // 12)
            lines.append("    budget %d, sets %d%s: %d rounds" % (b, k, ", resume budget %d" % c if c else "", R))
            for lo in range(0, R, step):
                hi = min(R, lo + step)
                lines.append("      rounds %3d..%3d  %s  suspended %7.1f  live %6.0f  %8.3f ms" % (
                    lo, hi - 1, " ".join("%6.0f" % c for c in cnt[lo:hi].mean(axis=0)), ctr[lo:hi, 1].mean(), ctr[lo:hi, 3].mean(), per[lo:hi].mean()))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, "w").write(text)
    return rc


if __name__ == "__main__":
    sys.exit(main())
