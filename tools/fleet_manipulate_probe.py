"""Wall time of a fleet mission to 'manipulate finish' (B = 8192, N = 20, M = 3, the fleet and the pose targets of
tests/mission_emu_helper.py:mission_fleet) with DeviceFleet.run_mission(manipulate=...), and run_mission without the manipulate phase
against the parent commit; writes profiles/fleet_manipulate.txt.  With --meta: the kernel metadata report
profiles/fleet_manipulate_kernel_meta.txt (no GPU needed).

  python tools/fleet_manipulate_probe.py [--parent DIR] [--ticks T] [--out FILE]
      three rounds alternating the variants, host clock around a run that ends in a synchronise, best and spread of each; per tick
      an event on the stream gives the time line, reported by the fleet's phase mix.
      --parent DIR: a checkout of the parent commit with its library built: run_mission(T) of both packages in the same rounds.
      Condition: outputs bit for bit equal and this build's best time within the parent's best plus the parent's own spread.
  python tools/fleet_manipulate_probe.py --meta LISTING --meta-parent LISTING [--meta-out FILE]
      LISTING: the listing of tools/kernel_meta.sh (or the same lines read from the code object inside a built libmmpc.so) for this
      tree and for the parent commit's.  Condition: every kernel of the parent is there with the same registers, spills, scratch and
      LDS, and the manipulate kernel is the one addition.
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

N, M, B, ROUNDS = 20, 3, 8192, 3


def load_parent(path):
    pkg = os.path.join(path, "mobile-manipulator-mpc_amd")
    spec = importlib.util.spec_from_file_location("mmpc_parent", os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["mmpc_parent"] = mod
    spec.loader.exec_module(mod)
    return mod


def meta_report(listing, parent, out):
    rows = lambda path: {l[:78].rstrip(): l[78:].split() for l in open(path).read().splitlines() if " vgpr " in l}
    new, old = rows(listing), rows(parent)
    lines = ["kernel metadata of libmmpc.so with the manipulate kernel (llvm-readelf --notes of the gfx950 code object of the library as",
             "build.py builds it, in the format of tools/kernel_meta.sh; names cut at 78 characters)", "",
             "the new kernel beside the two it is modelled on and the IK kernel whose solver it runs on lane 0:"]
    for name in ("mmpc_tick_kernel", "mmpc_mission_kernel", "mmpc_ik_kernel", "mmpc_manipulate_kernel"):
        lines += ["  %-78s %s" % (k, " ".join("%s %5s" % (a, b) for a, b in zip(v[::2], v[1::2]))) for k, v in new.items() if name in k]
    changed = [k for k in old if new.get(k) != old[k]]
    added = [k for k in new if k not in old]
    lines += ["", "against the parent commit, the %d kernels that existed before: %d unchanged in vgpr, agpr, vspill, sspill, scratch and lds" % (
        len(old), len(old) - len(changed))]
    lines += ["  CHANGED %s: %s -> %s" % (k, " ".join(old[k]), " ".join(new.get(k, ["missing"]))) for k in changed]
    lines += ["added: %s" % ", ".join(added), "", "all kernels:"]
    lines += ["  %-78s %s" % (k, " ".join("%s %5s" % (a, b) for a, b in zip(v[::2], v[1::2]))) for k, v in new.items()]
    text = "\n".join(lines) + "\n"
    print(text)
    open(out, "w").write(text)
    return 0 if not changed and len(added) == 1 and "mmpc_manipulate_kernel" in added[0] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent"); ap.add_argument("--ticks", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fleet_manipulate.txt"))
    ap.add_argument("--meta"); ap.add_argument("--meta-parent")
    ap.add_argument("--meta-out", default=os.path.join(ROOT, "profiles", "fleet_manipulate_kernel_meta.txt"))
    ap.add_argument("--commit", help="label of the code measured, for the report (default: git rev-parse HEAD)")
    args = ap.parse_args()
    if args.meta:
        return meta_report(args.meta, args.meta_parent, args.meta_out)
    import torch
    import mmpc_loader
    import mission_emu_helper as H
    T = args.ticks
    mm = mmpc_loader.load()
    F = H.mission_fleet(mm, B, N, 0.1)
    fleet = mm.DeviceFleet(mm, F["x0"], F["glob"], F["obs0"], F["vel"], N=N)
    man = dict(pose=F["pose"], t_manipulate=2.0)
    stamps = {}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def mission(fl, key, **kw):
        ev = []

        def on_tick(t, s):
            e = torch.cuda.Event(enable_timing=True); e.record(); ev.append(e)
        e0 = torch.cuda.Event(enable_timing=True); e0.record()
        r = fl.run_mission(T, on_tick=on_tick, **kw)
        stamps[key] = [e0] + ev
        return r

    variants = {"with manipulate": lambda: mission(fleet, "man", manipulate=man), "without, this build": lambda: mission(fleet, "this")}
    if args.parent:
        parent = load_parent(args.parent)
        pfleet = parent.DeviceFleet(parent, F["x0"], F["glob"], F["obs0"], F["vel"], N=N)
        variants["without, parent commit"] = lambda: mission(pfleet, "parent")
    times = {k: [] for k in variants}; last = {}
    for k, fn in variants.items():
        fn(); torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for k, fn in variants.items():
            ms, last[k] = timed(fn)
            times[k].append(ms)
    try:
        commit = args.commit or subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL, text=True).strip()
    except Exception:
        commit = "working tree (no git metadata)"
    rm, r0 = last["with manipulate"], last["without, this build"]
    ph = rm["phase"]
    solves = {"with manipulate": int(((ph < 3) | (ph == 4)).sum())}
    for k in variants:
        if k != "with manipulate":
            solves[k] = int((last[k]["phase"] < 3).sum())
    fin = rm["final_phase"]
    lines = ["fleet manipulate probe: B = %d, N = %d, M = %d, T = %d ticks, t_manipulate = 2 s (plans of 21 rows); %s; taken on top of commit %s" % (
                 B, N, M, T, torch.cuda.get_device_name(0), commit),
             "after T ticks: %d of %d robots at 'manipulate finish', %d in 'manipulate', %d still driving; IK solves: %d, failed: %d; solves in a run: %d, "
             "of them in 'manipulate': %d; every solve converged: %s" % (
                 int((fin == 5).sum()), B, int((fin == 4).sum()), int((fin < 3).sum()), int((rm["ik_status"] >= 0).sum()), int((rm["ik_status"] > 0).sum()),
                 solves["with manipulate"], int((ph == 4).sum()), bool(rm["all_converged"])),
             "ticks a robot spends in 'manipulate': %s" % (lambda n: "min %d, median %d, max %d" % (n.min(), np.median(n), n.max()))(
                 (ph == 4).sum(dim=1).cpu().numpy()[(fin == 5).cpu().numpy()]),
             "solves of the run with manipulate by the phase they were made in (a failed solve does not stop a robot; a tick lasts as long as its slowest solve):"]
    st, it = rm["status"], rm["iters"]
    for p, name in ((0, "move"), (1, "approach"), (2, "rotate"), (4, "manipulate")):
        sel = ph == p
        if int(sel.sum()):
            lines.append("  %-10s solves %8d  not converged %6d (status 1: %d, status 2: %d)  iterations mean %5.1f  max %4d" % (
                name, int(sel.sum()), int((st[sel] != 0).sum()), int((st[sel] == 1).sum()), int((st[sel] == 2).sum()), float(it[sel].double().mean()),
                int(it[sel].max())))
    left = (fin == 4).cpu().numpy()
    if left.any():
        import manipulate_emu_helper as MH
        xs = rm["x"].cpu().numpy()
        err = np.array([np.linalg.norm(MH.fk(mm, xs[b]) - F["pose"][b, :3]) for b in np.flatnonzero(left)])
        arm = np.abs(xs[left, 6:] - rm["qgoal"].cpu().numpy()[left]).max()
        lines.append("the %d robots still in 'manipulate': endpoint error %.1f-%.1f mm (finish at 10), arm within %.1e rad of q_goal, ticks in the phase %s" % (
            int(left.sum()), 1e3 * err.min(), 1e3 * err.max(), arm, sorted((ph == 4).sum(dim=1).cpu().numpy()[left].tolist())))
    lines.append("wall time of one run (host clock, ends in a synchronise; three streams, with manipulate four), %d rounds alternating the variants:" % ROUNDS)
    for k, v in times.items():
        lines.append("  %-24s best %9.2f ms  spread %7.2f ms  (%s)  %7.3f ms per tick  %8.0f solves/s" % (
            k, min(v), max(v) - min(v), " ".join("%.2f" % t for t in v), min(v) / T, solves[k] / (min(v) * 1e-3)))
    rc = 0
    keys = ("u0", "iters", "status", "phase", "counts", "x", "final_phase")
    if args.parent:
        rp = last["without, parent commit"]
        same = all(bool(torch.equal(r0[k], rp[k])) for k in keys)
        p, m = times["without, parent commit"], times["without, this build"]
        ok = same and min(m) <= min(p) + (max(p) - min(p))
        lines.append("run_mission without manipulate, this build against the parent commit: u0, iters, status, phase, counts, x, final_phase bit for bit "
                     "equal: %s; this build's best within the parent's best + its own spread: %s" % (same, "met" if ok else "MISSED"))
        rc = 0 if ok else 1
    # up to 'move finish' the mission with the manipulate phase is the one without
    done0 = (r0["phase"] == 3)
    before = ~(done0.cumsum(dim=1) > 0)
    lines.append("with manipulate against without, every (robot, tick) before the robot's 'move finish': u0, iters, phase bitwise equal %s" % all(
        bool(torch.equal(rm[k][before], r0[k][before])) for k in ("u0", "iters", "phase")))
    lines.append("time line of the last round by phase mix (mean robots in move / approach / rotate / manipulate / manipulate finish, ms per tick between "
                 "stream events; 'without': move / approach / rotate / move finish):")
    cnt = torch.cat([rm["counts"][:, :3], rm["mcounts"]], dim=1).double().cpu().numpy()
    cnt0 = r0["counts"].double().cpu().numpy()
    per = {s: np.array([a.elapsed_time(b) for a, b in zip(stamps[s][:-1], stamps[s][1:])]) for s in stamps}
    step = max(1, T // 12)
    for lo in range(0, T, step):
        hi = min(T, lo + step)
        c, c0 = cnt[lo:hi].mean(axis=0), cnt0[lo:hi].mean(axis=0)
        lines.append("  ticks %3d..%3d  %6.0f %6.0f %6.0f %6.0f %6.0f  %8.3f ms   | without %6.0f %6.0f %6.0f %6.0f  %8.3f ms" % (
            lo, hi - 1, c[0], c[1], c[2], c[3], c[4], per["man"][lo:hi].mean(), c0[0], c0[1], c0[2], c0[3], per["this"][lo:hi].mean()))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, "w").write(text)
    return rc


if __name__ == "__main__":
    sys.exit(main())
