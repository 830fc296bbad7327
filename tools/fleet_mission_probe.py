"""Wall time of a fleet mission (B = 8192, N = 20, M = 3, seeded goals 2.9-3.4 m away: tests/mission_emu_helper.py:mission_fleet)
with DeviceFleet.run_mission on one stream and on three, against the same mission driven from the host; the cost of the list
argument of the generic wrappers against the parent commit; writes profiles/fleet_mission.txt.

  python tools/fleet_mission_probe.py [--parent DIR] [--stats CSV] [--ticks T] [--out FILE]
      three rounds alternating the variants, host clock around a run that ends in a synchronise, best and spread of each; per tick
      an event on the stream gives the time line, reported by the fleet's phase mix.
      host baseline (a tool, not product): the mission kernel, then the phases are read back and the robots of each phase are
      compacted into a whole-batch mmpc_solve_batch_device call on that phase's handle, results scattered back.
      --parent DIR: a checkout of the parent commit with its library built: the C4 batch (B = 8192, N = 20, M = 5) on the generic
      kernel (MMPC_FORCE_GENERIC) of both libraries in the same rounds.  Condition: outputs bit for bit equal and this build's best
      time within the parent's best plus the parent's own round-to-round spread.
      --stats CSV: the kernel_stats.csv of a separate `rocprofv3 --kernel-trace --stats --output-format csv ... -- python tools/fleet_mission_probe.py
      --trace-run`: time of mmpc_mission_kernel against mmpc_tick_kernel in the same run.
"""
import argparse
import csv
import importlib.util
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mmpc_loader  # noqa: E402
from oracle import nlp, synth  # noqa: E402
import mission_emu_helper as H  # noqa: E402

N, M, B, ROUNDS = 20, 3, 8192, 3


def load_parent(path):
    pkg = os.path.join(path, "mobile-manipulator-mpc_amd")
    spec = importlib.util.spec_from_file_location("mmpc_parent", os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["mmpc_parent"] = mod
    spec.loader.exec_module(mod)
    return mod


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def host_mission(fleet, T):
    """the mission with the phases read back once per tick: three compacted whole-batch solves, scattered into the output set"""
    engs = fleet._mission_handles()
    F, sets = fleet._min, fleet._msets
    x = fleet.x0.clone()
    tick = torch.zeros(fleet.B, dtype=torch.int64, device=fleet.dev)
    phase, lists, counts = F["phase"].zero_(), F["lists"], F["counts"]
    its = torch.zeros((fleet.B, T), dtype=torch.int32, device=fleet.dev); phs = torch.zeros((fleet.B, T), dtype=torch.int32, device=fleet.dev)
    ok = True
    prev = None
    for t in range(T):
        out = sets[t & 1]
        engs[0].mission_prepare(x, tick, phase, lists, counts, U_prev=prev, glob=fleet.glob, x_in=F["x_in"], traj_ref=F["loc"], obs0=fleet.obs0,
                                vel=fleet.vel, obs=F["obs"])
        ul = prev if prev is not None else F["zero"]
        ph = phase.cpu()                                            # the one synchronisation per tick
        for p, e in enumerate(engs):
            idx = torch.nonzero(ph == p).flatten().to(fleet.dev)
            if idx.numel() == 0:
                continue
            o = e.solve_batch_device(F["x_in"][idx], F["loc"][idx], fleet.uref[idx], ul[idx], F["obs"][idx])
            out["U"][idx] = o["U"]; out["iters"][idx] = o["iters"]
            its[idx, t] = o["iters"]
            ok = ok and bool((o["status"] == 0).all())
        phs[:, t] = phase
        prev = out["U"]
    engs[0].mission_prepare(x, tick, phase, lists, counts, U_prev=prev, glob=fleet.glob)
    return dict(iters=its, phase=phs, x=x, all_converged=ok)


def read_stats(path):
    rows = list(csv.DictReader(open(path)))
    pick = lambda name: [r for r in rows if name in r["Name"]]
    out = {}
    for name in ("mmpc_mission_kernel", "mmpc_tick_kernel"):
        r = pick(name)
        out[name] = (float(r[0]["AverageNs"]) / 1e3, int(r[0]["Calls"])) if r else (float("nan"), 0)
    return out


def generic_ab(mm, parent, lines):
    d = synth.make_batch(B, N=20, M=5, config_id=4)
    par = nlp.WholeBodyParams(N=20)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    xi, tr, ur, ob = t(np.clip(d["x_init"], par.xlim[0], par.xlim[1])), t(d["traj_ref"]), t(d["u_ref"]), t(d["obs"])
    ul = torch.zeros((B, 20, 5), dtype=torch.float64, device=dev)
    os.environ["MMPC_FORCE_GENERIC"] = "1"
    try:
        engs = {k: pkg.MPCWholeBody(pkg.MobileManipulator(0.1), [], [], N=20, max_batch=B, n_obstacles=5)._engine for k, pkg in (("parent", parent), ("this", mm))}
    finally:
        del os.environ["MMPC_FORCE_GENERIC"]
    assert not engs["this"].runs_specialised
    outs, times = {}, {k: [] for k in engs}
    for k, e in engs.items():
        outs[k] = e.solve_batch_device(xi, tr, ur, ul, ob)
    for _ in range(ROUNDS):
        for k, e in engs.items():
            ms, _ = timed(lambda: e.solve_batch_device(xi, tr, ur, ul, ob, out=outs[k]))
            times[k].append(ms)
    same = all(bool(torch.equal(outs["this"][k], outs["parent"][k])) for k in ("X", "U", "s", "status", "iters", "cost", "err"))
    p, m = times["parent"], times["this"]
    ok = same and min(m) <= min(p) + (max(p) - min(p))
    lines.append("generic wrappers with the list argument against the parent's, C4 batch (B = %d, N = 20, M = 5) under MMPC_FORCE_GENERIC, %d rounds:" % (B, ROUNDS))
    for k in ("parent", "this"):
        lines.append("  %-8s best %8.2f ms  spread %6.2f ms  (%s)" % (k, min(times[k]), max(times[k]) - min(times[k]), " ".join("%.2f" % v for v in times[k])))
    lines.append("  outputs bit for bit equal: %s; this build's best within the parent's best + its own spread: %s" % (same, "met" if ok else "MISSED"))
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent"); ap.add_argument("--stats"); ap.add_argument("--ticks", type=int, default=160)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fleet_mission.txt"))
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--commit", help="label of the code measured, for the report (default: git rev-parse HEAD)")
    args = ap.parse_args()
    T = args.ticks
    mm = mmpc_loader.load()
    F = H.mission_fleet(mm, B, N, 0.1)
    fleet = mm.DeviceFleet(mm, F["x0"], F["glob"], F["obs0"], F["vel"], N=N)
    if args.trace_run:
        fused = mm.DeviceFleet(mm, F["x0"], F["glob"], F["obs0"], F["vel"], N=N, fused=True)
        fleet.run_mission(20); fused.run_lockstep(20)
        torch.cuda.synchronize()
        return 0
    stamps = {}

    def mission(streams):
        ev = []

        def on_tick(t, s):
            e = torch.cuda.Event(enable_timing=True); e.record(); ev.append(e)
        e0 = torch.cuda.Event(enable_timing=True); e0.record()
        r = fleet.run_mission(T, streams=streams, on_tick=on_tick)
        stamps[streams] = [e0] + ev
        return r

    variants = {"run_mission, 1 stream": lambda: mission(1), "run_mission, 3 streams": lambda: mission(3), "host-driven baseline": lambda: host_mission(fleet, T)}
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
    r1 = last["run_mission, 1 stream"]
    solves = int((r1["phase"] < 3).sum())
    lines = ["fleet mission probe: B = %d, N = %d, M = %d, T = %d ticks; %s; taken on top of commit %s" % (B, N, M, T, torch.cuda.get_device_name(0), commit),
             "robots finished after T ticks: %d of %d; solves in a run: %d; every solve converged: %s" % (
                 int((r1["final_phase"] == 3).sum()), B, solves, bool(r1["all_converged"])),
             "wall time of one run (host clock, ends in a synchronise), %d rounds alternating the variants:" % ROUNDS]
    for k, v in times.items():
        lines.append("  %-24s best %9.2f ms  spread %7.2f ms  (%s)  %7.3f ms per tick  %8.0f solves/s" % (
            k, min(v), max(v) - min(v), " ".join("%.2f" % t for t in v), min(v) / T, solves / (min(v) * 1e-3)))
    h = last["host-driven baseline"]
    lines.append("host-driven baseline against run_mission: phases equal %s, iteration counts equal %s, x bitwise equal %s" % (
        bool(torch.equal(h["phase"], r1["phase"])), bool(torch.equal(h["iters"], r1["iters"])), bool(torch.equal(h["x"], r1["x"]))))
    r3 = last["run_mission, 3 streams"]
    lines.append("3 streams against 1: u0, iters, phase, x bitwise equal %s" % all(bool(torch.equal(r1[k], r3[k])) for k in ("u0", "iters", "phase", "x")))
    lines.append("time line of the last round by phase mix (mean robots in move / approach / rotate / done, ms per tick between stream events):")
    cnt = r1["counts"].double().cpu().numpy()
    per = {s: np.array([a.elapsed_time(b) for a, b in zip(stamps[s][:-1], stamps[s][1:])]) for s in (1, 3)}
    step = max(1, T // 8)
    for lo in range(0, T, step):
        hi = min(T, lo + step)
        c = cnt[lo:hi].mean(axis=0)
        lines.append("  ticks %3d..%3d  %6.0f %6.0f %6.0f %6.0f   1 stream %7.3f   3 streams %7.3f" % (
            lo, hi - 1, c[0], c[1], c[2], c[3], per[1][lo:hi].mean(), per[3][lo:hi].mean()))
    rc = 0
    if args.parent:
        rc = 0 if generic_ab(mm, load_parent(args.parent), lines) else 1
    if args.stats:
        s = read_stats(args.stats)
        lines.append("kernel trace of a separate run (20 mission ticks, 20 fused lock-step ticks of the same fleet): mmpc_mission_kernel %.1f us on average over %d "
                     "calls, mmpc_tick_kernel %.1f us over %d calls" % (s["mmpc_mission_kernel"] + s["mmpc_tick_kernel"]))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, "w").write(text)
    return rc


if __name__ == "__main__":
    sys.exit(main())
