"""Wall time of C5's receding-horizon loop (B = 8192, N = 30, M = 8, T = 10, seed 5) with the torch glue and with the fused tick
kernel (mmpc_tick_prepare_device), lock step and shifted warm start; writes profiles/fleet_tick.txt.

  python tools/fleet_tick_probe.py [--parent DIR] [--stats CSV] [--out FILE]
      three rounds alternating the variants, host clock around a run that ends in a synchronise, best and spread of each.
      --parent DIR: a checkout of the parent commit with its library built; its run_lockstep is loaded as a second package and
      timed in the same rounds.  Gate (exit status 1): fused lock step is not slower than the parent's lock step by more than the
      spread of the parent's own three rounds.
      --stats CSV: the kernel_stats.csv of a separate `rocprofv3 --kernel-trace --stats ... -- python tools/fleet_tick_probe.py
      --trace-run` (one warm-up and one fused lock-step run): share of GPU time in the solver, kernels per tick, tick kernel time.
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
import mmpc_loader  # noqa: E402
from oracle import nlp, synth  # noqa: E402

N, M, B, T, SEED, ROUNDS = 30, 8, 8192, 10, 5, 3


def load_parent(path):
    pkg = os.path.join(path, "mobile-manipulator-mpc_amd")
    spec = importlib.util.spec_from_file_location("mmpc_parent", os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["mmpc_parent"] = mod
    spec.loader.exec_module(mod)
    return mod


def make_fleet(pkg, d, **kw):
    dev = torch.device("cuda", 0)
    glob = torch.from_numpy(d["traj_ref"]).to(dev)
    step = (glob[:, N] - glob[:, 0]) / N
    glob = glob[:, :1] + step[:, None, :] * torch.arange(51, dtype=torch.float64, device=dev)[None, :, None]
    par = nlp.WholeBodyParams(N=N)
    return pkg.DeviceFleet(pkg, np.clip(d["x_init"], par.xlim[0], par.xlim[1]), glob, d["obs"], d["obs_vel"], N=N, **kw)


def torch_shifted_loop(fleet):
    """the shifted warm start built by torch expressions, a loop of N plant steps per tick (as tools/probe_c5.py --shifted and
    bench.py:run_all(shifted=True))"""
    eng = fleet.engs[0]
    f64 = fleet.f64
    x = fleet.x0.clone(); ul = torch.zeros((B, N, 5), **f64)
    ug = torch.zeros((B, N, 5), **f64); xg = torch.zeros((B, N + 1, 9), **f64)
    tick = torch.zeros(B, dtype=torch.int64, device=fleet.dev)
    its = []
    out = None
    eng.set_warm_start(None, 1.0); eng.reset()
    for t in range(T):
        loc, obs = fleet.inputs(x, tick)
        xgs = None
        if t >= 1:
            ug[:, :-1] = ul[:, 1:]; ug[:, -1] = ul[:, -1]
            xg[:, 0] = torch.minimum(torch.maximum(x, fleet.xlo), fleet.xhi)
            for k in range(N):
                xg[:, k + 1] = fleet.plant(xg[:, k], ug[:, k])
            if t == 1:
                eng.set_warm_start(ug, 0.1)
            xgs = xg
        out = eng.solve_batch_device(x, loc, fleet.uref, ul, obs, x_guess=xgs, out=out)
        ul = out["U"].clone()
        its.append(out["iters"].clone())
        x = fleet.plant(x, out["U"][:, 0]); tick = tick + 1
    eng.set_warm_start(None, 1.0)
    return dict(iters=torch.stack(its, dim=1), all_converged=(out["status"] == 0).all())


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def read_stats(path):
    rows = list(csv.DictReader(open(path)))
    tot = sum(float(r["TotalDurationNs"]) for r in rows)
    solver = sum(float(r["TotalDurationNs"]) for r in rows if "mmpc_fast_kernel" in r["Name"])
    tk = [r for r in rows if "mmpc_tick_kernel" in r["Name"]]
    calls = sum(int(r["Calls"]) for r in rows)
    return dict(share=solver / tot, calls=calls, tick_avg_us=float(tk[0]["AverageNs"]) / 1e3 if tk else float("nan"),
                tick_calls=int(tk[0]["Calls"]) if tk else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent"); ap.add_argument("--stats"); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fleet_tick.txt"))
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--commit", help="label of the code measured, for the report (default: git rev-parse HEAD)")
    args = ap.parse_args()
    mm = mmpc_loader.load()
    d = synth.make_batch(B, N=N, M=M, config_id=SEED, moving=True)
    if args.trace_run:
        fleet = make_fleet(mm, d, fused=True)
        for _ in range(2):
            fleet.run_lockstep(T)
            torch.cuda.synchronize()
        return 0
    variants = {}
    if args.parent:
        pf = make_fleet(load_parent(args.parent), d)
        variants["parent run_lockstep"] = pf.run_lockstep
    variants["fused=False"] = make_fleet(mm, d).run_lockstep
    variants["fused=True"] = make_fleet(mm, d, fused=True).run_lockstep
    variants["shifted, fused"] = make_fleet(mm, d, fused=True, warm_start="shifted").run_lockstep
    loop_fleet = make_fleet(mm, d)
    variants["shifted, torch loop"] = lambda T_: torch_shifted_loop(loop_fleet)
    times = {k: [] for k in variants}; last = {}
    for k, fn in variants.items():          # warm-up: code objects, allocations, every shape of the timed window
        fn(T); torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for k, fn in variants.items():
            ms, last[k] = timed(lambda: fn(T))
            times[k].append(ms)
    try:
        commit = args.commit or subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL, text=True).strip()
    except Exception:
        commit = "working tree (no git metadata)"
    lines = ["fleet tick probe: C5 fleet, B = %d, N = %d, M = %d, T = %d ticks, seed %d; %s; taken on top of commit %s" % (
        B, N, M, T, SEED, torch.cuda.get_device_name(0), commit),
        "wall time of one run of T ticks (host clock, ends in a synchronise), %d rounds alternating the variants:" % ROUNDS]
    for k, v in times.items():
        it = last[k]["iters"].double()
        lines.append("  %-22s best %8.2f ms  spread %6.2f ms  (%s)  %7.0f solves/s  mean iterations %.2f (ticks 1..: %.2f)  all converged %s" % (
            k, min(v), max(v) - min(v), " ".join("%.2f" % t for t in v), B * T / (min(v) * 1e-3), float(it.mean()), float(it[:, 1:].mean()),
            bool(last[k]["all_converged"])))
    a, f = last["fused=False"], last["fused=True"]
    du = (a["u0"] - f["u0"]).abs().amax(dim=2)
    lines.append("fused against unfused lock step: u0 bitwise equal %s (tick 0: %s), max |du0| %.3e, (robot, tick) pairs above 1e-6: %d of %d in %d robots, "
                 "above 1e-3: %d in %d robots, equal iteration counts %.4f" % (
                     bool(torch.equal(a["u0"], f["u0"])), bool(torch.equal(a["u0"][:, 0], f["u0"][:, 0])), float(du.max()), int((du > 1e-6).sum()), du.numel(),
                     int((du > 1e-6).any(dim=1).sum()), int((du > 1e-3).sum()), int((du > 1e-3).any(dim=1).sum()), float((a["iters"] == f["iters"]).double().mean())))
    s_f, s_l = last["shifted, fused"], last["shifted, torch loop"]
    lines.append("shifted: mean iterations fused %.2f, torch loop %.2f; ratio to the reference warm start %.3f" % (
        float(s_f["iters"].double().mean()), float(s_l["iters"].double().mean()),
        float(s_f["iters"][:, 1:].double().mean()) / float(f["iters"][:, 1:].double().mean())))
    rc = 0
    if args.parent:
        p = times["parent run_lockstep"]
        slack = max(p) - min(p)
        ok = min(times["fused=True"]) <= min(p) + slack
        lines.append("gate: fused lock step %.2f ms against the parent's %.2f ms + its own spread %.2f ms: %s" % (
            min(times["fused=True"]), min(p), slack, "met" if ok else "MISSED"))
        rc = 0 if ok else 1
    if args.stats:
        s = read_stats(args.stats)
        lines.append("kernel trace of a separate run (warm-up + one fused lock-step run, %d ticks in all): %.2f %% of GPU time in mmpc_fast_kernel, "
                     "%.1f kernels per tick, tick kernel %.1f us on average over %d calls" % (2 * T, 100 * s["share"], s["calls"] / (2.0 * T), s["tick_avg_us"], s["tick_calls"]))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, "w").write(text)
    return rc


if __name__ == "__main__":
    sys.exit(main())
