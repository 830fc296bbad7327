"""The linear-motion obstacle mode (obs_per_stage = 2) beside the per-stage table: kernel metadata and wall times.

  python tools/obstacle_motion_probe.py --meta [--meta-input FILE] [--build-times BEFORE_S AFTER_S]
      no GPU: compiles the product kernels for gfx950 (tools/kernel_meta.sh) and writes profiles/obstacle_motion_kernel_meta.txt -
      every motion instantiation beside its table and static siblings, and the requirements on its scratch.
  python tools/obstacle_motion_probe.py [--parent DIR]
      on the GPU, protocol of tools/fleet_tick_probe.py (alternating rounds, at least three, host clock to a synchronise); writes
      profiles/obstacle_motion.txt:
        C5 lock step, fused, B = 8192, T = 10, seed 5: motion against table on this build (and the table on the parent commit:
        --parent DIR, a checkout of it with its library built);
        whole-body N = 20, M = 5, moving obstacles, B = 8192, one solve per launch: motion against table.
      Gates (exit status 1): motion not slower than table by more than the spread between the table's rounds; table not slower
      than the parent's by more than the spread of the parent's rounds.
"""
import argparse
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, M, B, T, SEED, ROUNDS = 30, 8, 8192, 10, 5, 3


def meta(args):
    if args.meta_input:                      # the output of an earlier tools/kernel_meta.sh run of the same sources
        txt = open(args.meta_input).read()
    else:
        co = os.path.join(ROOT, "profiles", "_obstacle_motion.co")
        txt = subprocess.check_output(["bash", os.path.join(ROOT, "tools", "kernel_meta.sh")], text=True, env=dict(os.environ, MMPC_META_OUT=co))
        os.remove(co)
    rows = {}
    for ln in txt.splitlines():
        m = re.match(r"_Z16mmpc_fast_kernelILi(\d)ELi(\d+)ELi(\d+)ELi\dELb(\d)ELi(\d)E\S*\s+(.*)", ln)
        if m:
            k, n, mc, cont, ops, rest = m.groups()
            rows[(int(k), int(n), int(mc), int(cont), int(ops))] = rest
        m = re.match(r"_Z17mmpc_solve_kernelILi(\d)ELi0ELin1ELi(n1|2)ELin1E\S*\s+(.*)", ln)
        if m:
            rows[("generic", int(m.group(1)), 2 if m.group(2) == "2" else -1)] = m.group(3)
    num = lambda s, key: int(re.search(key + r"\s+(\d+)", s).group(1))
    out = ["kernel metadata of the motion instantiations (OPS = 2) beside their siblings (OPS = 0 static record, 1 table per stage);",
           "hipcc --offload-arch=gfx950 -O3 -mllvm -amdgpu-mfma-vgpr-form, from the code object's notes (tools/kernel_meta.sh)", ""]
    ok = True
    for (k, n, mc) in sorted({key[:3] for key in rows if key[0] != "generic"}):
        for cont in (0, 1):
            out.append("mmpc_fast_kernel<%d,%d,%d> %s" % (k, n, mc, "budgeted / continuation" if cont else "one launch"))
            for ops in (0, 1, 2):
                out.append("    OPS %d  %s" % (ops, rows[(k, n, mc, cont, ops)]))
            s2 = num(rows[(k, n, mc, cont, 2)], "scratch")
            sib = [num(rows[(k, n, mc, cont, o)], "scratch") for o in (0, 1)]
            good = s2 <= min(sib) if k == 0 else s2 <= max(sib)
            ok &= good
            out.append("    scratch of the motion kernel %d against %d / %d of its siblings: %s" % (s2, sib[0], sib[1], "ok" if good else "MORE"))
    out.append("")
    for kind in (0, 1, 2):
        out.append("mmpc_solve_kernel<%d> (run-time-sized generic kernel)" % kind)
        out.append("    OPS 0/1 %s" % rows[("generic", kind, -1)])
        out.append("    OPS 2   %s" % rows[("generic", kind, 2)])
    out += ["", "all kernels of the library:"] + ["  " + ln for ln in txt.splitlines()]
    if args.build_times:
        out += ["", "build time of libmmpc.so (hipcc, host + device, one process): %s s before, %s s after (the specialised list grows by half: "
                    "16 -> 24 instantiations; three more of the run-time-sized generic kernel)" % tuple(args.build_times)]
    path = os.path.join(ROOT, "profiles", "obstacle_motion_kernel_meta.txt")
    open(path, "w").write("\n".join(out) + "\n")
    print("\n".join(out[:40]))
    return 0 if ok else 1


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def rounds(variants, warm=1):
    import torch
    times = {k: [] for k in variants}; last = {}
    for k, fn in variants.items():
        for _ in range(warm):
            fn(); torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for k, fn in variants.items():
            ms, last[k] = timed(fn)
            times[k].append(ms)
    return times, last


def bench(args):
    import numpy as np
    import torch
    import mmpc_loader
    from oracle import nlp, synth
    from tools.fleet_tick_probe import load_parent, make_fleet
    mm = mmpc_loader.load()
    dev = torch.device("cuda", 0)
    lines = ["obstacle motion probe; %s; wall time (host clock, ends in a synchronise), %d rounds alternating the variants" % (torch.cuda.get_device_name(0), ROUNDS)]
    rc = 0
    fmt = lambda k, v, n: "  %-30s best %8.2f ms  spread %6.2f ms  (%s)  %8.0f solves/s" % (k, min(v), max(v) - min(v), " ".join("%.2f" % t for t in v), n / (min(v) * 1e-3))

    # ---- C5 lock step, fused
    d = synth.make_batch(B, N=N, M=M, config_id=SEED, moving=True)
    variants = {}
    if args.parent:
        pf = make_fleet(load_parent(args.parent), d, fused=True)
        variants["parent, table"] = lambda: pf.run_lockstep(T)
    ft, fm = make_fleet(mm, d, fused=True), make_fleet(mm, d, fused=True, obstacles="motion")
    variants["table"] = lambda: ft.run_lockstep(T)
    variants["motion"] = lambda: fm.run_lockstep(T)
    times, last = rounds(variants)
    lines.append("C5 lock step, fused: B = %d, N = %d, M = %d, T = %d ticks, seed %d" % (B, N, M, T, SEED))
    lines += [fmt(k, v, B * T) for k, v in times.items()]
    a, b = last["table"], last["motion"]
    lines.append("  motion against table: u0, x, iters bitwise equal %s; all converged %s / %s; mean iterations %.2f; table buffer of a fleet %.1f MB, record %.2f MB" % (
        bool(torch.equal(a["u0"], b["u0"]) and torch.equal(a["x"], b["x"]) and torch.equal(a["iters"], b["iters"])), bool(a["all_converged"]),
        bool(b["all_converged"]), float(b["iters"].double().mean()), B * (N + 1) * M * 3 * 8 / 1e6, B * M * 5 * 8 / 1e6))
    tb = times["table"]; spread = max(tb) - min(tb)
    ok = min(times["motion"]) <= min(tb) + spread
    lines.append("  gate: motion %.2f ms against table %.2f ms + its spread %.2f ms: %s" % (min(times["motion"]), min(tb), spread, "met" if ok else "MISSED"))
    rc |= 0 if ok else 1
    if args.parent:
        p = times["parent, table"]; ps = max(p) - min(p)
        ok = min(tb) <= min(p) + ps
        lines.append("  gate: table %.2f ms against the parent's %.2f ms + the spread of its rounds %.2f ms: %s" % (min(tb), min(p), ps, "met" if ok else "MISSED"))
        rc |= 0 if ok else 1
    del ft, fm, variants, last
    torch.cuda.empty_cache()

    # ---- whole-body N = 20, M = 5, one solve per launch
    n, m = 20, 5
    d = synth.make_batch(B, N=n, M=m, config_id=SEED, moving=True)
    par = nlp.WholeBodyParams(N=n)
    rec = np.concatenate([d["obs"], d["obs_vel"]], axis=2)
    tick = np.zeros(B, np.int64)
    tab = np.empty((B, n + 1, m, 3))
    tk = np.arange(n + 1, dtype=np.float64) * par.dt
    tab[..., 0] = rec[:, None, :, 0] + rec[:, None, :, 3] * tk[None, :, None]
    tab[..., 1] = rec[:, None, :, 1] + rec[:, None, :, 4] * tk[None, :, None]
    tab[..., 2] = rec[:, None, :, 2]
    t_ = lambda a_: torch.from_numpy(np.ascontiguousarray(a_)).to(dev)
    x, tr, ur, ul = t_(np.clip(d["x_init"], par.xlim[0], par.xlim[1])), t_(d["traj_ref"]), t_(d["u_ref"]), t_(np.zeros((B, n, 5)))
    eng = {k: mm._capi.Engine(0, n, m, par.dt, par.ulim, par.xlim, par.dulim, max_batch=B, obs_per_stage=v, max_iter=2000) for k, v in (("table", True), ("motion", "motion"))}
    eng["motion"].set_obstacle_clock(t_(tick))
    obs = dict(table=t_(tab), motion=t_(rec))
    outs = {k: e.solve_batch_device(x, tr, ur, ul, obs[k]) for k, e in eng.items()}
    for e in eng.values():
        e.set_schedule_hint(2)               # the a-priori launch order: no memory of the launch before (what bench.py times)
    variants = {k: (lambda k=k: eng[k].solve_batch_device(x, tr, ur, ul, obs[k], out=outs[k])) for k in eng}
    times, last = rounds(variants, warm=2)
    lines.append("whole-body N = %d, M = %d, moving obstacles, B = %d, one solve per launch (schedule hint 2); problems per CU: table %d, motion %d" % (
        n, m, B, eng["table"].problems_per_cu, eng["motion"].problems_per_cu))
    lines += [fmt(k, v, B) for k, v in times.items()]
    a, b = last["table"], last["motion"]
    lines.append("  motion against table: X, U, s, status, iters, cost bitwise equal %s; converged %d / %d of %d" % (
        all(bool(torch.equal(a[k], b[k])) for k in ("X", "U", "s", "status", "iters", "cost")), int((a["status"] == 0).sum()), int((b["status"] == 0).sum()), B))
    tb = times["table"]; spread = max(tb) - min(tb)
    ok = min(times["motion"]) <= min(tb) + spread
    lines.append("  gate: motion %.2f ms against table %.2f ms + its spread %.2f ms: %s" % (min(times["motion"]), min(tb), spread, "met" if ok else "MISSED"))
    rc |= 0 if ok else 1
    text = "\n".join(lines) + "\n"
    print(text)
    open(args.out, "w").write(text)
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meta", action="store_true"); ap.add_argument("--meta-input"); ap.add_argument("--build-times", nargs=2)
    ap.add_argument("--parent"); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "obstacle_motion.txt"))
    args = ap.parse_args()
    return meta(args) if args.meta else bench(args)


if __name__ == "__main__":
    sys.exit(main())
