"""The objective scaling (mmpc_set_objective_scaling: IPOPT's nlp_scaling_method = gradient-based) on record.

  python tools/objective_scaling_probe.py --fixtures
      no GPU: the class of each of the 67 second-source fixtures (tests/golden/slsqp_solutions.npz; same minimum / other /
      costlier, the rules of tests/test_slsqp_golden.py) on the host emulation of the kernels, scaling off or on x mu_0 = 1 or 0.1.
      A record, not an assertion.
  python tools/objective_scaling_probe.py --gpu [--parent DIR]
      on the GPU, alternating rounds (at least three, host clock to a synchronise): C4 batches (whole-body N = 20, M = 5,
      B = 8192, seeds 3..12, one solve per launch, a-priori launch order): iteration counts and ms per launch, scaling on against
      off; and the same launch with the option off on this build against the parent commit's (--parent DIR: a checkout of it
      with its library built).  Gate (exit status 1): off not slower than the parent by more than the spread of the parent's
      rounds.
  python tools/objective_scaling_probe.py --meta BEFORE AFTER
      no GPU: two outputs of tools/kernel_meta.sh (parent commit, this commit) side by side ->
      profiles/objective_scaling_kernel_meta.txt; exit status 1 if a whole-body specialised kernel of one launch has scratch,
      a kernel's LDS changed or the list of kernels changed.
Each mode rewrites its own section of profiles/objective_scaling.txt and keeps the others.
"""
import argparse
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
OUT = os.path.join(ROOT, "profiles", "objective_scaling.txt")
G = 100.0
N, M, B, SEEDS, ROUNDS = 20, 5, 8192, tuple(range(3, 13)), 3


def write_section(tag, lines):
    parts = {}
    if os.path.exists(OUT):
        cur = None
        for ln in open(OUT).read().splitlines():
            m = re.match(r"## (\w+)", ln)
            if m:
                cur = m.group(1); parts[cur] = []
            elif cur:
                parts[cur].append(ln)
    parts[tag] = list(lines)
    with open(OUT, "w") as f:
        for k in ("fixtures", "gpu"):
            if k in parts:
                f.write("## %s\n%s\n" % (k, "\n".join(parts[k]).rstrip("\n") + "\n"))


# ---- 1: fixture classes on the host emulation
def fixtures(args):
    import numpy as np
    import scaling_helper as sh
    import test_slsqp_golden as tg
    from oracle import nlp
    cases = tg.load_cases()
    table, iters = {}, {}
    variants = [(0.0, 1.0), (G, 1.0), (0.0, 0.1), (G, 0.1)]
    for name, par, g in cases:
        hs = g["hs"] if len(g["hs"]) else None
        obs = g["obs"]
        d = dict(x_init=g["x_init"][None], traj_ref=g["traj_ref"][None], u_ref=g["u_ref"][None], u_last=g["u_last"][None], obs=obs[None])
        Mx = obs.shape[-2]
        diag = all(np.count_nonzero(w - np.diag(np.diag(w))) == 0 for w in (par.Q, par.P, par.R, par.W))
        fast = (sh.kind_id(par), par.N, Mx) in sh.FAST and hs is None and not par.terminal_xy_equality and diag
        runs = [(float(g["cost"]), float(g["cert_E0"])), (float(g["cost2"]), float(g["cert_E02"]) + (float(g["dX2"]) if int(g["same_min2"]) else 0.0))]
        best = min([c for c, e in runs if e <= 1e-3] or [c for c, e in runs])
        for v in variants:
            r = sh.solve(par, d, v[0], fast=fast, max_iter=2000, mu_init=v[1], hs=hs)
            cost = float(r["cost"][0])
            same = any(abs(cost - c) <= tg.TOL_COST * abs(c) for c, _ in runs)
            cls = "FAILED" if r["status"][0] != 0 else ("same" if same else "other") + ("+costlier" if cost > best * (1 + tg.TOL_COST) else "")
            table[(name, v)] = cls; iters[(name, v)] = int(r["iters"][0])
            if v == (G, 1.0):
                table[(name, "sigma")] = float(r["scale"][0])
    hdr = ["off mu0=1", "on mu0=1", "off mu0=0.1", "on mu0=0.1"]
    lines = ["fixture classes on the host emulation of the kernels (67 second-source fixtures, rules of tests/test_slsqp_golden.py: 'same' = cost",
             "equal to one of the two SLSQP runs to 1e-6, 'other' = another local minimum, '+costlier' = costs more than the best SLSQP run);",
             "objective scaling off / on (max_gradient 100) x initial barrier parameter 1 / 0.1; iteration count in brackets", "",
             "%-10s %-8s " % ("fixture", "sigma") + " ".join("%-22s" % h for h in hdr)]
    for name, _, _ in cases:
        lines.append("%-10s %-8.4f " % (name, table[(name, "sigma")]) + " ".join("%-22s" % ("%s (%d)" % (table[(name, v)], iters[(name, v)])) for v in variants))
    lines.append("")
    for h, v in zip(hdr, variants):
        cl = [table[(n, v)] for n, _, _ in cases]
        lines.append("%-12s same %2d  other %2d  costlier %2d  failed %d  mean iterations %.2f  scaled fixtures (sigma < 1) %d" % (
            h, sum(c.startswith("same") for c in cl), sum(c.startswith("other") for c in cl), sum("costlier" in c for c in cl),
            sum(c == "FAILED" for c in cl), np.mean([iters[(n, v)] for n, _, _ in cases]), sum(table[(n, "sigma")] < 1 for n, _, _ in cases)))
    for a, b in ((variants[0], variants[1]), (variants[2], variants[3])):
        moved = ["%s: %s -> %s" % (n, table[(n, a)], table[(n, b)]) for n, _, _ in cases if table[(n, a)] != table[(n, b)]]
        lines.append("scaling on against off at mu0 = %g: class changes: %s" % (a[1], "; ".join(moved) or "none"))
    print("\n".join(lines))
    write_section("fixtures", lines)
    return 0


# ---- 2, 3: the C4 batch on the GPU
def gpu(args):
    import numpy as np
    import torch
    import mmpc_loader
    from oracle import nlp, synth
    mm = mmpc_loader.load()
    pkgs = {"this": mm}
    if args.parent:
        from tools.fleet_tick_probe import load_parent
        pkgs["parent"] = load_parent(args.parent)
    dev = torch.device("cuda", 0)
    par = nlp.WholeBodyParams(N=N)
    t_ = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    eng = {k: p._capi.Engine(0, N, M, par.dt, par.ulim, par.xlim, par.dulim, max_batch=B, max_iter=2000) for k, p in pkgs.items()}
    eng["this, on"] = mm._capi.Engine(0, N, M, par.dt, par.ulim, par.xlim, par.dulim, max_batch=B, max_iter=2000)
    scale = torch.zeros(B, dtype=torch.float64, device=dev)
    eng["this, on"].set_objective_scaling(G, scale)
    for e in eng.values():
        e.set_schedule_hint(2)               # the a-priori launch order: no memory of the launch before (what bench.py times)
    order = [k for k in ("parent", "this", "this, on") if k in eng]
    names = {"parent": "parent commit", "this": "this commit, off", "this, on": "this commit, on"}
    ul = t_(np.zeros((B, N, 5)))
    lines = ["C4 batches on %s: whole-body N = %d, M = %d, B = %d, one solve per launch, cold start, schedule hint 2; wall time (host clock," % (torch.cuda.get_device_name(0), N, M, B),
             "ends in a synchronise), %d rounds per seed alternating the variants after one warm-up launch each; best of the rounds" % ROUNDS, "",
             "seed  " + "  ".join("%-44s" % names[k] for k in order)]
    tot = {k: [] for k in order}; spreads = {k: [] for k in order}; stats = {k: [] for k in order}
    off_bits = True
    for seed in SEEDS:
        d = synth.make_batch(B, N=N, M=M, config_id=seed)
        x, tr, ur, ob = t_(np.clip(d["x_init"], par.xlim[0], par.xlim[1])), t_(d["traj_ref"]), t_(d["u_ref"]), t_(d["obs"])
        outs = {k: eng[k].solve_batch_device(x, tr, ur, ul, ob) for k in order}      # warm-up
        torch.cuda.synchronize()
        times = {k: [] for k in order}
        for _ in range(ROUNDS):
            for k in order:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng[k].solve_batch_device(x, tr, ur, ul, ob, out=outs[k])
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) * 1e3)
        row = []
        for k in order:
            it = outs[k]["iters"].cpu().numpy(); st = outs[k]["status"].cpu().numpy()
            tot[k].append(min(times[k])); spreads[k].append(max(times[k]) - min(times[k])); stats[k].append((it.mean(), it.max(), (st == 0).mean()))
            row.append("%-44s" % ("%.3f ms (+%.3f) it mean %.2f max %3d conv %.5f" % (min(times[k]), max(times[k]) - min(times[k]), it.mean(), it.max(), (st == 0).mean())))
        if "parent" in eng:
            off_bits &= all(bool(torch.equal(outs["this"][q], outs["parent"][q])) for q in ("X", "U", "s", "status", "iters", "cost", "err"))
        sg = scale.cpu().numpy()
        lines.append("%4d  %s  scaled %.1f %% min sigma %.3f" % (seed, "  ".join(row), 100 * (sg < 1).mean(), sg.min()))
    lines.append("")
    for k in order:
        s = np.array(stats[k])
        lines.append("%-18s mean of the seeds' best %.3f ms per launch (%.0f solves/s); mean spread of a seed's rounds %.3f ms; iterations mean %.2f, slowest %d; converged %.5f" % (
            names[k], np.mean(tot[k]), B / (np.mean(tot[k]) * 1e-3), np.mean(spreads[k]), s[:, 0].mean(), int(s[:, 1].max()), s[:, 2].mean()))
    rc = 0
    if "parent" in eng:
        a, p, sp = np.mean(tot["this"]), np.mean(tot["parent"]), np.mean(spreads["parent"])
        ok = a <= p + sp
        lines.append("off path against the parent commit: outputs bitwise equal on every seed: %s; %.3f ms against %.3f ms + the parent's round-to-round spread %.3f ms: %s" % (
            off_bits, a, p, sp, "met" if ok else "MISSED"))
        rc = 0 if ok and off_bits else 1
    print("\n".join(lines))
    write_section("gpu", lines)
    return rc


# ---- 4: kernel metadata before / after
def meta(args):
    rd = lambda p: {ln.split()[0]: ln.split(None, 1)[1].strip() for ln in open(p).read().splitlines() if ln.strip()}
    a, b = rd(args.meta[0]), rd(args.meta[1])
    num = lambda s, key: int(re.search(key + r"\s+(\d+)", s).group(1))
    out = ["registers, spills, scratch and LDS of every kernel of libmmpc.so on the parent commit (first line) and with the objective scaling (second line);",
           "hipcc --offload-arch=gfx950 -O3 -mllvm -amdgpu-mfma-vgpr-form, from the code object's notes (tools/kernel_meta.sh)", ""]
    ok = sorted(a) == sorted(b)
    out.append("kernels: %d before, %d after; the same list: %s" % (len(a), len(b), ok))
    for k in a:
        if k not in b:
            continue
        out += [k, "    " + a[k], "    " + b[k] + ("" if a[k] != b[k] else "   (unchanged)")]
        if num(a[k], "lds") != num(b[k], "lds"):
            ok = False; out.append("    LDS CHANGED")
        if re.match(r"_Z16mmpc_fast_kernelILi0E", k) and num(b[k], "scratch") > num(a[k], "scratch"):
            ok = False; out.append("    MORE SCRATCH")
        if re.match(r"_Z16mmpc_fast_kernelILi0ELi\d+ELi\dELi1ELb0E", k) and num(b[k], "scratch") != 0:
            ok = False; out.append("    SCRATCH IN A WHOLE-BODY SPECIALISED KERNEL")
    out += ["", "LDS of every kernel unchanged, no whole-body specialised kernel gained scratch, those of one launch have none: %s" % ok]
    open(os.path.join(ROOT, "profiles", "objective_scaling_kernel_meta.txt"), "w").write("\n".join(out) + "\n")
    print("\n".join(out[-3:]))
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fixtures", action="store_true"); ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--parent"); ap.add_argument("--meta", nargs=2, metavar=("BEFORE", "AFTER"))
    args = ap.parse_args()
    if args.meta:
        return meta(args)
    if args.fixtures:
        return fixtures(args)
    if args.gpu:
        return gpu(args)
    ap.error("one of --fixtures, --gpu, --meta")


if __name__ == "__main__":
    sys.exit(main())
