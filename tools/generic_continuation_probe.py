"""Measurements behind profiles/generic_continuation.txt: what iteration budgets on the generic kernel cost, and that a default handle
pays nothing for them.

  python tools/generic_continuation_probe.py [--parent DIR] [--rounds R] [--out FILE]
      the C4 batch (B = 8192, N = 20, M = 5, config 4) under MMPC_FORCE_GENERIC, all variants alternating in one process, host clock
      around a launch (or a launch and its continuation) that ends in a synchronise, best and spread of each:
        parent      --parent DIR: a checkout of the parent commit with its library built, a default handle (static-LDS generic kernel)
        this        this tree, a default handle (the same kernel); condition: outputs bit for bit the parent's, this build's best
                    within the parent's best plus the parent's own round-to-round spread
        optin       this tree, a handle created with generic_budget, no budget (the run-time-sized generic kernel)
        never       the same handle, a budget no row reaches (the CONT twin, nothing parks)
        cut24       the same handle, a budget of 24 plus the continuation
      `parent` and `this` run the static-LDS instantiation of the shape, the three opted-in variants the run-time-sized kernel and its
      CONT twin: outputs bit for bit equal within each group (against `this` / against `optin`); between the groups - two
      instantiations of one template with other constants, whose rounding differs - whether status and iteration counts are equal on
      every row and the largest |dX| are reported, not required (a row at the edge of the tolerance takes one iteration more or less)."""
import argparse
import importlib.util
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import mmpc_loader  # noqa: E402
from oracle import nlp, synth  # noqa: E402

B = 8192
KEYS = ("X", "U", "s", "status", "iters", "cost", "err")


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
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent"); ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "generic_continuation_timing.txt"))
    args = ap.parse_args()
    mm = mmpc_loader.load()
    d = synth.make_batch(B, N=20, M=5, config_id=4)
    par = nlp.WholeBodyParams(N=20)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    xi, tr, ur, ob = t(np.clip(d["x_init"], par.xlim[0], par.xlim[1])), t(d["traj_ref"]), t(d["u_ref"]), t(d["obs"])
    ul = torch.zeros((B, 20, 5), dtype=torch.float64, device=dev)
    mk = lambda pkg, **kw: pkg.MPCWholeBody(pkg.MobileManipulator(0.1), [], [], N=20, max_batch=B, n_obstacles=5, **kw)._engine
    os.environ["MMPC_FORCE_GENERIC"] = "1"
    try:
        engs = {}
        if args.parent:
            engs["parent"] = mk(load_parent(args.parent))
        engs["this"] = mk(mm)
        engs["optin"] = mk(mm, generic_budget=True)
        engs["never"] = mk(mm, generic_budget=True)
        engs["cut24"] = mk(mm, generic_budget=True)
    finally:
        del os.environ["MMPC_FORCE_GENERIC"]
    assert not any(e.runs_specialised for e in engs.values())
    engs["never"].set_iteration_budget(1 << 20)
    engs["cut24"].set_iteration_budget(24)

    def run(k, out=None):
        e = engs[k]
        out = e.solve_batch_device(xi, tr, ur, ul, ob, out=out)
        if k == "cut24":
            e.resume_batch_device(xi, tr, ur, ul, ob, out)
        return out

    outs = {k: run(k) for k in engs}
    torch.cuda.synchronize()
    nsusp = int((engs["this"].solve_batch_device(xi, tr, ur, ul, ob)["iters"] > 24).sum())
    times = {k: [] for k in engs}
    for _ in range(args.rounds):
        for k in engs:
            times[k].append(timed(lambda: run(k, outs[k])))
    ref_of = lambda k: "this" if k in ("parent", "this") else "optin"
    same = {k: all(bool(torch.equal(outs[k][q], outs[ref_of(k)][q])) for q in KEYS) for k in engs}
    across = all(bool(torch.equal(outs["optin"][q], outs["this"][q])) for q in ("status", "iters"))
    dx = float((outs["optin"]["X"] - outs["this"]["X"]).abs().max())
    it = outs["this"]["iters"]
    lines = ["C4 batch (B = %d, N = 20, M = 5, config 4) under MMPC_FORCE_GENERIC, %d rounds, the variants alternating in one process" % (B, args.rounds),
             "iterations: mean %.1f, max %d; rows with more than 24: %d" % (float(it.double().mean()), int(it.max()), nsusp)]
    for k in engs:
        v = times[k]
        lines.append("  %-8s best %8.2f ms  spread %6.2f ms  (%s)  outputs bit for bit those of `%s`: %s" % (
            k, min(v), max(v) - min(v), " ".join("%.2f" % x for x in v), ref_of(k), same[k]))
    lines.append("  `optin` against `this` (run-time-sized against static-LDS instantiation): status and iterations equal: %s, max |dX| %.2e" % (across, dx))
    ok = all(same.values())
    if args.parent:
        p, m = times["parent"], times["this"]
        met = min(m) <= min(p) + (max(p) - min(p))
        ok = ok and met
        lines.append("  default handle: this build's best within the parent's best + its own spread: %s" % ("met" if met else "MISSED"))
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
