"""Greedy list scheduling of a batch's iteration counts on n slots, in the three launch orders - what a launch of one wave per
instance would take if a freed slot went to the next instance of the order at once and every iteration cost the same (CPU only):
  python tools/list_schedule_sim.py [--seeds 3 4 5] [--slots 1024] [--batch 8192] [--counts FILE.npy [--keys FILE.npy]]
                                    [--turnover U] [--out FILE]
      the iteration counts come from the CPU oracle (oracle/mmpc_oracle.c, the C4 generator: whole-body N = 20, M = 5) on the
      seeds given - they equal the device's on 99.87 % of the instances - or from --counts (e.g. the `iters` array of
      bench.py --dump-outputs); the a-priori key is the host mirror of mmpc_difficulty_key (circle term).  Orders: batch order,
      descending key (ties in batch order; the device breaks them by atomics), descending count (the exact longest-first order).
      --turnover U: iteration units a slot loses between two instances (dispatch of a workgroup, its prologue and epilogue).
      Per order: makespan in iteration units, the time the queue runs empty, the mean load of a slot (sum / slots: the bound), and
      the count of the instance that ends last."""
import argparse
import heapq
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BASE_R = 0.4      # MMPC_BASE_R (csrc/mmpc_core.h)


def difficulty_key(traj_ref, obs):
    """mmpc_difficulty_key for a static record: max over stages and obstacles of (r + base radius) - |ref_k - centre|, as 0..255"""
    d = traj_ref[:, :, None, :2] - obs[:, None, :, :2]
    worst = ((obs[:, None, :, 2] + BASE_R) - np.sqrt((d * d).sum(-1))).max(axis=(1, 2))
    return np.clip((worst + 1.5) * (255.0 / 2.5), 0.0, 255.0).astype(np.int64)


def list_schedule(counts, order, slots, turnover=0.0):
    """(makespan, time the last instance starts, index of the instance that ends last)"""
    free = [0.0] * min(slots, len(order))
    heapq.heapify(free)
    end_max, last, start_last = 0.0, -1, 0.0
    for b in order:
        t0 = heapq.heappop(free)
        t1 = t0 + counts[b] + turnover
        heapq.heappush(free, t1)
        start_last = t0
        if t1 > end_max:
            end_max, last = t1, b
    return end_max, start_last, last


def orders(counts, keys):
    B = len(counts)
    o = {"batch order": np.arange(B)}
    if keys is not None:
        o["by key"] = np.argsort(-keys, kind="stable")
    o["exact"] = np.argsort(-counts, kind="stable")
    return o


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, nargs="*", default=[3, 4, 5])
    ap.add_argument("--slots", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--counts", default=None)
    ap.add_argument("--keys", default=None)
    ap.add_argument("--turnover", type=float, default=0.0)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cases = []
    if args.counts:
        cases.append((os.path.basename(args.counts), np.load(args.counts).astype(np.int64).ravel(),
                      np.load(args.keys).astype(np.int64).ravel() if args.keys else None))
    else:
        from oracle import coracle, nlp, synth
        par = nlp.WholeBodyParams()
        for seed in args.seeds:
            d = synth.make_batch(args.batch, config_id=seed)
            x = np.clip(d["x_init"], par.xlim[0], par.xlim[1])
            o = coracle.solve_batch(par, x, d["traj_ref"], d["u_ref"], np.zeros((args.batch, par.N, par.nu)), d["obs"], nthreads=args.threads)
            cases.append(("seed %d" % seed, o["iters"].astype(np.int64), difficulty_key(d["traj_ref"], d["obs"])))
    lines = ["list scheduling on %d slots, turnover %.2f iteration units per instance" % (args.slots, args.turnover)]
    for name, counts, keys in cases:
        lines.append("%s: %d instances, iterations sum %d mean %.2f max %d, sum / slots %.1f" % (
            name, len(counts), counts.sum(), counts.mean(), counts.max(), counts.sum() / args.slots))
        for oname, order in orders(counts, keys).items():
            span, start_last, last = list_schedule(counts, order, args.slots, args.turnover)
            lines.append("  %-12s makespan %6.1f units | the queue is empty at %6.1f | the instance that ends last has %d iterations" % (
                oname, span, start_last, counts[last]))
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
