"""A/B of the launch forms of the specialised C4 kernel (whole-body N = 20, M = 5, B = 8192), on the GPU:
  python tools/persistent_launch_probe.py [--parent DIR] [--seeds 3 4 ...] [--rounds 3] [--steps 10] [--out FILE]
      variants: `persistent` (this tree, mmpc_set_persistent_grid 0: resident workgroups that draw launch positions from a ticket),
      `per-instance` (this tree, persistent grid < 0: one workgroup per instance) and, with --parent DIR (a built checkout of the
      parent commit), `parent`.  Per seed of the C4 generator and per launch order (a-priori key = what bench.py times, batch
      order): `rounds` rounds alternating the variants, each a warm-up launch and `steps` launches on the host clock that ends in
      a synchronise; mean of the rounds and their spread (max - min).  The variants' outputs of a seed are compared bit for bit.
  python tools/persistent_launch_probe.py --stamps [--seeds 3] [--out FILE]
      needs a library built with -DMMPC_STAMP_INST (tools/build_variant.sh): per instance the start and end on the 100 MHz clock all
      XCDs share, the wave's cycle counter at both ends and the XCD; prints, for both launch forms in key order, the cycles
      per iteration of the 100 instances that end last against the batch mean and the time between the end of an instance and the
      start of the next one on the same workgroup (persistent form) or, for the per-instance form, the time from the end of the
      k-th instance to finish to the start of the (k + slots)-th instance to start.
Nothing is gated: the figures go to profiles/persistent_launch.txt by hand."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, N, M = 8192, 20, 5
KEYS = ("X", "U", "s", "status", "iters", "cost", "err")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--seeds", type=int, nargs="*", default=[3])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--stamps", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import mmpc_loader
    from oracle import synth
    mm = mmpc_loader.load()
    dev = torch.device("cuda", 0)
    pkgs = [("persistent", mm, 0), ("per-instance", mm, -1)]
    if args.parent:
        from tools.fleet_tick_probe import load_parent
        pkgs.append(("parent", load_parent(args.parent), None))
    ctrls = {}
    for name, pkg, grid in pkgs:
        c = pkg.MPCWholeBody(pkg.MobileManipulator(0.1), [], [], N=N, max_batch=B, n_obstacles=M)
        ctrls[name] = c
    lines = ["persistent launch probe; %s; B = %d, N = %d, M = %d; %d rounds alternating the variants, %d launches per round after one "
             "warm-up launch, host clock to a synchronise; mean of the rounds (spread = max - min)" % (
                 torch.cuda.get_device_name(0), B, N, M, args.rounds, args.steps)]

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    for seed in args.seeds:
        d = synth.make_batch(B, N=N, M=M, config_id=seed)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        c0 = ctrls["persistent"]
        tens = [t(np.clip(d["x_init"], c0.xlim[0], c0.xlim[1])), t(d["traj_ref"]), t(d["u_ref"]),
                torch.zeros((B, N, 5), dtype=torch.float64, device=dev), t(d["obs"])]
        outs = {}

        def launch(name, mode, n):
            eng = ctrls[name]._engine
            grid = dict((p[0], p[2]) for p in pkgs)[name]
            if grid is not None:
                eng.set_persistent_grid(grid)
            eng.set_schedule_hint(mode)
            outs[name] = eng.solve_batch_device(*tens, out=outs.get(name))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                eng.solve_batch_device(*tens, out=outs[name])
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / max(n, 1) * 1e3

        if args.stamps:
            stamps(mm, ctrls, launch, outs, seed, emit)
            continue
        res = {}
        for mode in (2, 0):
            for r in range(args.rounds):
                for name, _, _ in pkgs:
                    res.setdefault((name, mode), []).append(launch(name, mode, args.steps))
        ref = {k: outs["per-instance"][k].cpu().numpy() for k in KEYS}
        for name, _, _ in pkgs:
            same = all(np.array_equal(outs[name][k].cpu().numpy().view(np.uint8), ref[k].view(np.uint8)) for k in KEYS)
            it = outs[name]["iters"].cpu().numpy()
            f = lambda v: "%.3f ms (%.3f)" % (np.mean(v), np.max(v) - np.min(v))
            emit("%-12s seed %d | batch order %s | a-priori key %s | iters mean %.2f max %d sum %d | outputs bitwise those of per-instance: %s" % (
                name, seed, f(res[(name, 0)]), f(res[(name, 2)]), it.mean(), it.max(), it.sum(), same))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def stamps(mm, ctrls, launch, outs, seed, emit):
    L = mm._capi.lib()
    if not hasattr(L, "mmpc_debug_read_inst_stamps"):
        raise SystemExit("--stamps needs a library built with -DMMPC_STAMP_INST")
    L.mmpc_debug_read_inst_stamps.argtypes = [ctypes.c_void_p, ctypes.c_int]
    eng = ctrls["persistent"]._engine
    import torch
    slots = eng.problems_per_cu * torch.cuda.get_device_properties(0).multi_processor_count
    for name in ("per-instance", "persistent"):
        launch(name, 2, 1)
        launch(name, 2, 0)       # the launch the stamps are read from
        buf = np.zeros((B, 6), np.uint64)
        assert L.mmpc_debug_read_inst_stamps(buf.ctypes.data_as(ctypes.c_void_p), B) == 0
        it = outs[name]["iters"].cpu().numpy().astype(float)
        r0, r1, c0, c1, xcc, wg = (buf[:, i].astype(np.int64) for i in range(6))
        origin = r0.min()
        us0, us1 = (r0 - origin) / 100.0, (r1 - origin) / 100.0
        cyc = (c1 - c0) / it
        last = np.argsort(us1)[-100:]
        clock = np.median((c1 - c0) / np.maximum(r1 - r0, 1)) * 100.0
        emit("%-12s seed %d, key order: launch %.1f us from the first start to the last end; wave clock %.0f MHz" % (name, seed, us1.max(), clock))
        emit("  cycles per iteration: batch mean %.0f (us per iteration %.2f); the 100 instances that end last: mean %.0f, their iterations mean %.1f "
             "(batch %.1f)" % (cyc.mean(), ((us1 - us0) / it).mean(), cyc[last].mean(), it[last].mean(), it.mean()))
        emit("  instances per XCD: %s" % np.bincount(xcc.astype(int), minlength=8).tolist())
        if name == "persistent":
            gaps = []
            for g in np.unique(wg):
                rows = np.nonzero(wg == g)[0]
                rows = rows[np.argsort(us0[rows])]
                gaps.extend((us0[rows[1:]] - us1[rows[:-1]]).tolist())
            gaps = np.array(gaps)
            emit("  end of an instance -> start of the next on the same workgroup (%d turnovers): mean %.2f us, median %.2f, p99 %.2f, max %.2f" % (
                len(gaps), gaps.mean(), np.median(gaps), np.percentile(gaps, 99), gaps.max()))
        else:
            e, s = np.sort(us1), np.sort(us0)
            gaps = s[slots:] - e[:B - slots]
            emit("  k-th end -> (k + %d)-th start (a greedy queue on %d slots would make this 0; %d turnovers): mean %.2f us, median %.2f, p99 %.2f, max %.2f" % (
                slots, slots, len(gaps), gaps.mean(), np.median(gaps), np.percentile(gaps, 99), gaps.max()))
        busy = (us1 - us0).sum() / (slots * us1.max())
        emit("  slot occupancy: sum of the instances' times / (%d slots x launch) = %.3f; first start of the last-starting 1 %%: %.1f us" % (
            slots, busy, np.percentile(us0, 99)))


if __name__ == "__main__":
    main()
