"""Wall time of a fleet mission under the reference protocol and with run_mission(warm_start="shifted") (B = 8192, N = 20, M = 3, the
fleet and the pose targets of tests/mission_emu_helper.py:mission_fleet: the fleets of profiles/fleet_mission.txt, T = 160, and
profiles/fleet_manipulate.txt, T = 240 with the manipulate phase); writes profiles/fleet_mission_warm.txt.  With --meta: the kernel
metadata report profiles/fleet_mission_warm_kernel_meta.txt (no GPU needed).

  python tools/fleet_mission_warm_probe.py [--parent DIR] [--out FILE]
      three rounds alternating the variants, host clock around a run that ends in a synchronise, best and spread of each.
      --parent DIR: a checkout of the parent commit with its library built: its run_mission(160) in the same rounds.
      Condition: the reference protocol's outputs bit for bit the parent's and this build's best time within the parent's best plus
      the parent's own spread (the default path queues nothing new).  What the warm start does to the tick time is reported, not bounded.
  python tools/fleet_mission_warm_probe.py --meta LISTING --meta-parent LISTING [--meta-out FILE]
      LISTING: the listing of tools/kernel_meta.sh for this tree and for the parent commit's.  Condition: every kernel of the parent
      is there with the same registers, spills, scratch and LDS, and the guess kernel is the one addition, with scratch 0 and LDS 0.
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

N, M, B, ROUNDS = 20, 3, 8192, 3
PHASES = ((0, "move"), (1, "approach"), (2, "rotate"), (4, "manipulate"))


def meta_report(listing, parent, out):
    rows = lambda path: {l[:78].rstrip(): l[78:].split() for l in open(path).read().splitlines() if " vgpr " in l}
    new, old = rows(listing), rows(parent)
    fmt = lambda k, v: "  %-78s %s" % (k, " ".join("%s %5s" % (a, b) for a, b in zip(v[::2], v[1::2])))
    lines = ["kernel metadata of libmmpc.so with the guess kernel (llvm-readelf --notes of the gfx950 code object of the library as",
             "build.py builds it, in the format of tools/kernel_meta.sh; names cut at 78 characters)", "",
             "the new kernel beside the three glue kernels of a mission tick:"]
    for name in ("mmpc_tick_kernel", "mmpc_mission_kernel", "mmpc_manipulate_kernel", "mmpc_guess_kernel"):
        lines += [fmt(k, v) for k, v in new.items() if name in k]
    for k, v in new.items():
        if "mmpc_guess_kernel" in k:
            vg = int(dict(zip(v[::2], v[1::2]))["vgpr"])
            lines.append("  guess kernel: occupancy by registers min(8, 512 // %d) = %d waves/SIMD (VGPRs in granules of 8; no LDS to limit it; the compiler's "
                         "own remark is printed by tests/test_fleet_guess_cpu.py)" % (-(-vg // 8) * 8, min(8, 512 // (-(-vg // 8) * 8))))
    changed = [k for k in old if new.get(k) != old[k]]
    added = [k for k in new if k not in old]
    lines += ["", "against the parent commit, the %d kernels that existed before: %d unchanged in vgpr, agpr, vspill, sspill, scratch and lds" % (
        len(old), len(old) - len(changed))]
    lines += ["  CHANGED %s: %s -> %s" % (k, " ".join(old[k]), " ".join(new.get(k, ["missing"]))) for k in changed]
    lines += ["added: %s" % ", ".join(added), "", "all kernels:"]
    lines += [fmt(k, v) for k, v in new.items()]
    text = "\n".join(lines) + "\n"
    print(text)
    open(out, "w").write(text)
    ok = not changed and len(added) == 1 and "mmpc_guess_kernel" in added[0]
    if ok:
        g = dict(zip(new[added[0]][::2], new[added[0]][1::2]))
        ok = int(g["scratch"]) == 0 and int(g["lds"]) == 0
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fleet_mission_warm.txt"))
    ap.add_argument("--meta"); ap.add_argument("--meta-parent")
    ap.add_argument("--meta-out", default=os.path.join(ROOT, "profiles", "fleet_mission_warm_kernel_meta.txt"))
    ap.add_argument("--commit", help="label of the code measured, for the report (default: git rev-parse HEAD)")
    ap.add_argument("--robots", type=int, default=B)
    args = ap.parse_args()
    if args.meta:
        return meta_report(args.meta, args.meta_parent, args.meta_out)
    import torch
    import mmpc_loader
    import mission_emu_helper as H
    from fleet_manipulate_probe import load_parent
    nb = args.robots
    mm = mmpc_loader.load()
    F = H.mission_fleet(mm, nb, N, 0.1)
    fleet = mm.DeviceFleet(mm, F["x0"], F["glob"], F["obs0"], F["vel"], N=N)
    man = dict(pose=F["pose"], t_manipulate=2.0)
    try:
        commit = args.commit or subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL, text=True).strip()
    except Exception:
        commit = "working tree (no git metadata)"
    lines = ["fleet mission warm-start probe: B = %d, N = %d, M = %d; %s; taken on top of commit %s" % (nb, N, M, torch.cuda.get_device_name(0), commit),
             "wall time of one run: host clock, ends in a synchronise; streams=3 (with manipulate four); %d rounds alternating the variants after one "
             "run of 5 ticks of each (handles and buffers are created there)" % ROUNDS,
             "a failed solve does not stop a robot; a tick lasts as long as its slowest solve"]
    rc = 0
    keys = ("u0", "iters", "status", "phase", "counts", "x", "final_phase")
    for title, T, kw, last_phase in (("without the manipulate phase", 160, {}, 3), ("with the manipulate phase", 240, dict(manipulate=man), 5)):
        variants = {"reference": lambda: fleet.run_mission(T, **kw), "shifted": lambda: fleet.run_mission(T, warm_start="shifted", **kw)}
        warmup = {"reference": lambda: fleet.run_mission(5, **kw), "shifted": lambda: fleet.run_mission(5, warm_start="shifted", **kw)}
        if args.parent and not kw:
            parent = load_parent(args.parent)
            pfleet = parent.DeviceFleet(parent, F["x0"], F["glob"], F["obs0"], F["vel"], N=N)
            variants["reference, parent commit"] = lambda: pfleet.run_mission(T)
            warmup["reference, parent commit"] = lambda: pfleet.run_mission(5)
        for fn in warmup.values():
            fn(); torch.cuda.synchronize()
        times = {k: [] for k in variants}; last = {}
        for _ in range(ROUNDS):
            for k, fn in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                last[k] = fn()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) * 1e3)
        lines += ["", "%s, T = %d ticks:" % (title, T)]
        for k, v in times.items():
            r = last[k]
            ph = r["phase"]
            nsolve = int(((ph < 3) | (ph == 4)).sum())
            lines.append("  %-26s best %9.2f ms  spread %7.2f ms  (%s)  %7.3f ms per tick  %8.0f solves/s  solves %d" % (
                k, min(v), max(v) - min(v), " ".join("%.2f" % t for t in v), min(v) / T, nsolve / (min(v) * 1e-3), nsolve))
        for k in ("reference", "shifted"):
            r = last[k]
            ph, st, it = r["phase"], r["status"], r["iters"]
            lines.append("  %s: robots finished (phase %d after T ticks) %d of %d; every solve converged: %s; iterations from tick 1 on: mean %.2f" % (
                k, last_phase, int((r["final_phase"] == last_phase).sum()), nb, bool(r["all_converged"]),
                float(it[:, 1:][(ph[:, 1:] < 3) | (ph[:, 1:] == 4)].double().mean())))
            for p, name in PHASES:
                sel = ph == p
                if int(sel.sum()):
                    lines.append("    %-10s solves %8d  status 1: %5d  status 2: %5d  iterations mean %5.1f  slowest %4d" % (
                        name, int(sel.sum()), int((st[sel] == 1).sum()), int((st[sel] == 2).sum()), float(it[sel].double().mean()), int(it[sel].max())))
        same0 = all(bool(torch.equal(last["reference"][k][:, 0], last["shifted"][k][:, 0])) for k in ("u0", "iters", "status", "phase"))
        lines.append("  tick 0 of the shifted run bit for bit the reference protocol's: %s" % same0)
        r, s = min(times["reference"]), min(times["shifted"])
        lines.append("  shifted against reference: %.3f -> %.3f ms per tick (%+.1f %%)" % (r / T, s / T, 100 * (s - r) / r))
        if "reference, parent commit" in variants:
            rp, r0 = last["reference, parent commit"], last["reference"]
            same = all(bool(torch.equal(r0[k], rp[k])) for k in keys)
            p, m = times["reference, parent commit"], times["reference"]
            ok = same and min(m) <= min(p) + (max(p) - min(p))
            lines.append("  reference protocol, this build against the parent commit: %s bit for bit equal: %s; this build's best within the parent's "
                         "best + its own spread: %s" % (", ".join(keys), same, "met" if ok else "MISSED"))
            rc = 0 if ok else 1
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, "w").write(text)
    return rc


if __name__ == "__main__":
    sys.exit(main())
