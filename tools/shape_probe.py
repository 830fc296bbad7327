"""Shape libraries (csrc/mmpc_shape.hip, build.py:build_shape_library) beside the generic kernel: kernel metadata and wall times.

  python tools/shape_probe.py --meta [--parent-lib FILE]
      no GPU: reads the code objects out of csrc/libmmpc.so and out of every library under csrc/shapes/ (nothing is compiled) and
      writes profiles/shape_libraries_kernel_meta.txt: registers, spills, scratch and LDS of the six kernels of every shape, and -
      with --parent-lib, the libmmpc.so of the parent commit - whether every kernel of libmmpc.so kept its figures.
      Exit status 1 when one of them differs.
  python tools/shape_probe.py [--parent DIR]
      on the GPU; writes profiles/shape_libraries.txt.  Per shape of SHAPES: B = 8192 seeded instances (oracle.synth.make_batch),
      one solve per launch, the shape's library (specialise="cached": build the libraries first) against the generic kernel of
      this build on the same batch (and of the parent commit: --parent DIR, a checkout of it with its library built), three
      alternating rounds, host clock to a synchronise as tools/obstacle_motion_probe.py does.  Nothing is gated: the table is
      what the feature promises.
"""
import argparse
import glob
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(0, 10, 2), (0, 20, 4), (0, 25, 4), (0, 31, 8), (1, 20, 5)]
B, ROUNDS = 8192, 3
LLVM = os.environ.get("MMPC_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
CSRC = os.path.join(ROOT, "mobile-manipulator-mpc_amd", "csrc")


def kernel_notes(lib):
    """{kernel name: figures} from the gfx950 code object bundled in a shared library (the notes tools/kernel_meta.sh prints)"""
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat"), os.path.join(tmp, "co")
        subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib, fat])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                               "--input=" + fat, "--output=" + co])
        txt = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
    rows = {}
    for blk in re.split(r"\n\s*- \.agpr_count:", txt)[1:]:
        g = lambda k: (re.search(r"\." + k + r":\s*(\S+)", blk) or [None, "?"])[1]
        rows[g("name")] = "vgpr %3s agpr %3s sgpr %3s vspill %3s sspill %3s scratch %5s lds %6s" % (
            g("vgpr_count"), blk.split()[0], g("sgpr_count"), g("vgpr_spill_count"), g("sgpr_spill_count"), g("private_segment_fixed_size"),
            g("group_segment_fixed_size"))
    return rows


def meta(args):
    out = ["kernel metadata of the shape libraries (csrc/shapes/) and of libmmpc.so, from the code objects' notes;",
           "hipcc --offload-arch=gfx950 -O3 -mllvm -amdgpu-mfma-vgpr-form", ""]
    rc = 0
    for lib in sorted(glob.glob(os.path.join(CSRC, "shapes", "libmmpc_shape_*.so")), key=lambda p: [int(v) for v in re.findall(r"\d+", os.path.basename(p))]):
        rows = kernel_notes(lib)
        out.append("%s (%d kB)" % (os.path.basename(lib), os.path.getsize(lib) // 1024))
        for name in sorted(rows):
            m = re.match(r"_Z16mmpc_fast_kernelILi(\d)ELi(\d+)ELi(\d+)ELi(\d)ELb(\d)ELi(\d)E", name)
            if m:
                out.append("    <%s,%s,%s> WPE %s %-23s OPS %s  %s" % (m.group(1), m.group(2), m.group(3), m.group(4),
                                                                     "budgeted / continuation" if m.group(5) == "1" else "one launch", m.group(6), rows[name]))
    mine = kernel_notes(os.path.join(CSRC, "libmmpc.so"))
    if args.parent_lib:
        theirs = kernel_notes(args.parent_lib)
        diff = sorted(k for k in set(mine) | set(theirs) if mine.get(k) != theirs.get(k))
        out += ["", "libmmpc.so against the parent commit's: %d kernels, %d in the parent's; kernels whose registers, spills, scratch or LDS differ: %s"
                % (len(mine), len(theirs), diff if diff else "none")]
        rc = 1 if diff else 0
    out += ["", "all kernels of libmmpc.so:"] + ["  %-82s %s" % (k[:82], mine[k]) for k in sorted(mine)]
    open(os.path.join(ROOT, "profiles", "shape_libraries_kernel_meta.txt"), "w").write("\n".join(out) + "\n")
    print("\n".join(out[:60]))
    return rc


def bench(args):
    import numpy as np
    import torch
    import mmpc_loader
    from oracle import nlp, synth
    from tools.obstacle_motion_probe import rounds
    mm = mmpc_loader.load()
    parent = None
    if args.parent:
        from tools.fleet_tick_probe import load_parent
        parent = load_parent(args.parent)
    dev = torch.device("cuda", 0)
    t_ = lambda a_: torch.from_numpy(np.ascontiguousarray(a_)).to(dev)
    lines = ["shape library probe; %s; B = %d seeded instances, one solve per launch (schedule hint 2), wall time (host clock, ends in a synchronise), "
             "%d rounds alternating the variants" % (torch.cuda.get_device_name(0), B, ROUNDS)]
    fmt = lambda k, v, e, it: "  %-22s best %8.2f ms  spread %6.2f ms  (%s)  %8.0f solves/s  problems per CU %d  LDS %6d B  mean iterations %.2f" % (
        k, min(v), max(v) - min(v), " ".join("%.2f" % t for t in v), B / (min(v) * 1e-3), e.problems_per_cu, e.lds_bytes, it)
    table = []
    for (k, n, m) in SHAPES:
        par = nlp.WholeBodyParams(N=n) if k == 0 else nlp.BaseParams(N=n)
        d = synth.make_batch(B, N=n, M=m, kind="wholebody" if k == 0 else "base", config_id=3 if k == 0 else 2)
        x = t_(np.clip(d["x_init"], par.xlim[0], par.xlim[1]) if k == 0 else d["x_init"])
        tr, ur, ul, ob = t_(d["traj_ref"]), t_(d["u_ref"]), t_(np.zeros((B, n, par.nu))), t_(d["obs"])
        mk = lambda pkg, **kw: pkg._capi.Engine(k, n, m, par.dt, par.ulim, par.xlim, par.dulim, max_batch=B, max_iter=2000, **kw)
        eng = {"shape library": mk(mm, specialise="cached"), "generic": mk(mm)}
        if parent:
            eng["generic, parent"] = mk(parent)
        assert eng["shape library"].runs_specialised and not eng["generic"].runs_specialised, "build the shape's library first (build_shape_library)"
        outs = {key: e.solve_batch_device(x, tr, ur, ul, ob) for key, e in eng.items()}
        for e in eng.values():
            e.set_schedule_hint(2)               # the a-priori launch order: no memory of the launch before (what bench.py times)
        variants = {key: (lambda key=key: eng[key].solve_batch_device(x, tr, ur, ul, ob, out=outs[key])) for key in eng}
        times, last = rounds(variants, warm=2)
        a, g = last["shape library"], last["generic"]
        lines.append("(%d, %d, %d)" % (k, n, m))
        lines += [fmt(key, v, eng[key], float(last[key]["iters"].double().mean())) for key, v in times.items()]
        ratio = min(times["generic"]) / min(times["shape library"])
        lines.append("  shape library against generic: %.2fx; converged %d / %d of %d; equal iteration counts %.4f; max |dX| %.2e max |dU| %.2e" % (
            ratio, int((a["status"] == 0).sum()), int((g["status"] == 0).sum()), B, float((a["iters"] == g["iters"]).double().mean()),
            float((a["X"] - g["X"]).abs().max()), float((a["U"] - g["U"]).abs().max())))
        if parent:
            p = last["generic, parent"]
            lines.append("  generic against the parent's generic: X, U, s, status, iters, cost bitwise equal %s" % all(bool(torch.equal(g[key], p[key])) for key in ("X", "U", "s", "status", "iters", "cost")))
        table.append("  (%d, %2d, %2d)  %8.2f ms  %8.2f ms  %5.2fx" % (k, n, m, min(times["shape library"]), min(times["generic"]), ratio))
        del eng, outs, variants, last
        torch.cuda.empty_cache()
    lines += ["", "summary: shape, shape library, generic kernel, ratio"] + table
    text = "\n".join(lines) + "\n"
    print(text)
    open(args.out, "w").write(text)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meta", action="store_true"); ap.add_argument("--parent-lib")
    ap.add_argument("--parent"); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shape_libraries.txt"))
    args = ap.parse_args()
    return meta(args) if args.meta else bench(args)


if __name__ == "__main__":
    sys.exit(main())
