#!/usr/bin/env python3
"""Resource metadata and code size of the kernels of two device code objects, side by side.

usage: tools/kernel_meta_diff.py A.co B.co [name-filter]
The code objects are what tools/kernel_meta.sh leaves behind (MMPC_META_OUT=A.co tools/kernel_meta.sh in each tree).  Per kernel:
VGPR, AGPR, SGPR, spills, scratch bytes, static LDS bytes (code-object notes) and the size of the kernel's code (its symbol); a
kernel that is in both objects is marked `same` when all of them agree, `text` when its code bytes are identical too."""
import re
import subprocess
import sys

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


def read(co):
    notes = subprocess.check_output([READELF, "--notes", co], text=True)
    out = {}
    for blk in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        blk = ".agpr_count:" + blk
        g = lambda k: (re.search(r"\." + k + r":\s*(\S+)", blk) or [None, "?"])[1]
        name = g("name")
        out[name] = {k: g(k) for k in KEYS}
    syms = subprocess.check_output([READELF, "-s", "-W", co], text=True)
    text = open(co, "rb").read()
    secs = subprocess.check_output([READELF, "-S", "-W", co], text=True)
    m = re.search(r"\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", secs)
    addr, off = int(m.group(1), 16), int(m.group(2), 16)
    for line in syms.splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == "FUNC" and f[7] in out:
            size, val = int(f[2]), int(f[1], 16)
            out[f[7]]["code_bytes"] = size
            out[f[7]]["_text"] = text[off + val - addr: off + val - addr + size]
    return out


def main():
    a, b = read(sys.argv[1]), read(sys.argv[2])
    flt = sys.argv[3] if len(sys.argv) > 3 else ""
    print("%-64s %5s %5s %5s %6s %6s %7s %7s %9s  %s" % ("kernel (A | B)", "vgpr", "agpr", "sgpr", "vspill", "sspill", "scratch", "lds", "code", ""))
    for name in list(a) + [n for n in b if n not in a]:
        if flt and flt not in name:
            continue
        rows = [(t, d[name]) for t, d in (("A", a), ("B", b)) if name in d]
        same = len(rows) == 2 and all(rows[0][1].get(k) == rows[1][1].get(k) for k in KEYS + ("code_bytes",))
        mark = ("text" if rows[0][1].get("_text") == rows[1][1].get("_text") else "same") if same else ("" if len(rows) == 2 else "only " + rows[0][0])
        short = re.sub(r"PK10MmpcParams.*", "", name)
        for t, r in (rows[:1] if same else rows):
            print("%-64s %5s %5s %5s %6s %6s %7s %7s %9s  %s" % ((short if same else t + " " + short)[:64], r["vgpr_count"], r["agpr_count"], r["sgpr_count"],
                                                                    r["vgpr_spill_count"], r["sgpr_spill_count"], r["private_segment_fixed_size"],
                                                                    r["group_segment_fixed_size"], r.get("code_bytes", "?"), mark))


if __name__ == "__main__":
    main()
