#!/usr/bin/env python3
"""Table of the history kernels' register use from `make -C neutral_amd asm`
(neutral_amd/build/resource_usage.txt): VGPRs, SGPRs, scratch, waves per SIMD.  The kernels'
last template argument, the mask of optional scores (neutral_kernels.h: Score), is spelled out.
  python tools/kernel_resources.py [pattern]
  python tools/kernel_resources.py --compare OTHER/resource_usage.txt [pattern]
--compare: the kernels of the other listing (another commit's) by name against this build's --
every one that moved in VGPRs, AGPRs, SGPRs, scratch, LDS or occupancy, those that exist on one
side only counted: the "off is off" check of a feature behind a new Score bit."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TXT = os.path.join(ROOT, "neutral_amd", "build", "resource_usage.txt")


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names),
                         capture_output=True, text=True).stdout.splitlines()
    return [re.sub(r"\(.*", "", o).replace("neutral::", "").replace("void ", "") for o in out]


SCORES = ((1, "collisions"), (2, "roulette"), (4, "spectrum"), (8, "current"), (16, "outflow"))


def scores_of(demangled):
    """the names of the Score bits in a history kernel's last template argument"""
    m = re.search(r", (\d+)u>$", demangled)
    if not m or not re.match(r"(history_kernel|history_regroup_kernel|stream_kernel)<", demangled):
        return ""
    mask = int(m.group(1))
    return "+".join(name for bit, name in SCORES if mask & bit) or "-"


def read(path):
    rows, cur = [], None
    for line in open(path):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = {"name": m.group(1)}
            rows.append(cur)
            continue
        for key, rx in (("vgpr", r" VGPRs: (\d+)"), ("agpr", r"AGPRs: (\d+)"),
                        ("sgpr", r"TotalSGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                        ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(rx, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return rows


KEYS = ("vgpr", "agpr", "sgpr", "scratch", "lds", "occ")


def compare(other, pat):
    theirs = {r["name"]: r for r in read(other) if re.search(pat, r["name"])}
    ours = {r["name"]: r for r in read(TXT) if re.search(pat, r["name"])}
    moved = [n for n in theirs if n in ours and any(theirs[n].get(k, 0) != ours[n].get(k, 0) for k in KEYS)]
    for n, d in zip(moved, demangle(moved)):
        print(d, " ".join(f"{k} {theirs[n].get(k, 0)} -> {ours[n].get(k, 0)}" for k in KEYS
                          if theirs[n].get(k, 0) != ours[n].get(k, 0)))
    print(f"{len(theirs)} kernels there, {len(ours)} here: {len(set(theirs) & set(ours))} in both, "
          f"{len(moved)} moved, {len(set(theirs) - set(ours))} gone, {len(set(ours) - set(theirs))} new")
    return 1 if moved or set(theirs) - set(ours) else 0


def main():
    args = sys.argv[1:]
    other = None
    if args and args[0] == "--compare":
        other, args = args[1], args[2:]
    pat = args[0] if args else "history|stream_kernel"
    if other:
        sys.exit(compare(other, pat))
    rows = [r for r in read(TXT) if re.search(pat, r["name"])]
    for r, n in zip(rows, demangle([r["name"] for r in rows])):
        print(f"{n:70s} {scores_of(n):32s} vgpr {r.get('vgpr', 0):3d} agpr {r.get('agpr', 0):3d} "
              f"sgpr {r.get('sgpr', 0):3d} scratch {r.get('scratch', 0):4d} waves/SIMD {r.get('occ', 0)}")


if __name__ == "__main__":
    main()
