#!/usr/bin/env python3
"""Compare the kernel resource usage of two builds, one remark log per
translation unit (hipcc ... -Rpass-analysis=kernel-resource-usage -c X.hip 2> X.log).

    tools/resource_diff.py PARENT_DIR NEW_DIR [--cxxfilt PATH] > resources.md

Every kernel is keyed by (translation unit, demangled name).  Reports the
kernels of the parent that are absent or differ in VGPRs, AGPRs, SGPRs, scratch,
waves/SIMD or spill counts, and the kernels only the new build has.

--plain is accepted and ignored (it used to select this behaviour).
"""
import glob
import os
import re
import subprocess
import sys

FIELDS = (("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("TotalSGPRs", "SGPRs"), ("ScratchSize [bytes/lane]", "scratch B/lane"),
          ("Occupancy [waves/SIMD]", "waves/SIMD"), ("SGPRs Spill", "SGPR spills"), ("VGPRs Spill", "VGPR spills"))
REMARK = re.compile(r"remark:\s+([A-Za-z /\[\]]+?): (\S+) \[-Rpass-analysis")


def parse(d, cxxfilt):
    out = {}
    for path in sorted(glob.glob(os.path.join(d, "*.log"))):
        tu = os.path.basename(path)[:-4]
        cur = None
        for line in open(path, errors="replace"):
            m = REMARK.search(line)
            if not m:
                continue
            k, v = m.group(1).strip(), m.group(2)
            if k == "Function Name":
                cur = out.setdefault((tu, v), {})
            elif cur is not None:
                cur[k] = v
    names = sorted({n for _, n in out})
    dem = subprocess.run([cxxfilt], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    short = {}
    for n, d_ in zip(names, dem):
        d_ = re.sub(r"^void ", "", d_)
        d_ = d_.replace("invsim::(anonymous namespace)::", "").replace("invsim::", "")
        depth, end = 0, len(d_)
        for i, ch in enumerate(d_):      # cut the argument list: the first '(' outside the template arguments
            depth += ch == "<"
            depth -= ch == ">"
            if ch == "(" and depth == 0:
                end = i
                break
        d_ = d_[:end]
        short[n] = d_
    return {(tu, short[n]): v for (tu, n), v in out.items()}


def row(r):
    return tuple(r.get(k, "?") for k, _ in FIELDS)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    cxxfilt = "c++filt"
    if "--cxxfilt" in sys.argv:
        cxxfilt = sys.argv[sys.argv.index("--cxxfilt") + 1]
        args.remove(cxxfilt)
    old, new = parse(args[0], cxxfilt), parse(args[1], cxxfilt)
    same = [k for k in old if k in new and row(old[k]) == row(new[k])]
    diff = [k for k in old if k in new and row(old[k]) != row(new[k])]
    gone = [k for k in old if k not in new]
    added = [k for k in new if k not in old]
    print(f"- existing instantiations: {len(old)}; identical in " + ", ".join(h for _, h in FIELDS) +
          f": {len(same)}; different in any of them: {len(diff)}")
    print(f"- parent kernels absent from the new build: {len(gone)}")
    print(f"- new kernels: {len(added)}"
          + (" (" + ", ".join(f"`{n}` in {tu}" for tu, n in added) + ")" if added else ""))
    for title, ks in (("Different", diff), ("Absent", gone)):
        if ks:
            print(f"\n## {title}\n")
            for k in sorted(ks):
                print(f"- `{k[1]}` ({k[0]}): {row(old[k])} -> {row(new.get(k, {}))}")


if __name__ == "__main__":
    main()
