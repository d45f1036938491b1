#!/usr/bin/env python3
"""Compare the kernel resource usage of two builds, one remark log per
translation unit (hipcc ... -Rpass-analysis=kernel-resource-usage -c X.hip 2> X.log).

    tools/resource_diff.py PARENT_DIR NEW_DIR [--cxxfilt PATH] [--plain] > resources.md

Every kernel is keyed by (translation unit, demangled name).  Reports the
kernels of the parent that are absent or differ in VGPRs, AGPRs, SGPRs, scratch,
waves/SIMD or spill counts, and lists the EXT (invsim_rollout_metrics)
instantiations beside the policy instantiation they are a variant of: the same
template arguments with RND = EXT = false (the parent's name), or, for the
InvMgmt translation unit invmgmt_ext, the kernel of the same name in invmgmt
(Pcg) / invmgmt_ph (PhiloxGen).

--plain: both builds already have the EXT template argument (every change after
the one that added it): names are compared as they are, and the EXT table is
left out.
"""
import glob
import os
import re
import subprocess
import sys

FIELDS = (("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("TotalSGPRs", "SGPRs"), ("ScratchSize [bytes/lane]", "scratch B/lane"),
          ("Occupancy [waves/SIMD]", "waves/SIMD"), ("SGPRs Spill", "SGPR spills"), ("VGPRs Spill", "VGPR spills"))
REMARK = re.compile(r"remark:\s+([A-Za-z /\[\]]+?): (\S+) \[-Rpass-analysis")


# templates that gained the trailing template argument EXT: their instantiations
# with EXT = false are compared under the parent's names (without that argument)
EXT_TEMPLATES = ("nv_run_kernel<", "net_spec_kernel<", "net_run_kernel<")


def parse(d, cxxfilt, parent_names=False):
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
        if parent_names and d_.startswith(EXT_TEMPLATES) and d_.endswith(", false>"):
            d_ = d_[:-len(", false>")] + ">"
        short[n] = d_
    return {(tu, short[n]): v for (tu, n), v in out.items()}


def row(r):
    return tuple(r.get(k, "?") for k, _ in FIELDS)


def sibling(tu, name):
    if tu == "invmgmt_ext":
        return ("invmgmt_ph" if "PhiloxGen" in name else "invmgmt", name)
    if name.endswith(", false, true>"):
        return (tu, name[:-len(", false, true>")] + ", false>")
    return None


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    cxxfilt = "c++filt"
    if "--cxxfilt" in sys.argv:
        cxxfilt = sys.argv[sys.argv.index("--cxxfilt") + 1]
        args.remove(cxxfilt)
    plain = "--plain" in sys.argv
    old, new = parse(args[0], cxxfilt), parse(args[1], cxxfilt, parent_names=not plain)
    same = [k for k in old if k in new and row(old[k]) == row(new[k])]
    diff = [k for k in old if k in new and row(old[k]) != row(new[k])]
    gone = [k for k in old if k not in new]
    added = [k for k in new if k not in old]
    ext = [k for k in added if sibling(*k) in new and (k[0] == "invmgmt_ext" or k[1].endswith(", false, true>"))]
    other = [k for k in added if k not in ext]
    print(f"- existing instantiations: {len(old)}; identical in " + ", ".join(h for _, h in FIELDS) +
          f": {len(same)}; different in any of them: {len(diff)}")
    print(f"- parent kernels absent from the new build: {len(gone)}")
    print(f"- new kernels: {len(ext)} EXT instantiations and {len(other)} others"
          + (" (" + ", ".join(f"`{n}` in {tu}" for tu, n in other) + ")" if other else ""))
    for title, ks in (("Different", diff), ("Absent", gone)):
        if ks:
            print(f"\n## {title}\n")
            for k in sorted(ks):
                print(f"- `{k[1]}` ({k[0]}): {row(old[k])} -> {row(new.get(k, {}))}")
    if plain:
        return
    worse = []
    print("\n## The EXT instantiations against the policy instantiation they are a variant of\n")
    print("(POL sibling -> EXT)\n")
    print("| kernel (EXT) | translation unit | " + " | ".join(h for _, h in FIELDS) + " |")
    print("|---|---|" + "---|" * len(FIELDS))
    for k in sorted(ext):
        s, e = new[sibling(*k)], new[k]
        cells = [f"{s.get(f, '?')} -> {e.get(f, '?')}" for f, _ in FIELDS]
        print(f"| `{k[1]}` | {k[0]} | " + " | ".join(cells) + " |")
        if int(e["ScratchSize [bytes/lane]"]) > int(s["ScratchSize [bytes/lane]"]) or \
                int(e["Occupancy [waves/SIMD]"]) < int(s["Occupancy [waves/SIMD]"]):
            worse.append(k)
    print(f"\nEXT kernels that gain scratch or lose a wave per SIMD against their sibling: {len(worse)}")
    for k in sorted(worse):
        print(f"- `{k[1]}` ({k[0]})")


if __name__ == "__main__":
    main()
