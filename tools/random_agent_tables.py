"""The two tables of profiles/random_agent/table.md from the raw lines beside it:

  python tools/random_agent_tables.py profiles/random_agent

raw_random_agent_ab.jsonl: tools/random_agent_ab.py --raw (one line per child
process); raw_bench_ab.jsonl: tools/bench_ab.sh (one line per bench.py run).
"""
import collections
import json
import os
import sys

VARIANTS = ["compose@parent", "compose", "sample+rollout", "random", "random-metrics", "constant-metrics"]
WORKLOADS = ["invmgmt_backlog", "invmgmt_lostsales", "net_backlog", "newsvendor"]


def lines(path):
    return [json.loads(ln) for ln in open(path) if ln.strip()]


def main(d):
    ab = collections.defaultdict(list)
    shapes = []
    for r in lines(os.path.join(d, "raw_random_agent_ab.jsonl")):
        if (r["cls"], r["n"]) not in shapes:
            shapes.append((r["cls"], r["n"]))
        ab[r["cls"], r["n"], r["variant"]].append(r["median_us"])
    vs = [v for v in VARIANTS if any(k[2] == v for k in ab)]
    print("us per 30-step launch (HIP events), median of the launches of a run, min - max over the runs\n")
    print("| env | N | " + " | ".join(vs) + " |")
    print("|---|---|" + "---|" * len(vs))
    for cls, n in shapes:
        print(f"| {cls} | {n} | " + " | ".join(f"{min(ab[cls, n, v]):.1f} - {max(ab[cls, n, v]):.1f}" for v in vs) + " |")
    be = collections.defaultdict(list)
    for r in lines(os.path.join(d, "raw_bench_ab.jsonl")):
        be[r["workload"], r["mode"], r["arm"]].append(r)
    print("\n| workload | mode | parent G env-steps/s, min - max | new G env-steps/s, min - max | "
          "parent us / launch | new us / launch | ranges overlap |")
    print("|---|---|---|---|---|---|---|")
    for w in WORKLOADS:
        for m in ("step", "policy"):
            def rng(arm, k, s=1.0):
                v = [x[k] * s for x in be[w, m, arm]]
                return min(v), max(v)
            pv, nv = rng("parent", "value", 1e-9), rng("new", "value", 1e-9)
            pu, nu = rng("parent", "kernel_us"), rng("new", "kernel_us")
            ov = "yes" if nv[1] >= pv[0] else "NO"
            print(f"| {w} | {m} | {pv[0]:.3f} - {pv[1]:.3f} | {nv[0]:.3f} - {nv[1]:.3f} | "
                  f"{pu[0]:.3f} - {pu[1]:.3f} | {nu[0]:.3f} - {nu[1]:.3f} | {ov} |")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "profiles/random_agent")
