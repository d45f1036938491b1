"""A/B timing of the LEVELS policy (INVSIM_POLICY_LEVELS) against BaseStock and
against the open-loop route (HIP events; every variant in a fresh child process
under its own time limit, several runs with the variants alternating inside
every run).

  part r  one launch of K = 30 from a reset, us per launch; "-metrics": metrics
          only, "-full": obs + reward + flags + metrics:
            basestock@parent-*  rollout_policy(BaseStockAgent(1.0)) on another build
                                (--parent-tree: a checkout of the parent commit with
                                its library built)
            basestock-*         the same on this build
            levels-*            rollout_policy(LevelsAgent.from_safety_factor(env, 1.0)):
                                the same trajectory from a per-env [N, 3] tensor
            levels-ro-*         the same with reorder points (+inf: the same trajectory)
            plan-*              rollout_metrics on the precomputed [30, N, 3] plan of
                                the same orders, the batched route before LEVELS
  part t  wall clock (perf_counter around the call, which ends synchronised), ms:
            evaluate-1024x64    evaluate_levels of 1 024 candidates x 64 episodes
            tune-1-256x64       tune_levels(population=256, n_episodes=64, iterations=1)
            tune-5-256x64       the same with iterations=5 (an iteration: the difference / 4)

  python tools/policy_levels_ab.py --part r|t [--parent-tree DIR] [--runs 5] [--raw FILE] > part.md

The child that runs directly after a plan-* child (the one-wave run kernels)
measures 12-13 us more per launch than the same variant anywhere else in the
order, on either build (profiles/policy_levels/table.md, "Child order").  So
after every plan-* child an untimed spacer child (basestock-metrics, its line
dropped) runs before the next variant; --no-spacer leaves it out.

A child that fails or runs out of time ends the whole measurement: nothing
more is started on the GPU after it.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 30
SHAPES = [("InvManagementBacklogEnv", 65536), ("InvManagementLostSalesEnv", 32768)]
PARTS = {
    "r": ["basestock@parent-metrics", "basestock-metrics", "levels-metrics", "levels-ro-metrics", "plan-metrics",
          "basestock@parent-full", "basestock-full", "levels-full", "levels-ro-full", "plan-full"],
    "t": ["evaluate-1024x64", "tune-1-256x64", "tune-5-256x64"],
}
CHILD_LIMIT_S = 150


def child(tree, variant, cls, n, launches):
    sys.path.insert(0, os.path.join(tree, "or-gym-inventory_amd"))
    import numpy as np
    import torch
    import invsim
    dev = torch.device("cuda:0")
    env_cls = getattr(invsim, cls)
    if variant in PARTS["t"]:
        from invsim.policies import evaluate_levels, tune_levels
        lv = np.random.default_rng(0).uniform(0.0, 1.0, size=(1024, 3)) * np.array([120.0, 360.0, 660.0])
        t = []
        for _ in range(launches):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if variant.startswith("evaluate"):
                evaluate_levels(lv, env_cls, n_episodes=64, device=dev)
            else:
                tune_levels(env_cls, n_episodes=64, population=256, iterations=int(variant.split("-")[1]), device=dev)
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        t = sorted(t[1:])                      # the first call warms up (library handles, allocator)
        print(json.dumps({"variant": variant, "cls": cls, "launches": launches, "unit": "ms per call",
                          "median": t[len(t) // 2], "min": t[0]}))
        return
    env = env_cls(n, device=dev, autoreset_mode="disabled")
    env.reset(seed=11)
    full = variant.endswith("-full")
    met = torch.zeros((n, invsim.policies.metrics_dim(env)), dtype=torch.float64, device=dev)
    if variant.startswith("basestock"):
        agent = invsim.BaseStockAgent(1.0)
    elif variant.startswith("levels"):
        ro = torch.full((n, 3), float("inf"), dtype=torch.float64, device=dev) if "-ro-" in variant else None
        agent = invsim.LevelsAgent.from_safety_factor(env, np.ones(n))
        agent.reorder = ro
    else:
        plan = env.rollout_policy(invsim.BaseStockAgent(1.0), K, actions=True)["actions"]

    def launch():
        if variant.startswith("plan"):
            env.rollout_metrics(plan, metrics=met, obs=full, rewards=full)
        else:
            env.rollout_policy(agent, K, obs=full, rewards=full, metrics=met)

    for _ in range(3):
        env.reset()
        launch()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for a, b in ev:
        env.reset()              # every timed launch covers periods 0 .. K - 1
        a.record()
        launch()
        b.record()
    torch.cuda.synchronize()
    us = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    print(json.dumps({"variant": variant, "cls": cls, "n": n, "K": K, "launches": launches, "unit": "us per launch",
                      "median": us[len(us) // 2], "min": us[0]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=4, metavar=("TREE", "VARIANT", "CLS", "N"))
    ap.add_argument("--part", choices=sorted(PARTS), default="r")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--raw", default=None, help="append every child's JSON line to this file")
    ap.add_argument("--variants", default=None, help="comma-separated variants of the part, in the order to run them "
                                                     "(a child's time can depend on the child before it)")
    ap.add_argument("--no-spacer", action="store_true", help="no spacer child after a plan-* child")
    ap.add_argument("--shapes", default=None, help="comma-separated indices into SHAPES (default: all of the part's)")
    args = ap.parse_args()
    if args.child:
        tree, variant, cls, n = args.child
        return child(tree, variant, cls, int(n), args.launches)
    variants = args.variants.split(",") if args.variants else PARTS[args.part]
    if any(v not in PARTS[args.part] for v in variants):
        sys.exit(f"--variants: part {args.part} has {PARTS[args.part]}")
    variants = [v for v in variants if "@parent" not in v or args.parent_tree]
    shapes = SHAPES[:1] if args.part == "t" else SHAPES
    if args.shapes:
        shapes = [SHAPES[int(i)] for i in args.shapes.split(",")]
    launches = min(args.launches, 6) if args.part == "t" else args.launches
    res = {}
    def run_child(v, cls, n):
        tree = args.parent_tree if "@parent" in v else ROOT
        cmd = [sys.executable, os.path.abspath(__file__), "--launches", str(launches), "--child", tree, v, cls, str(n)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT_S)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit(f"{v} {cls} {n}: child exit {p.returncode}; stopping")
        return p.stdout.strip().splitlines()[-1]

    for cls, n in shapes:
        for run in range(args.runs):
            for v in variants:
                line = run_child(v, cls, n)
                if v.startswith("plan") and not args.no_spacer:
                    run_child("basestock-metrics", cls, n)      # dropped: see the module text
                if args.raw:
                    with open(args.raw, "a") as f:
                        f.write(line + "\n")
                res.setdefault((cls, n, v), []).append(json.loads(line)["median"])
    unit = {"r": f"us per {K}-step launch (HIP events)", "t": "ms per call (wall clock, synchronised)"}[args.part]
    print(f"{unit}, median of the launches of a run, min - max over {args.runs} runs\n")
    print("| env | N | " + " | ".join(variants) + " |")
    print("|---|---|" + "---|" * len(variants))
    for cls, n in shapes:
        cells = [f"{min(res[cls, n, v]):.2f} - {max(res[cls, n, v]):.2f}" for v in variants]
        print(f"| {cls} | {n if args.part == 'r' else '-'} | " + " | ".join(cells) + " |")


if __name__ == "__main__":
    main()
