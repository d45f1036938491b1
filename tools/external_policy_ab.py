"""A/B timing of invsim_rollout_metrics and the TorchPolicyAgent closed loop
(HIP events; every variant in a fresh child process under its own time limit,
several runs with the variants alternating inside every run).

  part a  one call per step, 30 calls from a reset between two events, us per call:
            step@parent   env.step on another build (--parent-tree: a checkout of the
                          parent commit with its library built)
            step          env.step on this build
            metrics1      env.rollout_metrics of one row, obs + reward + flags + metrics
            metrics1-bare the same, metrics only
  part b  one launch of K = 30, us per launch:
            constant-metrics / constant-full   rollout_policy(ConstantOrderAgent), metrics only /
                                               obs + reward + flags + metrics (the fused kernels)
            ext-metrics / ext-full             rollout_metrics of the same constant action rows
                                               (the one-wave run kernels' EXT variants)
  part c  evaluate_agent, 65 536 InvMgmt Backlog episodes of 30 steps, us per evaluation
          (the function's own Time column times the episodes: wall clock around
          the synchronised rollout; divide by 65 536 for the time per episode):
            basestock     in-kernel BaseStockAgent
            torch-actor   TorchPolicyAgent around a 33-64-64-3 tanh actor

  python tools/external_policy_ab.py --part a|b|c [--parent-tree DIR] [--runs 5] [--raw FILE] > part.md

A child that fails or runs out of time ends the whole measurement: nothing
more is started on the GPU after it.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 30
SHAPES = [("InvManagementBacklogEnv", 65536), ("InvManagementLostSalesEnv", 32768),
          ("NetInvMgmtBacklogEnv", 32768), ("NewsvendorEnv", 65536)]
PARTS = {
    "a": ["step@parent", "step", "metrics1", "metrics1-bare"],
    "b": ["constant-metrics", "ext-metrics", "constant-full", "ext-full"],
    "c": ["basestock", "torch-actor"],
}
CHILD_LIMIT_S = 150


def _events(n):
    import torch
    return [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]


def child(tree, variant, cls, n, launches):
    sys.path.insert(0, os.path.join(tree, "or-gym-inventory_amd"))
    import torch
    import invsim
    dev = torch.device("cuda:0")
    if variant in PARTS["c"]:
        if variant == "basestock":
            agent = invsim.BaseStockAgent(1.0)
        else:
            torch.manual_seed(0)
            body = torch.nn.Sequential(torch.nn.Linear(33, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(),
                                       torch.nn.Linear(64, 3), torch.nn.Tanh()).to(dev)
            high = torch.tensor([100.0, 200.0, 230.0], device=dev)
            agent = invsim.TorchPolicyAgent(lambda o: high * (0.5 + 0.6 * body(o * 0.01)), name="Actor")
        t = []
        for _ in range(launches):
            res = invsim.evaluate_agent(agent, getattr(invsim, cls), {}, n_episodes=n, device=dev)
            t.append(float(res["Time"][0]) * 1e6 * n)      # Time is seconds per episode
        t = sorted(t[1:])                      # the first call warms up (library handles, allocator)
        print(json.dumps({"variant": variant, "cls": cls, "n": n, "launches": launches, "unit": "us per evaluation",
                          "median_us": t[len(t) // 2], "min_us": t[0]}))
        return
    env = getattr(invsim, cls)(n, device=dev)
    env.reset(seed=11)
    agent = invsim.ConstantOrderAgent(0.1)
    row = torch.as_tensor(agent.action(env), device=dev).expand(n, env.action_dim).contiguous()
    rows = row.expand(K, n, env.action_dim).contiguous()
    one = rows[:1]
    met = torch.zeros((n, invsim.policies.metrics_dim(env)), dtype=torch.float64, device=dev)

    def launch():
        if variant.startswith("step"):
            for _ in range(K):
                env.step(row)
        elif variant == "metrics1":
            for _ in range(K):
                env.rollout_metrics(one, metrics=met)
        elif variant == "metrics1-bare":
            for _ in range(K):
                env.rollout_metrics(one, metrics=met, obs=False, rewards=False)
        elif variant == "constant-metrics":
            env.rollout_policy(agent, K, obs=False, rewards=False, metrics=met)
        elif variant == "constant-full":
            env.rollout_policy(agent, K, obs=True, rewards=True, metrics=met)
        elif variant == "ext-metrics":
            env.rollout_metrics(rows, metrics=met, obs=False, rewards=False)
        else:
            env.rollout_metrics(rows, metrics=met)

    per = K if variant in PARTS["a"] else 1
    for _ in range(3):
        env.reset()
        launch()
    torch.cuda.synchronize()
    ev = _events(launches)
    for a, b in ev:
        env.reset()              # every timed launch covers periods 0 .. K - 1
        a.record()
        launch()
        b.record()
    torch.cuda.synchronize()
    us = sorted(a.elapsed_time(b) * 1e3 / per for a, b in ev)
    print(json.dumps({"variant": variant, "cls": cls, "n": n, "K": K, "launches": launches,
                      "unit": "us per call" if per > 1 else "us per launch",
                      "median_us": us[len(us) // 2], "min_us": us[0]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=4, metavar=("TREE", "VARIANT", "CLS", "N"))
    ap.add_argument("--part", choices=sorted(PARTS), default="a")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--raw", default=None, help="append every child's JSON line to this file")
    args = ap.parse_args()
    if args.child:
        tree, variant, cls, n = args.child
        return child(tree, variant, cls, int(n), args.launches)
    variants = [v for v in PARTS[args.part] if v != "step@parent" or args.parent_tree]
    shapes = [SHAPES[0]] if args.part == "c" else SHAPES
    launches = min(args.launches, 6) if args.part == "c" else args.launches
    res = {}
    for cls, n in shapes:
        for run in range(args.runs):
            for v in variants:
                tree = args.parent_tree if v == "step@parent" else ROOT
                cmd = [sys.executable, os.path.abspath(__file__), "--launches", str(launches),
                       "--child", tree, v, cls, str(n)]
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT_S)
                if p.returncode != 0:
                    sys.stderr.write(p.stdout + p.stderr)
                    sys.exit(f"{v} {cls} {n}: child exit {p.returncode}; stopping")
                line = p.stdout.strip().splitlines()[-1]
                if args.raw:
                    with open(args.raw, "a") as f:
                        f.write(line + "\n")
                res.setdefault((cls, n, v), []).append(json.loads(line)["median_us"])
    unit = {"a": "us per call (30 calls from a reset between two HIP events)", "b": f"us per {K}-step launch (HIP events)",
            "c": "us per evaluation of all episodes (evaluate_agent's Time x episodes)"}[args.part]
    print(f"{unit}, median of the launches of a run, min - max over {args.runs} runs\n")
    print("| env | N | " + " | ".join(variants) + " |")
    print("|---|---|" + "---|" * len(variants))
    for cls, n in shapes:
        cells = [f"{min(res[cls, n, v]):.2f} - {max(res[cls, n, v]):.2f}" for v in variants]
        print(f"| {cls} | {n} | " + " | ".join(cells) + " |")


if __name__ == "__main__":
    main()
