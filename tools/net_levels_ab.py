"""Timing of the NET_LEVELS policy (INVSIM_POLICY_NET_LEVELS) on the default
supply network against ConstantOrder and against the only way to run the rule
without it, a torch closed loop (HIP events; every variant in a fresh child
process under its own time limit, several runs with the variants alternating
inside every run).

  part r  one launch of K = 30 from a reset at 32 768 envs, metrics only, us per launch:
            constant@parent  rollout_policy(ConstantOrderAgent()) on another build
                             (--parent-tree: a checkout of the parent commit with
                             its library built)
            constant         the same on this build
            netlevels        rollout_policy(NetLevelsAgent.from_mean_demand(env)) from a
                             per-env [N, 11] device tensor
            torch            the same rule in torch (f64 positions from the observation:
                             X, U and the order windows, whose sums are the pipelines) as a
                             TorchPolicyAgent: 30 one-step launches with torch ops between
  part t  wall clock (perf_counter around the call, which ends synchronised), ms:
            evaluate-1024x64 evaluate_levels of 1 024 candidates x 64 episodes
            tune-1-256x64    tune_levels(population=256, n_episodes=64, iterations=1)

  python tools/net_levels_ab.py --part r|t [--parent-tree DIR] [--runs 5] [--raw FILE] > part.md

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
K, N = 30, 32768
CLS = "NetInvMgmtBacklogEnv"
PARTS = {"r": ["constant@parent", "constant", "netlevels", "torch"], "t": ["evaluate-1024x64", "tune-1-256x64"]}
CHILD_LIMIT_S = 150


def torch_rule(env, levels):
    """The rule on the observation, in torch f64 (timing only: the kernels sum the f64 state)."""
    import numpy as np
    import torch
    t = env.topology.tables
    J, E, RL = len(env.main_nodes), len(env.reorder_links), len(env.retail_links)
    dev = env.device
    into = torch.zeros((E, J), dtype=torch.float64, device=dev)        # link -> its purchaser
    into[torch.arange(E), torch.from_numpy(np.asarray(t["pur"][:E], np.int64))] = 1.0
    mkt = torch.zeros((RL, J), dtype=torch.float64, device=dev)
    mkt[torch.arange(RL), torch.from_numpy(np.asarray(t["rl_node"][:RL], np.int64))] = 1.0
    win = torch.zeros((env.obs_dim - RL - J, E), dtype=torch.float64, device=dev)   # window entry -> its link
    o = 0
    for k in range(E):
        L = int(t["L"][k])
        win[o:o + L, k] = 1.0
        o += L
    pur = torch.from_numpy(np.asarray(t["pur"][:E], np.int64)).to(dev)

    def fn(obs):
        x = obs.to(torch.float64)
        pos = x[:, RL:RL + J] + (x[:, RL + J:] @ win) @ into - x[:, :RL] @ mkt
        return torch.clamp(levels - pos[:, pur], min=0.0)              # (convert_actions clips to high)
    return fn


def child(tree, variant, launches):
    sys.path.insert(0, os.path.join(tree, "or-gym-inventory_amd"))
    import numpy as np
    import torch
    import invsim
    dev = torch.device("cuda:0")
    env_cls = getattr(invsim, CLS)
    if variant in PARTS["t"]:
        from invsim.policies import evaluate_levels, tune_levels
        base = np.asarray(invsim.NetLevelsAgent.from_mean_demand(env_cls(1, device=dev)).levels)
        lv = np.random.default_rng(0).uniform(0.0, 3.0, size=(1024, base.size)) * base
        t = []
        for _ in range(launches):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if variant.startswith("evaluate"):
                evaluate_levels(lv, env_cls, n_episodes=64, device=dev)
            else:
                tune_levels(env_cls, n_episodes=64, population=256, iterations=1, device=dev)
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        t = sorted(t[1:])                      # the first call warms up (library handles, allocator)
        print(json.dumps({"variant": variant, "launches": launches, "unit": "ms per call",
                          "median": t[len(t) // 2], "min": t[0]}))
        return
    env = env_cls(N, device=dev, autoreset_mode="disabled")
    obs0, _ = env.reset(seed=11)
    met = torch.zeros((N, invsim.policies.metrics_dim(env)), dtype=torch.float64, device=dev)
    kw = {}
    if variant.startswith("constant"):
        agent = invsim.ConstantOrderAgent()
    else:
        lv = invsim.NetLevelsAgent.from_mean_demand(env).tensors(env)[0]
        if variant == "netlevels":
            agent = invsim.NetLevelsAgent(lv)
        else:
            agent = invsim.TorchPolicyAgent(torch_rule(env, lv))
            kw = dict(obs0=obs0)

    def launch():
        env.rollout_policy(agent, K, obs=False, rewards=False, metrics=met, **kw)

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
    print(json.dumps({"variant": variant, "n": N, "K": K, "launches": launches, "unit": "us per launch",
                      "median": us[len(us) // 2], "min": us[0], "reward_per_step": float(met[:, 0].sum() / met[:, 1].sum())}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=2, metavar=("TREE", "VARIANT"))
    ap.add_argument("--part", choices=sorted(PARTS), default="r")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--raw", default=None, help="append every child's JSON line to this file")
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.child[1], args.launches)
    variants = [v for v in PARTS[args.part] if "@parent" not in v or args.parent_tree]
    launches = min(args.launches, 4) if args.part == "t" else args.launches
    runs = 1 if args.part == "t" else args.runs
    res = {}
    for run in range(runs):
        for v in variants:
            tree = args.parent_tree if "@parent" in v else ROOT
            cmd = [sys.executable, os.path.abspath(__file__), "--launches", str(launches), "--child", tree, v]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT_S)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                sys.exit(f"{v}: child exit {p.returncode}; stopping")
            line = p.stdout.strip().splitlines()[-1]
            if args.raw:
                with open(args.raw, "a") as f:
                    f.write(line + "\n")
            res.setdefault(v, []).append(json.loads(line)["median"])
    unit = {"r": f"us per {K}-step launch at {N} envs (HIP events), the median of each run's launches, per run",
            "t": "ms per call (wall clock, synchronised), median of the calls after the first"}[args.part]
    print(unit + "\n")
    print("| variant | " + " | ".join(f"run {i + 1}" for i in range(runs)) + " | median |")
    print("|---|" + "---|" * (runs + 1))
    for v in variants:
        s = sorted(res[v])
        print(f"| {v} | " + " | ".join(f"{x:.2f}" for x in res[v]) + f" | {s[len(s) // 2]:.2f} |")


if __name__ == "__main__":
    main()
