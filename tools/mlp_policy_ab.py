"""Timing of the in-library MLP actor (every variant in a fresh child process
under its own time limit, several runs with the variants alternating inside
every run).

  part eval   evaluate_agent, 65 536 InvMgmt Backlog episodes of 30 steps, the same
              33-64-64-3 tanh actor (squashed and rescaled to the action range) both
              ways, us per evaluation (the function's own Time column x episodes,
              the first call of a process dropped):
                mlp-agent     MLPPolicyAgent: invsim_rollout_mlp, two launches per step
                torch-actor   TorchPolicyAgent around the torch module (the parent's path)
  part split  the new path taken apart, HIP events around 30 calls / steps from a
              reset, us per step:
                loop          invsim_rollout_mlp, K = 30, metrics only
                mlp-launch    invsim_mlp_actions alone, 30 launches
                env-launch    invsim_rollout_metrics of one row, metrics only, 30 calls
  part mlp    invsim_mlp_actions alone at 65 536 envs (InvMgmt Backlog: 33 int64
              observations, 3 int64 actions), ReLU hidden layers [64, 64] and
              [256, 256]: us per launch (HIP events around 200 launches) and the
              achieved FMA/s = N x sum(dims[l] x dims[l + 1]) / time

  python tools/mlp_policy_ab.py --part eval|split|mlp [--runs 5] [--raw FILE] > part.md

INVSIM_LIB selects another build of the library, as everywhere.  A child that
fails or runs out of time ends the whole measurement: nothing more is started
on the GPU after it.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "or-gym-inventory_amd"))
N, K = 65536, 30
CLS = "InvManagementBacklogEnv"
PARTS = {
    "eval": ["mlp-agent", "torch-actor"],
    "split": ["loop", "mlp-launch", "env-launch"],
    "mlp": ["64x64", "256x256"],
}
CHILD_LIMIT_S = 150


def _actor(dev):
    """the 33-64-64-3 tanh actor of profiles/external_policy/table.md (c) as a torch
    module and as the same network handed to the library"""
    import numpy as np
    import torch
    import invsim
    torch.manual_seed(0)
    nn = torch.nn
    body = nn.Sequential(nn.Linear(33, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 3), nn.Tanh())
    high = np.array([100.0, 200.0, 230.0], np.float32)
    # high * (0.5 + 0.6 * tanh): out_scale = 0.6 high, out_shift = 0.5 high; o * 0.01: in_scale
    mlp = invsim.MLPPolicyAgent.from_module(body, in_scale=np.full(33, 0.01, np.float32), in_shift=np.zeros(33, np.float32),
                                            out_scale=0.6 * high, out_shift=0.5 * high, name="Actor")
    body = body.to(dev)
    th = torch.as_tensor(high, device=dev)
    return mlp, invsim.TorchPolicyAgent(lambda o: th * (0.5 + 0.6 * body(o * 0.01)), name="Actor")


def _relu(widths, env):
    import numpy as np
    import invsim
    rng = np.random.default_rng(0)
    dims = [env.obs_dim] + widths + [env.action_dim]
    layers = [((rng.standard_normal((o, i)) / np.sqrt(i)).astype(np.float32), np.zeros(o, np.float32))
              for i, o in zip(dims[:-1], dims[1:])]
    return invsim.MLPPolicyAgent(layers, activation="relu", in_scale=np.full(dims[0], 0.01, np.float32),
                                 in_shift=np.zeros(dims[0], np.float32)), dims


def child(variant, launches):
    import torch
    import invsim
    dev = torch.device("cuda:0")
    if variant in PARTS["eval"]:
        mlp, tor = _actor(dev)
        agent = mlp if variant == "mlp-agent" else tor
        t = []
        for _ in range(launches):
            res = invsim.evaluate_agent(agent, getattr(invsim, CLS), {}, n_episodes=N, device=dev)
            t.append(float(res["Time"][0]) * 1e6 * N)      # Time is seconds per episode
        t = sorted(t[1:])                      # the first call warms up (library handles, allocator)
        print(json.dumps({"variant": variant, "n": N, "launches": launches, "unit": "us per evaluation",
                          "median_us": t[len(t) // 2], "min_us": t[0]}))
        return
    env = getattr(invsim, CLS)(N, device=dev)
    obs0, _ = env.reset(seed=11)
    lib, h = env._lib, env._h
    extra = {}
    if variant in PARTS["mlp"]:
        agent, dims = _relu([int(w) for w in variant.split("x")], env)
        per = 200
        extra["fma_per_launch"] = N * sum(a * b for a, b in zip(dims[:-1], dims[1:]))
    else:
        agent, per = _actor(dev)[0], K
    obj = agent.device_object(env)
    act = torch.empty((N, env.action_dim), dtype=env.act_dtype, device=dev)
    met = torch.zeros((N, invsim.policies.metrics_dim(env)), dtype=torch.float64, device=dev)
    s = env._stream()

    def launch():
        if variant == "loop":
            rc = lib.invsim_rollout_mlp(h, K, obj, obs0.data_ptr(), None, None, None, None, None, met.data_ptr(), s)
            assert rc == 0
        elif variant == "env-launch":
            for _ in range(K):
                env._rollout_metrics(1, act, None, None, None, None, met)
        else:
            for _ in range(per):
                assert lib.invsim_mlp_actions(h, obj, obs0.data_ptr(), act.data_ptr(), None, s) == 0

    lib.invsim_mlp_actions(h, obj, obs0.data_ptr(), act.data_ptr(), None, s)      # env-launch steps with these
    for _ in range(3):
        env.reset()
        launch()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for a, b in ev:
        env.reset()              # every timed window covers periods 0 .. K - 1
        a.record()
        launch()
        b.record()
    torch.cuda.synchronize()
    us = sorted(a.elapsed_time(b) * 1e3 / per for a, b in ev)
    out = {"variant": variant, "n": N, "launches": launches, "per_window": per, "unit": "us per step / launch",
           "median_us": us[len(us) // 2], "min_us": us[0]}
    if extra:
        out["gfma_per_s"] = extra["fma_per_launch"] / out["median_us"] * 1e-3
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", metavar="VARIANT")
    ap.add_argument("--part", choices=sorted(PARTS), default="eval")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--raw", default=None, help="append every child's JSON line to this file")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.launches)
    variants = PARTS[args.part]
    launches = min(args.launches, 6) if args.part == "eval" else args.launches
    res, rate = {}, {}
    for run in range(args.runs):
        for v in variants:
            cmd = [sys.executable, os.path.abspath(__file__), "--launches", str(launches), "--child", v]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT_S)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                sys.exit(f"{v}: child exit {p.returncode}; stopping")
            line = p.stdout.strip().splitlines()[-1]
            if args.raw:
                with open(args.raw, "a") as f:
                    f.write(line + "\n")
            d = json.loads(line)
            res.setdefault(v, []).append(d["median_us"])
            if "gfma_per_s" in d:
                rate.setdefault(v, []).append(d["gfma_per_s"])
    unit = {"eval": "us per evaluation of all episodes (evaluate_agent's Time x episodes)",
            "split": "us per step (HIP events around 30 steps from a reset)",
            "mlp": "us per launch (HIP events around 200 launches)"}[args.part]
    print(f"{unit}, median of the windows of a run, min - max over {args.runs} runs\n")
    print(f"| env | N | " + " | ".join(variants) + " |")
    print("|---|---|" + "---|" * len(variants))
    print(f"| {CLS} | {N} | " + " | ".join(f"{min(res[v]):.2f} - {max(res[v]):.2f}" for v in variants) + " |")
    if rate:
        print(f"| G FMA/s | | " + " | ".join(f"{min(rate[v]):.0f} - {max(rate[v]):.0f}" for v in variants) + " |")
    if args.part == "eval":
        a, b = res["torch-actor"], res["mlp-agent"]
        print(f"\ntorch-actor / mlp-agent: {min(a) / max(b):.1f} - {max(a) / min(b):.1f}")


if __name__ == "__main__":
    main()
