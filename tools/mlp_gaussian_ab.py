"""Timing of the Gaussian MLP actor (every variant in a fresh child process
under its own time limit, several runs with the variants alternating inside
every run).  65 536 InvMgmt Backlog envs, the 33-64-64-3 tanh actor of
tools/mlp_policy_ab.py, HIP events around every window:

  det-parent   invsim_mlp_actions of the parent commit's build (--parent-tree), 200 launches
  det          invsim_mlp_actions of this build, 200 launches
  sample       invsim_mlp_sample (all four outputs), 200 launches
  collect      collect_rollout, K = 30 from a reset: one invsim_rollout_mlp_sample call
  torch-loop   the same collection as a Python loop: the network in torch,
               torch.randn noise, the log-probability in torch, convert_actions and a
               one-step invsim_rollout_metrics launch per step, into preallocated rows

  python tools/mlp_gaussian_ab.py --parent-tree DIR [--runs 5] [--raw FILE] > table.md

DIR holds the parent commit's or-gym-inventory_amd/ (package and built
library); the det-parent child imports invsim from there and nothing from this
tree.  Without --parent-tree that variant is left out.  A child that fails or
runs out of time ends the whole measurement: nothing more is started on the
GPU after it.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, K, PER = 65536, 30, 200
CLS = "InvManagementBacklogEnv"
VARIANTS = ["det-parent", "det", "sample", "collect", "torch-loop"]
CHILD_LIMIT_S = 150
HIGH = [100.0, 200.0, 230.0]
LOG_STD = [2.0, 2.5, 2.5]


def _body():
    import torch
    torch.manual_seed(0)
    nn = torch.nn
    return nn.Sequential(nn.Linear(33, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 3), nn.Tanh())


def _agent(invsim, gaussian):
    import numpy as np
    high = np.array(HIGH, np.float32)
    kw = dict(in_scale=np.full(33, 0.01, np.float32), in_shift=np.zeros(33, np.float32), out_scale=0.6 * high,
              out_shift=0.5 * high, name="Actor")
    if gaussian:
        return invsim.GaussianMLPPolicyAgent.from_module(_body(), log_std=np.array(LOG_STD, np.float32), seed=0, **kw)
    return invsim.MLPPolicyAgent.from_module(_body(), **kw)


def child(variant, launches, tree):
    sys.path.insert(0, os.path.join(tree, "or-gym-inventory_amd"))
    import torch
    import invsim
    assert os.path.abspath(invsim.__file__).startswith(os.path.abspath(tree)), invsim.__file__
    dev = torch.device("cuda:0")
    env = getattr(invsim, CLS)(N, device=dev)
    obs0, _ = env.reset(seed=11)
    lib, h, s = env._lib, env._h, env._stream()
    A = env.action_dim
    agent = _agent(invsim, variant in ("sample", "collect"))
    act = torch.empty((N, A), dtype=env.act_dtype, device=dev)
    per = PER if variant in ("det-parent", "det", "sample") else K
    if variant in ("det-parent", "det"):
        obj = agent.device_object(env)

        def launch():
            for _ in range(per):
                assert lib.invsim_mlp_actions(h, obj, obs0.data_ptr(), act.data_ptr(), None, s) == 0
    elif variant == "sample":
        obj = agent.device_object(env)
        raw, mean = (torch.empty((N, A), dtype=torch.float32, device=dev) for _ in range(2))
        lp = torch.empty(N, dtype=torch.float32, device=dev)

        def launch():
            for _ in range(per):
                assert lib.invsim_mlp_sample(h, obj, obs0.data_ptr(), act.data_ptr(), raw.data_ptr(), mean.data_ptr(),
                                             lp.data_ptr(), s) == 0
    elif variant == "collect":
        def launch():
            invsim.policies.collect_rollout(env, agent, K, obs0)
    else:
        body = _body().to(dev)
        th = torch.as_tensor(HIGH, device=dev)
        log_std = torch.as_tensor(LOG_STD, device=dev)
        std = log_std.exp()
        sp = env.single_action_space
        low, high = (torch.as_tensor(b.reshape(-1), device=dev) for b in (sp.low, sp.high))

        def launch():
            o = torch.empty((K, N, env.obs_dim), dtype=env.obs_dtype, device=dev)
            rew = torch.empty((K, N), dtype=torch.float64, device=dev)
            term, trunc = (torch.empty((K, N), dtype=torch.bool, device=dev) for _ in range(2))
            a_all = torch.empty((K, N, A), dtype=env.act_dtype, device=dev)
            r_all = torch.empty((K, N, A), dtype=torch.float32, device=dev)
            lp = torch.empty((K, N), dtype=torch.float32, device=dev)
            cur = obs0
            with torch.no_grad():
                for k in range(K):
                    mean = th * (0.5 + 0.6 * body(cur.to(torch.float32) * 0.01))
                    z = torch.randn_like(mean)
                    torch.addcmul(mean, std, z, out=r_all[k])
                    lp[k] = (-0.5 * z * z - log_std).sum(1) - 0.9189385332046727 * A
                    a_all[k] = invsim.policies.convert_actions(r_all[k], low, high, env.act_dtype)
                    env._rollout_metrics(1, a_all[k], o[k], rew[k], term[k], trunc[k], None)
                    cur = o[k]

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
    print(json.dumps({"variant": variant, "n": N, "launches": launches, "per_window": per,
                      "unit": "us per launch" if per == PER else "us per step",
                      "median_us": us[len(us) // 2], "min_us": us[0]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", metavar="VARIANT")
    ap.add_argument("--tree", default=ROOT, help="(child) the tree invsim is imported from")
    ap.add_argument("--parent-tree", default=None, help="the parent commit's tree, built")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--raw", default=None, help="append every child's JSON line to this file")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.launches, args.tree)
    variants = [v for v in VARIANTS if v != "det-parent" or args.parent_tree]
    res = {}
    for run in range(args.runs):
        for v in variants:
            tree = os.path.abspath(args.parent_tree) if v == "det-parent" else ROOT
            cmd = [sys.executable, os.path.abspath(__file__), "--launches", str(args.launches), "--child", v, "--tree", tree]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT_S)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                sys.exit(f"{v}: child exit {p.returncode}; stopping")
            line = p.stdout.strip().splitlines()[-1]
            if args.raw:
                with open(args.raw, "a") as f:
                    f.write(line + "\n")
            res.setdefault(v, []).append(json.loads(line)["median_us"])
    print(f"us per launch (det-parent, det, sample: HIP events around {PER} launches) or per step (collect, torch-loop: "
          f"around {K} steps from a reset), median of the windows of a run, min - max over {args.runs} runs\n")
    print("| env | N | " + " | ".join(variants) + " |")
    print("|---|---|" + "---|" * len(variants))
    print(f"| {CLS} | {N} | " + " | ".join(f"{min(res[v]):.2f} - {max(res[v]):.2f}" for v in variants) + " |")
    a, b = res["torch-loop"], res["collect"]
    print(f"\ntorch-loop / collect: {min(a) / max(b):.2f} - {max(a) / min(b):.2f}")
    a, b = res["sample"], res["det"]
    print(f"sample - det, us per launch: {min(a) - max(b):.2f} - {max(a) - min(b):.2f}")


if __name__ == "__main__":
    main()
