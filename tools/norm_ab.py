"""Timing of the running-normalisation calls (every group of variants in a
fresh child process under its own time limit, several runs, the variants of a
group alternating window by window inside the process, HIP events around every
window; the median window of a process is its figure):

  moments        invsim_moments over [30 x 65 536][33] int64 and [30 x 32 768][68] float32, against torch's
                 cast to float64 + mean + var over the rows and a copy_ of the same bytes (the streaming bound:
                 copy_ reads and writes, so it moves twice the bytes the reduction reads)
  moments-1m     the same at 1 048 576 envs ([30 x 1 048 576][33] int64, [30 x 1 048 576][68] float32)
  returns        invsim_discounted_returns + invsim_normalize_rewards over [30][65 536], against the torch loop
  collect        collect_rollout(critic=ValueMLP) without normalize, with it, and without it but with the same
                 statistics kept on the torch side (cast, mean, var, the returns loop), us per step
  det-parent, det   invsim_mlp_actions of the parent commit's build (--parent-tree) and of this one

  python tools/norm_ab.py [--parent-tree DIR] [--runs 5] [--raw FILE] > table.md

A child that fails or runs out of time ends the whole measurement: nothing
more is started on the GPU after it.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
N, N_BIG, K = 65536, 1048576, 30
SHAPES = {"i64x33": ("int64", N, 33, 8), "f32x68": ("float32", N // 2, 68, 4)}
GROUPS = ["moments", "moments-1m", "returns", "collect", "det-parent", "det"]
CHILD_LIMIT_S = 170
GAMMA, EPS, CLIP = 0.99, 1e-8, 10.0


def _window(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3


def _alternate(torch, fns, windows, warm=2):
    """{name: median us per window}, one window of each variant in turn"""
    for _ in range(warm):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(windows):
        for k, f in fns.items():
            us[k].append(_window(torch, f))
    return {k: sorted(v)[len(v) // 2] for k, v in us.items()}


def torch_returns(torch, rew, te, tr, ret, var):
    """VecNormalize's per-step rule in torch: returns, their valid mask, the normalised rewards"""
    Kk, n = rew.shape
    out = torch.empty_like(rew)
    done = te | tr
    prev = torch.zeros_like(done[0])
    for k in range(Kk):
        new = ret * GAMMA + rew[k]
        out[k] = torch.where(prev, 0.0, new)
        ret = torch.where(prev | done[k], 0.0, new)
        prev = done[k]
    return out, torch.clamp(rew / torch.sqrt(var + EPS), -CLIP, CLIP), ret


def child(group, windows, tree):
    sys.path.insert(0, os.path.join(tree, "or-gym-inventory_amd"))
    import torch
    import invsim
    from invsim import _capi
    assert os.path.abspath(invsim.__file__).startswith(os.path.abspath(tree)), invsim.__file__
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    out = {"group": group, "windows": windows}
    if group in ("moments", "moments-1m"):
        big = group.endswith("-1m")
        per = 2 if big else 20
        for name, (dt, n, cols, esz) in SHAPES.items():
            n = N_BIG if big else n
            rows = K * n
            g = torch.Generator(device=dev).manual_seed(0)
            if dt == "int64":
                x = torch.randint(0, 400, (rows, cols), device=dev, generator=g)
            else:
                x = torch.rand((rows, cols), device=dev, generator=g) * 400
            rm = invsim.RunningMoments(cols, dev).update(x)
            ref_mean, ref_var = x.double().mean(0), x.double().var(0, unbiased=False)
            torch.cuda.synchronize()
            out[f"{name}_rel_mean_diff_vs_torch"] = float(((rm.mean - ref_mean).abs() / ref_mean.abs()).max())
            out[f"{name}_rel_var_diff_vs_torch"] = float(((rm.var - ref_var).abs() / ref_var).max())
            del ref_mean, ref_var
            dst = torch.empty_like(x)

            def f_mom(x=x, rm=rm):
                for _ in range(per):
                    rm.update(x)

            def f_torch(x=x):
                for _ in range(per):
                    xd = x.double()
                    xd.mean(0), xd.var(0, unbiased=False)

            def f_copy(x=x, dst=dst):
                for _ in range(per):
                    dst.copy_(x)
            us = _alternate(torch, {"moments": f_mom, "torch": f_torch, "copy": f_copy}, windows)
            out[name] = {k: v / per for k, v in us.items()}
            out[name]["bytes"] = rows * cols * esz
            del x, dst, rm
            torch.cuda.empty_cache()
        print(json.dumps(out))
        return
    if group == "returns":
        from invsim import policies
        per = 50
        g = torch.Generator(device=dev).manual_seed(0)
        rew = (torch.rand((K, N), generator=g, device=dev, dtype=torch.float64) - 0.5) * 2e3
        te = torch.zeros((K, N), dtype=torch.bool, device=dev)
        tr = torch.zeros_like(te)
        tr[K - 1] = True
        ret = torch.zeros(N, dtype=torch.float64, device=dev)
        stats = torch.tensor([[1e4], [0.0], [1e4 * 250.0 ** 2]], dtype=torch.float64, device=dev)
        var = stats[2, 0] / stats[0, 0]

        def f_lib():
            for _ in range(per):
                policies.discounted_returns(rew, te, tr, ret, GAMMA)
                policies.normalize_rewards(rew, stats, EPS, CLIP)

        def f_torch():
            torch_returns(torch, rew, te, tr, ret, var)
        us = _alternate(torch, {"lib": f_lib, "torch": f_torch}, windows)
        out["returns"] = {"lib": us["lib"] / per, "torch": us["torch"]}
        print(json.dumps(out))
        return
    import gae_ab
    env = getattr(invsim, gae_ab.CLS)(N, device=dev)
    obs0, _ = env.reset(seed=11)
    actor = gae_ab._actor(invsim)
    if group in ("det-parent", "det"):
        lib, h, s = env._lib, env._h, env._stream()
        obj = actor.device_object(env)
        act = torch.empty((N, env.action_dim), dtype=env.act_dtype, device=dev)

        def launch():
            for _ in range(200):
                assert lib.invsim_mlp_actions(h, obj, obs0.data_ptr(), act.data_ptr(), None, s) == 0
        us = _alternate(torch, {"det": launch}, windows)
        out["det"] = us["det"] / 200
        print(json.dumps(out))
        return
    if group == "collect":
        from invsim import policies
        critic = gae_ab._critic(invsim)
        critic.device_object(env)
        norm = invsim.Normalizer(env, gamma=GAMMA)
        keep = {"ret": torch.zeros(N, dtype=torch.float64, device=dev)}

        def f_plain():
            env.reset()
            policies.collect_rollout(env, actor, K, obs0, critic=critic)

        def f_norm():
            env.reset()
            policies.collect_rollout(env, actor, K, obs0, critic=critic, normalize=norm)

        def f_torchnorm():
            env.reset()
            o = policies.collect_rollout(env, actor, K, obs0, critic=critic)
            xd = o["obs"].reshape(-1, env.obs_dim).double()
            xd.mean(0), xd.var(0, unbiased=False)
            dr, rn, keep["ret"] = torch_returns(torch, o["reward"], o["terminated"], o["truncated"], keep["ret"],
                                                torch.tensor(250.0 ** 2, dtype=torch.float64, device=dev))
            w = o["valid"].double()                              # the masked variance without a host round trip
            m = (dr * w).sum() / w.sum()
            (((dr - m) ** 2) * w).sum() / w.sum()
            policies.gae(rn, o["terminated"], o["truncated"], o["values"][0], torch.cat([o["values"][1:], o["last_value"][None]]))
        us = _alternate(torch, {"collect-critic": f_plain, "collect-normalize": f_norm, "collect-torch-normalize": f_torchnorm},
                        windows)
        out["collect"] = {k: v / K for k, v in us.items()}
        print(json.dumps(out))
        return
    raise SystemExit(f"unknown group {group}")


def _rng(v, fmt="{:.2f}"):
    return f"{fmt.format(min(v))} - {fmt.format(max(v))}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", metavar="GROUP")
    ap.add_argument("--tree", default=ROOT, help="(child) the tree invsim is imported from")
    ap.add_argument("--parent-tree", default=None, help="the parent commit's tree, built")
    ap.add_argument("--only", default=None, help="comma-separated groups to run")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--raw", default=None, help="append every child's JSON line to this file")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.windows, args.tree)
    groups = [g for g in GROUPS if args.parent_tree or g != "det-parent"]
    if args.only:
        groups = [g for g in groups if g in args.only.split(",")]
    res = {}
    for run in range(args.runs):
        for g in groups:
            tree = os.path.abspath(args.parent_tree) if g == "det-parent" else ROOT
            cmd = [sys.executable, os.path.abspath(__file__), "--windows", str(args.windows), "--child", g, "--tree", tree]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT_S)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                sys.exit(f"{g}: child exit {p.returncode}; stopping")
            line = p.stdout.strip().splitlines()[-1]
            if args.raw:
                with open(args.raw, "a") as f:
                    f.write(line + "\n")
            res.setdefault(g, []).append(json.loads(line))
            sys.stderr.write(f"run {run} {g} done\n")
    print(f"K = {K}; HIP events around every window, the median window of a process is its figure, min - max over "
          f"{args.runs} runs (one fresh process per group and run, the variants of a group alternating window by window)\n")
    for g, envs in (("moments", "65 536 / 32 768"), ("moments-1m", "1 048 576")):
        if g not in res:
            continue
        print(f"### invsim_moments, {envs} envs x K = {K} rows\n")
        print("| x | MB read | invsim_moments, us | torch cast + mean + var, us | copy_ of the same bytes, us | "
              "invsim_moments TB/s read | copy_ TB/s read + written | torch / invsim_moments |")
        print("|---|---|---|---|---|---|---|---|")
        for name in SHAPES:
            rows = [r[name] for r in res[g]]
            b = rows[0]["bytes"]
            m, t, c = ([r[k] for r in rows] for k in ("moments", "torch", "copy"))
            print(f"| {name} | {b / 1e6:.0f} | {_rng(m, '{:.1f}')} | {_rng(t, '{:.1f}')} | {_rng(c, '{:.1f}')} | "
                  f"{b / max(m) / 1e6:.2f} - {b / min(m) / 1e6:.2f} | {2 * b / max(c) / 1e6:.2f} - {2 * b / min(c) / 1e6:.2f} | "
                  f"{min(t) / max(m):.1f} - {max(t) / min(m):.1f} |")
        print()
        for name in SHAPES:
            print(f"{name}: largest relative difference from torch's float64 mean / var: "
                  f"{max(r[name + '_rel_mean_diff_vs_torch'] for r in res[g]):.2e} / "
                  f"{max(r[name + '_rel_var_diff_vs_torch'] for r in res[g]):.2e}\n")
    if "returns" in res:
        a, b = ([r["returns"][k] for r in res["returns"]] for k in ("lib", "torch"))
        print(f"### invsim_discounted_returns + invsim_normalize_rewards, [{K}][{N}]\n")
        print("| the two launches, us | torch loop, us | ratio |\n|---|---|---|")
        print(f"| {_rng(a)} | {_rng(b)} | {min(b) / max(a):.1f} - {max(b) / min(a):.1f} |\n")
    if "collect" in res:
        names = list(res["collect"][0]["collect"])
        print(f"### collect_rollout(critic=ValueMLP), {N} envs, us per step (K = {K} from a reset)\n")
        print("| " + " | ".join(names) + " |\n|" + "---|" * len(names))
        print("| " + " | ".join(_rng([r["collect"][k] for r in res["collect"]]) for k in names) + " |\n")
    names = [g for g in ("det-parent", "det") if g in res]
    if names:
        print("### invsim_mlp_actions, us per launch\n\n| " + " | ".join(names) + " |\n|" + "---|" * len(names))
        print("| " + " | ".join(_rng([r["det"] for r in res[g]]) for g in names) + " |")


if __name__ == "__main__":
    main()
