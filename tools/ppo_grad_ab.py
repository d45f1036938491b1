"""Timing of the PPO gradient calls against torch autograd of the same loss, on
one MI355X: 65 536 InvMgmt Backlog envs, K = 30 (1 966 080 samples), the
33-64-64-3 tanh actor and the 33-64-64-1 tanh critic, input rows from a
Normalizer.  Five runs; inside every run the variants alternate; HIP events
around every window; a variant's figure is the median window over the runs.

  grad-actor / grad-critic   ppo_actor_grad / value_grad on a minibatch of 4 096, 65 536 and all samples
                             (a random index tensor; obs read in place through it)
  torch-actor / torch-critic float32 autograd of the same loss on the same minibatch: gather of the
                             int64 rows from the [K + 1, N, O] block, cast, input affine, forward, loss
                             head, backward; the one-off cat([obs0, obs]) is timed on its own
  update                     PPOLearner.update: n_epochs = 2, batch_size = 65 536 (60 minibatches)
  update-torch               the same loop in torch: randperm, gather + cast, both losses, backward,
                             clip_grad_norm_, fused Adam; its cat included once per update

  python tools/ppo_grad_ab.py [--runs 5] > profiles/ppo_grad/table.md

Work per sample: 2 flops per weight forward and 4 backward, so 6 x (weights of
the network) x rows per call; the share of the float32 vector peak (157.3
TFLOP/s) is that over the time."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "or-gym-inventory_amd"))
N, K = 65536, 30
BATCHES = (4096, 65536, N * K)
PEAK = 157.3e12
LOG_SQRT_2PI = 0.9189385332046727


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    import torch

    import invsim
    from invsim.policies import (GaussianMLPPolicyAgent, Normalizer, PPOLearner, ValueMLP, collect_rollout,
                                 ppo_actor_grad, value_grad)
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    nn = torch.nn
    actor = nn.Sequential(nn.Linear(33, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 3)).to(dev)
    critic = nn.Sequential(nn.Linear(33, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 1)).to(dev)
    high = torch.tensor([100.0, 200.0, 230.0])
    log_std = nn.Parameter((0.2 * high).log().to(dev))
    ones, zeros = torch.ones(33), torch.zeros(33)
    osc, osh = (0.25 * high).to(dev), (0.5 * high).to(dev)
    env = invsim.InvManagementBacklogEnv(N, device=dev)
    obs0, _ = env.reset(seed=0)
    pi = GaussianMLPPolicyAgent.from_module(actor, log_std=log_std, seed=0, in_scale=ones, in_shift=zeros,
                                            out_scale=osc.cpu(), out_shift=osh.cpu())
    vf = ValueMLP.from_module(critic, in_scale=ones, in_shift=zeros)
    norm = Normalizer(env).observe(obs0)
    buf = collect_rollout(env, pi, K, obs0, critic=vf, normalize=norm)
    scale, shift = buf["obs_scale"], buf["obs_shift"]
    S = N * K
    adv_rms = invsim.RunningMoments(1, dev)
    adv_rms.stats.zero_()
    adv_rms.update(buf["advantages"], mask=buf["valid"])
    stats = adv_rms.stats
    valid = buf["valid"].reshape(-1)
    raw, old, adv, ret = (buf["raw_actions"].reshape(S, 3), buf["log_prob"].reshape(-1), buf["advantages"].reshape(-1),
                          buf["returns"].reshape(-1))
    mean_a, sd_a = stats[1, 0].float(), (stats[2, 0] / (stats[0, 0] - 1)).sqrt().float() + 1e-8

    def t_inputs(allobs, idx):
        return torch.addcmul(shift, allobs[idx].float(), scale)

    def t_actor_loss(allobs, idx):
        keep = valid[idx]
        n = keep.sum()
        mean = actor(t_inputs(allobs, idx)) * osc + osh
        z = (raw[idx] - mean) / log_std.exp()
        logp = -LOG_SQRT_2PI * 3 - (0.5 * z * z + log_std).sum(-1)
        ratio = (logp - old[idx]).exp()
        a = (adv[idx] - mean_a) / sd_a
        per = -torch.min(a * ratio, a * ratio.clamp(0.8, 1.2))
        return torch.where(keep, per, torch.zeros_like(per)).sum() / n

    def t_critic_loss(allobs, idx):
        keep = valid[idx]
        v = critic(t_inputs(allobs, idx))[:, 0]
        per = (ret[idx] - v) ** 2
        return 0.5 * torch.where(keep, per, torch.zeros_like(per)).sum() / keep.sum()

    params = list(actor.parameters()) + list(critic.parameters()) + [log_std]
    allobs = torch.cat([obs0[None], buf["obs"][:-1]]).reshape(S, 33)

    def window(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / reps          # us per call

    variants = {}
    gen = torch.Generator(device=dev).manual_seed(1)
    for rows in BATCHES:
        idx = torch.randperm(S, device=dev, generator=gen)[:rows].contiguous()
        reps = 50 if rows <= 65536 else 5
        ga = ppo_actor_grad(env, pi, buf, obs0, idx, adv_stats=stats)
        gc = value_grad(env, vf, buf, obs0, idx)
        ho_a, ho_c = invsim.policies._PPOGrads(pi, dev, log_std=True), invsim.policies._PPOGrads(vf, dev)
        del ga, gc

        def lib_a(idx=idx, ho=ho_a):
            ppo_actor_grad(env, pi, buf, obs0, idx, adv_stats=stats, out=ho)

        def lib_c(idx=idx, ho=ho_c):
            value_grad(env, vf, buf, obs0, idx, out=ho)

        def tor_a(idx=idx):
            torch.autograd.grad(t_actor_loss(allobs, idx), list(actor.parameters()) + [log_std])

        def tor_c(idx=idx):
            torch.autograd.grad(t_critic_loss(allobs, idx), list(critic.parameters()))
        variants[f"grad-actor {rows}"] = (lib_a, reps, rows, 33 * 64 + 64 * 64 + 64 * 3)
        variants[f"torch-actor {rows}"] = (tor_a, reps, rows, 33 * 64 + 64 * 64 + 64 * 3)
        variants[f"grad-critic {rows}"] = (lib_c, reps, rows, 33 * 64 + 64 * 64 + 64)
        variants[f"torch-critic {rows}"] = (tor_c, reps, rows, 33 * 64 + 64 * 64 + 64)
    variants["cat([obs0, obs[:-1]])"] = (lambda: torch.cat([obs0[None], buf["obs"][:-1]]), 5, 0, 0)

    EPOCHS, BATCH = 2, 65536
    learner = PPOLearner(env, pi, vf, actor, critic, log_std, n_epochs=EPOCHS, batch_size=BATCH)
    t_opt = torch.optim.Adam(params, lr=3e-4, eps=1e-5, fused=True)

    def torch_update():
        ao = torch.cat([obs0[None], buf["obs"][:-1]]).reshape(S, 33)
        for _ in range(EPOCHS):
            perm = torch.randperm(S, device=dev)
            for lo in range(0, S, BATCH):
                idx = perm[lo:lo + BATCH]
                t_opt.zero_grad(set_to_none=True)
                (t_actor_loss(ao, idx) + t_critic_loss(ao, idx)).backward()
                torch.nn.utils.clip_grad_norm_(params, 0.5, foreach=True)
                t_opt.step()

    def lib_update():
        learner.update(buf, obs0)
    # the two updates move the same parameters: each window starts from wherever the last one ended, which
    # changes no shape and no launch
    variants["update"] = (lib_update, 1, 0, 0)
    variants["update-torch"] = (torch_update, 1, 0, 0)

    for fn, *_ in variants.values():          # warm every shape
        fn()
    torch.cuda.synchronize()
    # torch_update sets .grad to fresh tensors: alias the learner's again before its windows
    def realias():
        for g, net, mod in ((learner._ga, pi, actor), (learner._gc, vf, critic)):
            for l, (w, b) in enumerate(net._module_params(mod)):
                w.grad, b.grad = g.weight[l], g.bias[l]
        log_std.grad = learner._ga.log_std
    times = {k: [] for k in variants}
    for _ in range(args.runs):
        for k, (fn, reps, _, _) in variants.items():
            if k == "update":
                realias()
            times[k].append(window(fn, reps))
    print("| variant | rows | median us | min .. max us | GFLOP/s | share of f32 vector peak |")
    print("|---|---|---|---|---|---|")
    for k, (fn, reps, rows, weights) in variants.items():
        t = times[k]
        med = statistics.median(t)
        fl = 6.0 * weights * rows / (med * 1e-6) if rows else 0.0
        print(f"| {k.split()[0]} | {rows or ''} | {med:.1f} | {min(t):.1f} .. {max(t):.1f} | "
              f"{fl / 1e9:.0f} | {100 * fl / PEAK:.2f} % |" if rows else
              f"| {k} | | {med:.1f} | {min(t):.1f} .. {max(t):.1f} | | |")
    print(f"\n{args.runs} runs, variants alternating inside each; update: {EPOCHS} epochs x {-(-S // BATCH)} minibatches "
          f"of {BATCH}.")
    env.close()


if __name__ == "__main__":
    main()
