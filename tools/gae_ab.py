"""Timing of the critic, GAE and parameter-update calls (every variant in a
fresh child process under its own time limit, several runs with the variants
alternating inside every run, HIP events around every window; the median
window of a process is its figure).  65 536 InvMgmt Backlog envs, K = 30, the
33-64-64-3 tanh actor of tools/mlp_gaussian_ab.py and a 33-64-64-1 tanh critic:

  gae            invsim_gae, K = 30, n = 65 536, 200 launches per window
  gae-torch      the textbook reverse loop in torch (float64, the same three outputs), one loop per window
  copy           torch.Tensor.copy_ moving the same 23 B * K * n (half read, half written), 200 per window
  gae-1m, gae-torch-1m, copy-1m   the same at n = 1 048 576 (20 launches per window)
  gae-variants   (--variants DIR) every DIR/libgae_<rows>x<threads>.so of `make gae_variants`, side by
                 side in one process, alternating inside every window, at both sizes
  collect-parent collect_rollout of the parent commit's build (--parent-tree), us per step
  collect        collect_rollout of this build without a critic
  collect-critic collect_rollout(critic=ValueMLP): plus two value launches and the GAE launch
  collect-torch  the same buffer with a torch critic and the torch GAE loop
  update         update_from_module of the actor (with log_std) and of the critic: wall time of the call
                 and the stream wait that follows it; and the host time of the call with a
                 collect_rollout queued in front of it (a call that synchronised would take that long)
  recreate       the parent's only path to new weights: invsim_mlp_destroy, invsim_mlp_create,
                 invsim_mlp_set_gaussian from a module, synchronised wall time
  det-parent, det   invsim_mlp_actions of the parent's build and of this one, 200 launches per window

  python tools/gae_ab.py [--parent-tree DIR] [--variants DIR] [--runs 3] [--raw FILE] > table.md

A child that fails or runs out of time ends the whole measurement: nothing
more is started on the GPU after it.
"""
import argparse
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, N_BIG, K, PER, PER_BIG = 65536, 1048576, 30, 200, 20
BYTES = 23                    # per (k, env): 14 read (reward 8, value 4, flags 2), 9 written (4 + 4 + 1)
CLS = "InvManagementBacklogEnv"
VARIANTS = ["gae", "gae-torch", "copy", "gae-1m", "gae-torch-1m", "copy-1m", "gae-variants", "collect-parent", "collect",
            "collect-critic", "collect-torch", "update", "recreate", "det-parent", "det"]
CHILD_LIMIT_S = 150
HIGH = [100.0, 200.0, 230.0]
LOG_STD = [2.0, 2.5, 2.5]
GAMMA, LAM = 0.99, 0.95


def _body(out, tanh_out):
    import torch
    torch.manual_seed(out)
    nn = torch.nn
    mods = [nn.Linear(33, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, out)]
    return nn.Sequential(*mods, nn.Tanh()) if tanh_out else nn.Sequential(*mods)


def _actor(invsim):
    import numpy as np
    high = np.array(HIGH, np.float32)
    return invsim.GaussianMLPPolicyAgent.from_module(
        _body(3, True), log_std=np.array(LOG_STD, np.float32), seed=0, in_scale=np.full(33, 0.01, np.float32),
        in_shift=np.zeros(33, np.float32), out_scale=0.6 * high, out_shift=0.5 * high, name="Actor")


def _critic(invsim):
    import numpy as np
    return invsim.ValueMLP.from_module(_body(1, False), in_scale=np.full(33, 0.01, np.float32),
                                       in_shift=np.zeros(33, np.float32))


def _gae_inputs(torch, n, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    rew = (torch.rand((K, n), generator=g, device=dev, dtype=torch.float64) - 0.5) * 2e3
    tr = torch.zeros((K, n), dtype=torch.bool, device=dev)
    tr[K - 1] = True                      # periods = 30: the last row truncates
    te = torch.zeros((K, n), dtype=torch.bool, device=dev)
    v0 = torch.randn(n, generator=g, device=dev) * 50
    v = torch.randn((K, n), generator=g, device=dev) * 50
    return rew, te, tr, v0, v


def torch_gae(torch, rew, te, tr, v0, v, done0=None):
    """the textbook reverse loop (float64, NEXT_STEP reset rows masked): invsim_gae's three outputs"""
    Kk, n = rew.shape
    adv = torch.empty((Kk, n), dtype=torch.float32, device=rew.device)
    ret = torch.empty_like(adv)
    valid = torch.empty((Kk, n), dtype=torch.bool, device=rew.device)
    done = te | tr
    carry = torch.zeros(n, dtype=torch.float64, device=rew.device)
    for k in range(Kk - 1, -1, -1):
        prev = done[k - 1] if k else (done0 if done0 is not None else torch.zeros_like(done[0]))
        vp = (v[k - 1] if k else v0).double()
        delta = rew[k] + torch.where(te[k], 0.0, GAMMA * v[k].double()) - vp
        a = torch.where(done[k], delta, delta + GAMMA * LAM * carry)
        carry = torch.where(prev, 0.0, a)
        adv[k] = carry.float()
        ret[k] = torch.where(prev, vp, a + vp).float()
        valid[k] = ~prev
    return adv, ret, valid


def _windows(torch, launch, launches, before=None):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for a, b in ev:
        if before:
            before()
        a.record()
        launch()
        b.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) * 1e3 for a, b in ev)


def child(variant, launches, tree, variants_dir):
    sys.path.insert(0, os.path.join(tree, "or-gym-inventory_amd"))
    import torch
    import invsim
    from invsim import _capi
    assert os.path.abspath(invsim.__file__).startswith(os.path.abspath(tree)), invsim.__file__
    dev = torch.device("cuda:0")
    out = {"variant": variant, "launches": launches}

    def report(us, per, unit, **more):
        out.update(per_window=per, unit=unit, median_us=us[len(us) // 2] / per, min_us=us[0] / per, **more)
        print(json.dumps(out))

    big = variant.endswith("-1m")
    n, per = (N_BIG, PER_BIG) if big else (N, PER)
    base = variant[:-3] if big else variant
    if base in ("gae", "gae-torch", "copy", "gae-variants"):
        torch.cuda.set_device(dev)
        s = torch.cuda.current_stream(dev).cuda_stream
        if base == "gae-variants":
            import ctypes as C
            libs = {}
            for path in sorted(glob.glob(os.path.join(variants_dir, "libgae_*.so"))):
                f = C.CDLL(path).gae_variant_launch
                P = C.c_void_p
                f.argtypes = [P, P, P, P, P, P, C.c_int32, C.c_int64, C.c_double, C.c_double, P, P, P, P]
                libs[os.path.basename(path)[len("libgae_"):-3]] = f
            assert libs, f"no libgae_*.so in {variants_dir}"
            res = {}
            for nn, pp in ((N, PER), (N_BIG, PER_BIG)):
                rew, te, tr, v0, v = _gae_inputs(torch, nn, dev)
                adv, ret = (torch.empty((K, nn), dtype=torch.float32, device=dev) for _ in range(2))
                valid = torch.empty((K, nn), dtype=torch.bool, device=dev)
                want = None
                for name, f in libs.items():
                    def launch(f=f):
                        for _ in range(pp):
                            assert f(rew.data_ptr(), te.data_ptr(), tr.data_ptr(), None, v0.data_ptr(), v.data_ptr(), K, nn,
                                     GAMMA, LAM, adv.data_ptr(), ret.data_ptr(), valid.data_ptr(), s) == 0
                    launch()
                    torch.cuda.synchronize()
                    got = (adv.clone(), ret.clone(), valid.clone())
                    want = want or got
                    assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                           b.view(torch.int32) if b.dtype == torch.float32 else b)
                               for a, b in zip(got, want)), f"{name}: the variants must agree bit for bit"
                    res.setdefault(name, {})[nn] = launch
                us = {name: [] for name in libs}
                for _ in range(launches):              # alternate inside the process: one window each, in turn
                    for name in libs:
                        us[name] += _windows(torch, res[name][nn], 1)
                out.setdefault("variants", {})[str(nn)] = {name: sorted(u)[len(u) // 2] / pp for name, u in us.items()}
            out["unit"] = "us per launch"
            print(json.dumps(out))
            return
        rew, te, tr, v0, v = _gae_inputs(torch, n, dev)
        if base == "gae":
            lib = _capi.lib()
            adv, ret = (torch.empty((K, n), dtype=torch.float32, device=dev) for _ in range(2))
            valid = torch.empty((K, n), dtype=torch.bool, device=dev)
            ref = invsim.policies.gae(rew, te, tr, v0, v, GAMMA, LAM)
            tg = torch_gae(torch, rew, te, tr, v0, v)
            out["max_abs_diff_vs_torch_loop"] = float((ref["advantages"] - tg[0]).abs().max())
            assert torch.equal(ref["valid"], tg[2])

            def launch():
                for _ in range(per):
                    assert lib.invsim_gae(rew.data_ptr(), te.data_ptr(), tr.data_ptr(), None, v0.data_ptr(), v.data_ptr(), K, n,
                                          GAMMA, LAM, adv.data_ptr(), ret.data_ptr(), valid.data_ptr(), s) == 0
            unit = "us per launch"
        elif base == "gae-torch":
            per = 1

            def launch():
                torch_gae(torch, rew, te, tr, v0, v)
            unit = "us per loop"
        else:
            src = torch.empty(BYTES * K * n // 2, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)

            def launch():
                for _ in range(per):
                    dst.copy_(src)
            unit = "us per copy"
        for _ in range(3):
            launch()
        torch.cuda.synchronize()
        us = _windows(torch, launch, launches)
        report(us, per, unit, n=n, bytes=BYTES * K * n)
        return

    env = getattr(invsim, CLS)(N, device=dev)
    obs0, _ = env.reset(seed=11)
    lib, h, s = env._lib, env._h, env._stream()
    A = env.action_dim
    actor = _actor(invsim)
    if variant in ("det-parent", "det"):
        obj = actor.device_object(env)
        act = torch.empty((N, A), dtype=env.act_dtype, device=dev)

        def launch():
            for _ in range(PER):
                assert lib.invsim_mlp_actions(h, obj, obs0.data_ptr(), act.data_ptr(), None, s) == 0
        for _ in range(3):
            launch()
        torch.cuda.synchronize()
        return report(_windows(torch, launch, launches), PER, "us per launch", n=N)
    if variant.startswith("collect"):
        if variant == "collect-critic":
            critic = _critic(invsim)
            critic.device_object(env)

            def launch():
                invsim.policies.collect_rollout(env, actor, K, obs0, critic=critic, gamma=GAMMA, gae_lambda=LAM)
        elif variant == "collect-torch":
            net = _body(1, False).to(dev)

            def launch():
                o = invsim.policies.collect_rollout(env, actor, K, obs0)
                with torch.no_grad():
                    val = net(torch.cat([obs0[None], o["obs"]]).float() * 0.01).reshape(K + 1, N)
                torch_gae(torch, o["reward"], o["terminated"], o["truncated"], val[0], val[1:])
        else:
            def launch():
                invsim.policies.collect_rollout(env, actor, K, obs0)
        for _ in range(3):
            env.reset()
            launch()
        torch.cuda.synchronize()
        return report(_windows(torch, launch, launches, before=env.reset), K, "us per step", n=N)
    if variant in ("update", "recreate"):
        critic = _critic(invsim)
        a_mod, c_mod = _body(3, True).to(dev), _body(1, False).to(dev)
        ls = torch.tensor(LOG_STD, device=dev)
        actor.device_object(env), critic.device_object(env)

        def wall(fn, reps=launches):
            t = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                t.append((time.perf_counter() - t0) * 1e6)
            return sorted(t)[len(t) // 2]
        if variant == "update":
            fa = lambda: actor.update_from_module(env, a_mod, log_std=ls)  # noqa: E731
            fc = lambda: critic.update_from_module(env, c_mod)  # noqa: E731
            fa(), fc()
            out["actor_us"], out["critic_us"] = wall(fa), wall(fc)
            # the host time of the call behind a queued rollout, against the time that rollout takes
            host, queued = [], []
            for _ in range(launches):
                env.reset()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                invsim.policies.collect_rollout(env, actor, K, obs0)
                t1 = time.perf_counter()
                fa()
                t2 = time.perf_counter()
                torch.cuda.synchronize()
                t3 = time.perf_counter()
                host.append((t2 - t1) * 1e6), queued.append((t3 - t0) * 1e6)
            out["actor_host_us_behind_rollout"] = sorted(host)[len(host) // 2]
            out["rollout_and_update_us"] = sorted(queued)[len(queued) // 2]
        else:
            import numpy as np

            def recreate(make):
                cur = {}

                def fn():
                    old = cur.get("agent")
                    if old is not None:
                        obj = old._objs.pop(env)[1]
                        env._mlps.remove(obj)
                        lib.invsim_mlp_destroy(obj)
                    new = make()                          # the module's parameters come to the host here
                    if hasattr(new, "_bufs"):
                        new._bufs[env] = env._arng        # keep the action generators: no re-seeding in the figure
                    new.device_object(env)
                    cur["agent"] = new
                return fn
            kw = dict(in_scale=np.full(33, 0.01, np.float32), in_shift=np.zeros(33, np.float32))
            ra = recreate(lambda: invsim.GaussianMLPPolicyAgent.from_module(
                a_mod, log_std=np.array(LOG_STD, np.float32), seed=0, **kw))
            rc = recreate(lambda: invsim.ValueMLP.from_module(c_mod, **kw))
            ra(), rc()
            out["actor_us"], out["critic_us"] = wall(ra), wall(rc)
        out["unit"] = "us per call, host wall clock, synchronised"
        print(json.dumps(out))
        return
    raise SystemExit(f"unknown variant {variant}")


def _rng(v, fmt="{:.2f}"):
    return f"{fmt.format(min(v))} - {fmt.format(max(v))}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", metavar="VARIANT")
    ap.add_argument("--tree", default=ROOT, help="(child) the tree invsim is imported from")
    ap.add_argument("--parent-tree", default=None, help="the parent commit's tree, built")
    ap.add_argument("--variants", default=None, help="directory of libgae_<rows>x<threads>.so (make gae_variants)")
    ap.add_argument("--only", default=None, help="comma-separated variants to run")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--raw", default=None, help="append every child's JSON line to this file")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.launches, args.tree, args.variants)
    variants = [v for v in VARIANTS if (args.parent_tree or not v.endswith("-parent")) and (args.variants or v != "gae-variants")]
    if args.only:
        variants = [v for v in variants if v in args.only.split(",")]
    res = {}
    for run in range(args.runs):
        for v in variants:
            tree = os.path.abspath(args.parent_tree) if v.endswith("-parent") else ROOT
            cmd = [sys.executable, os.path.abspath(__file__), "--launches", str(args.launches), "--child", v, "--tree", tree]
            if args.variants:
                cmd += ["--variants", os.path.abspath(args.variants)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT_S)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                sys.exit(f"{v}: child exit {p.returncode}; stopping")
            line = p.stdout.strip().splitlines()[-1]
            if args.raw:
                with open(args.raw, "a") as f:
                    f.write(line + "\n")
            res.setdefault(v, []).append(json.loads(line))
            sys.stderr.write(f"run {run} {v} done\n")
    med = lambda v: [r["median_us"] for r in res[v]]  # noqa: E731
    print(f"{CLS}, K = {K}; HIP events around every window, the median window of a process is its figure, "
          f"min - max over {args.runs} runs (one fresh process per variant and run, alternating)\n")
    for tag, n, names in (("", N, ("gae", "gae-torch", "copy")), ("-1m", N_BIG, ("gae-1m", "gae-torch-1m", "copy-1m"))):
        if not all(x in res for x in names):
            continue
        g, t, c = (med(x) for x in names)
        tot = BYTES * K * n
        print(f"### GAE, n = {n} ({tot / 1e6:.1f} MB per launch at {BYTES} B per (k, env))\n")
        print("| invsim_gae, us per launch | torch reverse loop, us per loop | copy_ of the same bytes, us |")
        print("|---|---|---|")
        print(f"| {_rng(g)} | {_rng(t)} | {_rng(c)} |\n")
        print(f"torch loop / invsim_gae: {min(t) / max(g):.1f} - {max(t) / min(g):.1f}")
        print(f"invsim_gae: {tot / max(g) / 1e6:.2f} - {tot / min(g) / 1e6:.2f} TB/s; copy_: "
              f"{tot / max(c) / 1e6:.2f} - {tot / min(c) / 1e6:.2f} TB/s; ratio {min(c) / max(g):.2f} - {max(c) / min(g):.2f}\n")
    if "gae-variants" in res:
        print("### GAE kernel variants (rows per block x threads per workgroup), us per launch, one process, alternating\n")
        for nn in (str(N), str(N_BIG)):
            names = sorted(res["gae-variants"][0]["variants"][nn], key=lambda s: tuple(int(x) for x in s.split("x"))[::-1])
            print(f"n = {nn}\n\n| " + " | ".join(names) + " |\n|" + "---|" * len(names))
            print("| " + " | ".join(_rng([r["variants"][nn][x] for r in res["gae-variants"]]) for x in names) + " |\n")
    names = [v for v in ("collect-parent", "collect", "collect-critic", "collect-torch") if v in res]
    if names:
        print(f"### Collection, us per step (K = {K} from a reset)\n\n| " + " | ".join(names) + " |\n|" + "---|" * len(names))
        print("| " + " | ".join(_rng(med(v)) for v in names) + " |\n")
        if "collect-critic" in res and "collect" in res:
            a, b = med("collect-critic"), med("collect")
            print(f"collect-critic - collect, us per step: {min(a) - max(b):.2f} - {max(a) - min(b):.2f}")
        if "collect-torch" in res and "collect-critic" in res:
            a, b = med("collect-torch"), med("collect-critic")
            print(f"collect-torch / collect-critic: {min(a) / max(b):.2f} - {max(a) / min(b):.2f}\n")
    if "update" in res and "recreate" in res:
        u, r = res["update"], res["recreate"]
        print("### New weights, us per call (host wall clock around the call and a device synchronise)\n")
        print("| | update_from_module | destroy + create + set_gaussian |\n|---|---|---|")
        for k, name in (("actor_us", "actor (with log_std)"), ("critic_us", "critic")):
            print(f"| {name} | {_rng([x[k] for x in u], '{:.0f}')} | {_rng([x[k] for x in r], '{:.0f}')} |")
        print(f"\nHost time of the actor's update_from_module with a K = {K} collect_rollout queued in front of it: "
              f"{_rng([x['actor_host_us_behind_rollout'] for x in u], '{:.0f}')} us; that rollout and the update take "
              f"{_rng([x['rollout_and_update_us'] for x in u], '{:.0f}')} us until the device is idle.\n")
    names = [v for v in ("det-parent", "det") if v in res]
    if names:
        print("### invsim_mlp_actions, us per launch\n\n| " + " | ".join(names) + " |\n|" + "---|" * len(names))
        print("| " + " | ".join(_rng(med(v)) for v in names) + " |")


if __name__ == "__main__":
    main()
