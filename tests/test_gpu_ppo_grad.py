"""GPU: invsim_ppo_actor_grad / invsim_value_grad and PPOLearner against the
float64 torch.autograd reference of tests/ppo_reference.py, on the cases and at
the tolerance (GRAD_TOL, 4 x torch's own float32 autograd error) stated there."""
import ctypes as C

import numpy as np
import pytest
import torch

import ppo_reference as pr
from test_gpu_gae import _cls_kw

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
EINVAL, ERANGE = -22, -34
SEED = 400


def _dev(gpu, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _env(gpu, family, n=4):
    cls, kw = _cls_kw(family)
    env = cls(n, device=gpu, **kw)
    obs0, _ = env.reset(seed=SEED)
    return env, obs0


def _agents(case):
    import invsim
    aff = {} if case["in_scale"] is None else dict(in_scale=case["in_scale"], in_shift=case["in_shift"])
    a_out = {} if case["out_scale"] is None else dict(out_scale=case["out_scale"], out_shift=case["out_shift"])
    v_out = {} if case["v_scale"] is None else dict(out_scale=case["v_scale"], out_shift=case["v_shift"])
    pi = invsim.GaussianMLPPolicyAgent.from_module(case["actor"], log_std=case["log_std"], seed=0, clip=False,
                                                   **aff, **a_out)
    vf = invsim.ValueMLP.from_module(case["critic"], **aff, **v_out)
    return pi, vf


def _buf(gpu, case, **over):
    c = dict(case, **over)
    buf = {"obs": _dev(gpu, c["obs"]), "raw_actions": _dev(gpu, c["raw"]), "log_prob": _dev(gpu, c["old_logp"]),
           "advantages": _dev(gpu, c["adv"]), "returns": _dev(gpu, c["returns"])}
    if c["valid"] is not None:
        buf["valid"] = _dev(gpu, c["valid"])
    return buf, _dev(gpu, c["obs0"]), _dev(gpu, c["idx"]), _dev(gpu, c["adv_stats"])


def _host(g):
    """a wrapper's result as float64 numpy, in the reference's structure"""
    out = {k: [t.detach().cpu().double().numpy() for t in g[k]] for k in ("weight", "bias")}
    out["stats"] = g["stats"].cpu().numpy().copy()
    if "log_std" in g:
        out["log_std"] = g["log_std"].cpu().double().numpy()
    return out


def _both(env, pi, vf, case, buf, obs0, idx, stats, clip_range=None):
    from invsim.policies import ppo_actor_grad, value_grad
    a = ppo_actor_grad(env, pi, buf, obs0, idx, case["clip_range"] if clip_range is None else clip_range,
                       case["ent_coef"], stats)
    c = value_grad(env, vf, buf, obs0, idx, case["vf_coef"])
    torch.cuda.synchronize(env.device)
    return {"actor": _host(a), "critic": _host(c)}


def _check(got, ref, what):
    worst = 0.0
    for net in ref:
        m = pr.compare(got[net], ref[net])
        print(f"{what} {net}: largest metric {m:.3e} = {m / pr.GRAD_TOL:.3f} of GRAD_TOL {pr.GRAD_TOL:.2e}")
        worst = max(worst, m)
    assert worst <= pr.GRAD_TOL, (what, worst)
    return worst


@pytest.mark.parametrize("name", list(pr.CASES))
def test_gradients_are_the_references(gpu, name):
    case, ref = pr.case_and_reference(name)
    env, _ = _env(gpu, case["family"])
    pi, vf = _agents(case)
    got = _both(env, pi, vf, case, *_buf(gpu, case))
    _check(got, ref, name)
    assert got["actor"]["stats"][0] == ref["actor"]["stats"][0] == got["critic"]["stats"][0]
    env.close()


def test_masked_samples_are_selected_out(gpu):
    """NaN in the masked samples' advantages / returns / raw actions and 2^62 in their
    observation rows reach no output: the result is that of the minibatch without them"""
    case, ref = pr.case_and_reference("im-64x64-rows63")
    bad = ~case["valid"]
    assert bad[case["idx"]].sum() >= 5
    adv, ret, raw = case["adv"].copy(), case["returns"].copy(), case["raw"].copy()
    adv[bad] = ret[bad] = raw[bad] = np.nan
    allobs = np.concatenate([case["obs0"], case["obs"]])
    allobs[:case["S"]][bad] = 2 ** 62
    n0 = case["n0"]
    env, _ = _env(gpu, "im")
    pi, vf = _agents(case)
    poisoned = _both(env, pi, vf, case, *_buf(gpu, case, adv=adv, returns=ret, raw=raw, obs0=allobs[:n0], obs=allobs[n0:]))
    for net in poisoned:
        for k, v in poisoned[net].items():
            assert all(np.isfinite(t).all() for t in (v if isinstance(v, list) else [v])), (net, k)
    kept = case["idx"][case["valid"][case["idx"]]]
    removed = _both(env, pi, vf, case, *_buf(gpu, case, idx=kept, valid=None))
    _check(poisoned, removed, "poisoned against removed")
    _check(poisoned, ref, "poisoned against the reference")
    # all masked: exact zeros
    none = np.flatnonzero(bad)[:7].astype(np.int64)
    zero = _both(env, pi, vf, case, *_buf(gpu, case, adv=adv, returns=ret, raw=raw, obs0=allobs[:n0], obs=allobs[n0:],
                                         idx=none))
    for net in zero:
        for k, v in zero[net].items():
            for t in (v if isinstance(v, list) else [v]):
                assert not np.any(t) and not np.signbit(t).any(), (net, k)
    env.close()


@pytest.mark.parametrize("name", ["im-two-tiles-per-group", "im-256x256-tanh", "net-64x64-tanh"])
def test_two_calls_give_the_same_bits(gpu, name):
    case, _ = pr.case_and_reference(name)
    env, _ = _env(gpu, case["family"])
    pi, vf = _agents(case)
    args = _buf(gpu, case)
    a, b = _both(env, pi, vf, case, *args), _both(env, pi, vf, case, *args)
    for net in a:
        for k, v in a[net].items():
            for x, y in zip(*((v, b[net][k]) if isinstance(v, list) else ([v], [b[net][k]]))):
                assert np.array_equal(x.view(np.int64), y.view(np.int64)), (net, k)
    env.close()


def test_a2c_is_the_same_call(gpu):
    """clip_range = +inf and old_logp = the current log-density: the gradient of -mean(adv * logp) - ent_coef * entropy"""
    case, _ = pr.case_and_reference("im-30x7-tanh")
    cur = pr.current_log_prob(case).astype(F32)
    ref = pr.grads(case, clip_range=float("inf"), old_logp=cur)
    env, _ = _env(gpu, "im")
    pi, vf = _agents(case)
    got = _both(env, pi, vf, case, *_buf(gpu, case, old_logp=cur), clip_range=float("inf"))
    _check(got, ref, "a2c")
    assert got["actor"]["stats"][4] == 0.0 and abs(got["actor"]["stats"][5] - 1.0) < 1e-5
    env.close()


def test_a_captured_call_follows_update_from_module(gpu):
    from invsim.policies import _PPOGrads, ppo_actor_grad, value_grad
    case, ref = pr.case_and_reference("im-64x64-seam")
    env, _ = _env(gpu, "im")
    pi, vf = _agents(case)
    buf, obs0, idx, stats = _buf(gpu, case)
    actor = pr.make_module([33, 64, 64, 3], "tanh", False, 10 * pr.CASES["im-64x64-seam"]["seed"]).to(gpu)
    critic = pr.make_module([33, 64, 64, 1], "tanh", False, 10 * pr.CASES["im-64x64-seam"]["seed"] + 1).to(gpu)
    log_std = _dev(gpu, case["log_std"])
    ga, gc = _PPOGrads(pi, gpu, log_std=True), _PPOGrads(vf, gpu)
    pi.update_from_module(env, actor, log_std=log_std)      # the first meeting and the scratch: before the capture
    vf.update_from_module(env, critic)
    ppo_actor_grad(env, pi, buf, obs0, idx, case["clip_range"], case["ent_coef"], stats, out=ga)
    value_grad(env, vf, buf, obs0, idx, case["vf_coef"], out=gc)

    def fn():
        pi.update_from_module(env, actor, log_std=log_std)
        vf.update_from_module(env, critic)
        ppo_actor_grad(env, pi, buf, obs0, idx, case["clip_range"], case["ent_coef"], stats, out=ga)
        value_grad(env, vf, buf, obs0, idx, case["vf_coef"], out=gc)
    g = env.capture(fn, warmup=1)
    for rep in range(2):
        if rep:         # an optimiser's step: new weights in the same tensors; the old log-densities stay
            with torch.no_grad():
                for p in list(actor.parameters()) + list(critic.parameters()):
                    p.mul_(0.9).add_(0.01)
                log_std.add_(0.05)
            new = dict(case, actor=pr.copy.deepcopy(actor).cpu(), critic=pr.copy.deepcopy(critic).cpu(),
                       log_std=log_std.cpu().numpy())
            ref = pr.grads(new)
        for t in ga.weight + ga.bias + gc.weight + gc.bias + [ga.log_std, ga.stats, gc.stats]:
            t.fill_(7.0)
        g.replay()
        torch.cuda.synchronize(gpu)
        _check({"actor": _host(ga.result()), "critic": _host(gc.result())}, ref, f"replay {rep}")
    env.close()


def test_every_refusal_is_decided_before_a_launch(gpu):
    import invsim
    case, _ = pr.case_and_reference("im-64x64-tanh")
    env, _ = _env(gpu, "im")
    other, _ = _env(gpu, "im")
    pi, vf = _agents(case)
    plain = invsim.MLPPolicyAgent.from_module(case["actor"], clip=False, in_scale=case["in_scale"],
                                              in_shift=case["in_shift"])
    buf, obs0, idx, stats = _buf(gpu, case)
    S, lib, h = case["S"], env._lib, env._h
    om, ov, op = pi.device_object(env), vf.device_object(env), plain.device_object(env)
    foreign = _agents(case)[0].device_object(other)
    need = invsim.policies.ppo_scratch_bytes(pi.dims, S)
    scratch = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device=gpu)
    gw = [torch.full(w.shape, 3.0, device=gpu) for w in pi.weights]
    gb = [torch.full((w.shape[0],), 3.0, device=gpu) for w in pi.weights]
    W = (C.c_void_p * 3)(*[t.data_ptr() for t in gw])
    B = (C.c_void_p * 3)(*[t.data_ptr() for t in gb])
    gls = torch.full((3,), 3.0, device=gpu)
    st = torch.full((6,), 3.0, dtype=torch.float64, device=gpu)
    p = lambda t: t.data_ptr()  # noqa: E731

    def actor(m=om, obs=p(buf["obs"]), rows=S, raw=p(buf["raw_actions"]), logp=p(buf["log_prob"]),
              adv=p(buf["advantages"]), clip=0.2, sc=p(scratch), nbytes=need, hh=h, n0=0):
        return lib.invsim_ppo_actor_grad(hh, m, None, n0, obs, None, rows, None, raw, logp, adv, None, clip, 0.0,
                                         C.cast(W, C.c_void_p), C.cast(B, C.c_void_p), p(gls), p(st), sc, nbytes,
                                         env._stream())

    def value(m=ov, obs=p(buf["obs"]), rows=S, ret=p(buf["returns"]), sc=p(scratch), nbytes=need, hh=h):
        return lib.invsim_value_grad(hh, m, None, 0, obs, None, rows, None, ret, 0.5, C.cast(W, C.c_void_p),
                                     C.cast(B, C.c_void_p), p(st), sc, nbytes, env._stream())
    refused = [
        (actor(m=ov), EINVAL), (value(m=om), EINVAL), (actor(m=op), EINVAL), (actor(m=foreign), EINVAL),
        (value(m=foreign), EINVAL), (actor(rows=-1), EINVAL), (value(rows=-1), EINVAL), (actor(obs=None), EINVAL),
        (actor(raw=None), EINVAL), (actor(logp=None), EINVAL), (actor(adv=None), EINVAL), (value(ret=None), EINVAL),
        (value(obs=None), EINVAL), (actor(clip=0.0), EINVAL), (actor(clip=-0.2), EINVAL), (actor(clip=float("nan")), EINVAL),
        (actor(sc=None), EINVAL), (value(sc=None), EINVAL), (actor(nbytes=need - 1), ERANGE),
        (value(nbytes=invsim.policies.ppo_scratch_bytes(vf.dims, S) - 1), ERANGE), (actor(n0=3), EINVAL),
        (actor(rows=0), 0), (value(rows=0), 0), (actor(rows=0, obs=None, raw=None, sc=None, nbytes=0), 0),
    ]
    torch.cuda.synchronize(gpu)
    for i, (rc, want) in enumerate(refused):
        assert rc == want, (i, rc, want)
    # nothing ran: the outputs and the scratch are what they were
    assert all(bool((t == 3.0).all()) for t in gw + gb + [gls, st]) and bool((scratch == 0x5A).all())
    assert actor() == 0 and value() == 0
    torch.cuda.synchronize(gpu)
    assert not bool((gls == 3.0).any()) and bool((scratch[need:] == 0x5A).all())
    env.close()
    other.close()


def test_a_network_past_the_lds_budget_is_refused(gpu):
    import invsim
    env, _ = _env(gpu, "im")
    mod = pr.make_module([33, 256, 256, 256, 1], "tanh", False, 3)
    vf = invsim.ValueMLP.from_module(mod)
    obs = torch.zeros((5, 33), dtype=torch.int64, device=gpu)
    assert env.mlp_values(vf, obs).shape == (5,)           # a legal invsim_mlp
    with pytest.raises(invsim._capi.InvsimError, match="LDS"):
        invsim.policies.value_grad(env, vf, {"obs": obs, "returns": torch.zeros(5, device=gpu)}, None)
    env.close()


# ---------------------------------------------------------------- end to end
def _params(actor, critic, log_std):
    return [p.detach().cpu().double().numpy() for p in list(actor.parameters()) + list(critic.parameters())] \
        + [log_std.detach().cpu().double().numpy()]


@pytest.mark.parametrize("family", ["im", "nv", "net"])
def test_learner_end_to_end(gpu, family):
    """two collect_rollout(critic=, normalize=) + PPOLearner.update iterations at 197
    envs, K = 9, beside the float64 learner of the reference fed the same buffers
    and permutations (both start an iteration with a fresh Adam): the parameters
    after the first minibatch to GRAD_TOL, after the whole update to 4 x what the
    float32 torch learner reaches; update enqueues without waiting for the device"""
    import copy

    import invsim
    from invsim.policies import Normalizer, PPOLearner, collect_rollout
    N, K, batch, epochs = 197, 9, 600, 2
    f = pr.FAMILIES[family]
    O, A = f["O"], f["A"]
    env, obs0 = _env(gpu, family, N)
    actor, critic = pr.make_module([O, 64, 64, A], "tanh", False, 71), pr.make_module([O, 64, 64, 1], "tanh", False, 72)
    ones, zeros = np.ones(O, F32), np.zeros(O, F32)
    # outputs of order 1 scaled into the action range, as a squashed actor's affine would
    high = env._action_high().astype(F64).reshape(-1)
    a_scale, a_shift = (0.1 * high).astype(F32), (0.3 * high).astype(F32)
    log_std_np = (np.log(0.1 * high) - 0.5).astype(F32)
    pi = invsim.GaussianMLPPolicyAgent.from_module(actor, log_std=log_std_np, seed=3, in_scale=ones, in_shift=zeros,
                                                   out_scale=a_scale, out_shift=a_shift)
    vf = invsim.ValueMLP.from_module(critic, in_scale=ones, in_shift=zeros)
    actor, critic = actor.to(gpu), critic.to(gpu)
    log_std = torch.nn.Parameter(_dev(gpu, log_std_np))
    norm = Normalizer(env)
    norm.observe(obs0)
    busy = torch.ones((4096, 4096), device=gpu)
    done0, slack = None, 0.0
    for it in range(2):
        buf = collect_rollout(env, pi, K, obs0, critic=vf, normalize=norm, done0=done0)
        before = (copy.deepcopy(actor), copy.deepcopy(critic), log_std.detach().clone())
        gen = torch.Generator(device=gpu).manual_seed(100 + it)
        perms = [torch.randperm(K * N, device=gpu, generator=gen) for _ in range(epochs)]
        # the first minibatch alone
        PPOLearner(env, pi, vf, actor, critic, log_std, n_epochs=1, batch_size=batch).update(buf, obs0,
                                                                                            perms=[perms[0][:batch]])
        got_first = _params(actor, critic, log_std)
        with torch.no_grad():
            for p, q in zip(list(actor.parameters()) + list(critic.parameters()) + [log_std],
                            list(before[0].parameters()) + list(before[1].parameters()) + [before[2]]):
                p.copy_(q)
        pi.update_from_module(env, actor, log_std=log_std)
        vf.update_from_module(env, critic)
        # the whole update, behind enough queued work that a wait for the device would show
        learner = PPOLearner(env, pi, vf, actor, critic, log_std, n_epochs=epochs, batch_size=batch)
        torch.cuda.synchronize(gpu)
        if it:
            for _ in range(60):
                busy = (busy @ busy).clamp_(0.0, 1e-3)
        stats = learner.update(buf, obs0, perms=perms)
        marker = torch.cuda.Event()
        marker.record()
        still_running = not marker.query()
        torch.cuda.synchronize(gpu)
        if it:
            assert still_running, "PPOLearner.update returned only after the device had finished the work queued before it"
        M = epochs * -(-K * N // batch)
        assert tuple(stats["actor"].shape) == (M, 6) and tuple(stats["critic"].shape) == (M, 2)
        assert bool(torch.isfinite(stats["actor"]).all()) and bool(torch.isfinite(stats["critic"]).all())
        assert all(p.grad is not None and p.grad.data_ptr() == g.data_ptr() for p, g in
                   [(log_std, learner._ga.log_std), (next(actor.parameters()), learner._ga.weight[0])])
        got_end = _params(actor, critic, log_std)
        host = dict(obs0=obs0.cpu().numpy(), obs=buf["obs"].reshape(K * N, O).cpu().numpy(),
                    raw=buf["raw_actions"].reshape(K * N, A).cpu().numpy(),
                    old_logp=buf["log_prob"].reshape(-1).cpu().numpy(), adv=buf["advantages"].reshape(-1).cpu().numpy(),
                    returns=buf["returns"].reshape(-1).cpu().numpy(), valid=buf["valid"].reshape(-1).cpu().numpy())
        kw = dict(in_scale=buf["obs_scale"].cpu().numpy(), in_shift=buf["obs_shift"].cpu().numpy(), out_scale=a_scale,
                  out_shift=a_shift)
        hperms = [p.cpu().numpy() for p in perms]
        start = (before[0].cpu(), before[1].cpu(), before[2].cpu().numpy())
        r64_first, r64_end = pr.learner(*start, host, hperms, batch, torch.float64, **kw)
        _, r32_end = pr.learner(*start, host, hperms, batch, torch.float32, **kw)
        m_first = max(pr.metric(a, b) for a, b in zip(got_first, r64_first))
        m32 = max(pr.metric(a, b) for a, b in zip(r32_end, r64_end))
        m_end = max(pr.metric(a, b) for a, b in zip(got_end, r64_end))
        print(f"{family} iteration {it}: after the first minibatch {m_first:.3e} (GRAD_TOL {pr.GRAD_TOL:.2e}); after "
              f"the update {m_end:.3e}, torch float32 {m32:.3e}, bound {4 * m32:.3e}")
        assert m_first <= pr.GRAD_TOL, (family, it, m_first)
        assert m_end <= 4 * m32, (family, it, m_end, m32)
        slack = max(slack, m_end / (4 * m32))
        obs0, done0 = buf["obs"][K - 1], buf["done"]
    print(f"{family}: largest end-of-update error / bound {slack:.3f}")
    env.close()
