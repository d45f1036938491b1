"""GPU: the PPO data path as a learner sees it.  Every kernel of the path (the
MLP actor and critic, Gaussian sampling and its log-probability, invsim_gae, the
running moments, the discounted return, reward and input-row normalisation,
invsim_mlp_update) and collect_rollout(critic=, normalize=) end to end are held
against the float64 / extended-precision references of tests/learner_reference.py,
which are written from the textbook definitions and share nothing with the
numpy models the bit-exact tests use.  The tolerances are derived bounds, stated
with each comparison function there; the one measured tolerance (MLP_TOL) is
measured by tests/test_learner_view.py on the same networks and observations."""
import numpy as np
import pytest
import torch

import learner_reference as lr
import norm_model
from test_gpu_gae import _cls_kw

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SEED = 400
B = norm_model.BLOCK             # the leaf size the moments' bound counts with (read from include/invsim.h)
GL = [(0.99, 0.95), (1.0, 1.0), (0.5, 0.0), (0.9, 1.0)]
FEATURES = {"done at row 0", "done at row K - 1", "terminated alone", "truncated alone", "both", "two episodes end",
            "done0", "no done0", "+-1e3"}


def _make(gpu, family, n):
    cls, kw = _cls_kw(family)
    env = cls(n, device=gpu, **kw)
    obs0, _ = env.reset(seed=SEED)
    f = lr.FAMILIES[family]
    assert env.obs_dim == f["O"] and np.array_equal(env._action_high().astype(F64), np.asarray(f["high"]))
    return env, obs0


def _dev(gpu, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _space(env):
    sp = env.single_action_space
    return np.asarray(sp.low, F64).reshape(-1), np.asarray(sp.high, F64).reshape(-1), np.dtype(sp.dtype)


def _convert(env):
    """the reference's output through invsim.policies.convert_actions, float64 in"""
    from invsim.policies import convert_actions
    low, high, _ = _space(env)
    return lambda ref: convert_actions(torch.from_numpy(ref), low, high, env.act_dtype).numpy()


# ---------------------------------------------------------------- (a) mean and values
@pytest.mark.parametrize("act", lr.ACTIVATIONS)
@pytest.mark.parametrize("i", range(len(lr.NETWORKS)), ids=[c[0] for c in lr.NETWORKS])
def test_mean_and_values_are_the_modules(gpu, i, act):
    """mlp_actions(raw=True), mlp_sample's mean and mlp_values against the torch
    module in float64, on the env's reset observations and on synthetic ones, N =
    197, 1 and 64, and mlp_values on a whole [K + 1, N, O] block; the converted actions
    are convert_actions of the reference away from the boundaries"""
    import invsim
    cid, family, hidden = lr.NETWORKS[i]
    f = lr.FAMILIES[family]
    A, O = len(f["high"]), f["O"]
    a_mod = lr.make_module([O] + hidden + [A], act, lr.module_seed(i, act))
    c_mod = lr.make_module([O] + hidden + [1], act, lr.module_seed(i, act, True))
    a_aff, c_aff = lr.affines(family), lr.affines(family, value=True)
    log_std = np.log(0.2 * np.asarray(f["high"])).astype(F32)
    worst = 0.0
    for n in lr.N_ENVS:
        env, obs0 = _make(gpu, family, n)
        low, high, adt = _space(env)
        plain = invsim.MLPPolicyAgent.from_module(a_mod, **a_aff)
        gauss = invsim.GaussianMLPPolicyAgent.from_module(a_mod, log_std=log_std, seed=0, **a_aff)
        critic = invsim.ValueMLP.from_module(c_mod, **c_aff)
        for sname, obs in (("reset", obs0), ("synthetic", _dev(gpu, lr.synthetic_obs(family, lr.N_ENVS[0], seed=i + 1)[:n]))):
            what = f"{cid} {act} n={n} {sname}"
            ref, cond = lr.forward64(a_mod, obs, **a_aff)
            lr.check_condition(ref, cond, what)
            actions, raw = env.mlp_actions(plain, obs, raw=True)
            worst = max(worst, lr.check_forward(raw, ref, cond, f"{what}: mlp_actions raw"))
            lr.check_actions(actions, ref, cond, low, high, adt, f"{what}: mlp_actions", _convert(env))
            out = env.mlp_sample(gauss, obs)
            lr.check_forward(out["mean"], ref, cond, f"{what}: mlp_sample mean")
            assert torch.equal(out["mean"], raw), f"{what}: the sampling launch reports another mean"
            vref, vcond = lr.forward64(c_mod, obs, **c_aff)
            lr.check_condition(vref, vcond, what)
            v = env.mlp_values(critic, obs)
            assert tuple(v.shape) == (n,)
            worst = max(worst, lr.check_forward(v, vref[:, 0], vcond[:, 0], f"{what}: mlp_values"))
        blk = _dev(gpu, lr.synthetic_obs(family, (lr.K + 1) * lr.N_ENVS[0], seed=i + 50)[:(lr.K + 1) * n]).reshape(lr.K + 1, n, O)
        vref, vcond = lr.forward64(c_mod, blk, **c_aff)
        lr.check_condition(vref, vcond, f"{cid} {act} n={n} block")
        v = env.mlp_values(critic, blk)
        assert tuple(v.shape) == (lr.K + 1, n)
        worst = max(worst, lr.check_forward(v, vref[..., 0], vcond[..., 0], f"{cid} {act} n={n}: mlp_values on the block"))
        env.close()
    print(f"{cid} {act}: max |kernel - f64| / condition scale = {worst:.3e} (MLP_TOL {lr.MLP_TOL:.3e})")


# ---------------------------------------------------------------- (b) samples and log-probabilities
def _std32(log_std):
    """the library's std: exp in float64, rounded to float32"""
    return np.exp(np.asarray(log_std, F32).astype(F64)).astype(F32)


def _check_stream(raw, mean, std, z, what):
    """raw within one float32 ulp of mean + std * float32(z), evaluated in float64"""
    want = mean.astype(F64) + std.astype(F64) * z.astype(F32).astype(F64)
    err = np.abs(raw.astype(F64) - want)
    ulp = np.spacing(np.abs(want).astype(F32)).astype(F64)
    assert (err <= ulp).all(), f"{what}: {int((err > ulp).sum())} samples are not the documented stream, " \
                               f"worst {float((err / ulp).max()):.3g} ulp"


@pytest.mark.parametrize("family,width", [("im", 0.2), ("nv", 0.2), ("net", 0.2), ("im", 0.002)])
def test_samples_and_log_probs_are_the_distributions(gpu, family, width):
    """mlp_sample and collect_rollout: log_prob against Normal(mean, std).log_prob(raw).sum(-1)
    of the library's own float32 mean and raw within the derived bound, the
    importance ratio a learner forms from it, and the sample against numpy's
    stream for the env's global index, continuing across the steps"""
    import invsim
    n, Kk = lr.N_ENVS[0], lr.K
    i = [c[1] for c in lr.NETWORKS].index(family)
    f = lr.FAMILIES[family]
    A = len(f["high"])
    mod = lr.make_module([f["O"]] + lr.OWN[family] + [A], "relu", lr.module_seed(i, "relu"))
    aff = lr.affines(family)
    log_std = np.log(width * np.asarray(f["high"])).astype(F32)
    std = _std32(log_std)
    env, obs0 = _make(gpu, family, n)
    agent = invsim.GaussianMLPPolicyAgent.from_module(mod, log_std=log_std, seed=5, **aff)
    z = lr.action_normals(5, 0, n, A * (1 + Kk)).reshape(n, 1 + Kk, A)
    syn = _dev(gpu, lr.synthetic_obs(family, n, seed=i + 1))
    out = env.mlp_sample(agent, syn)
    mean, raw = out["mean"].cpu().numpy(), out["raw_actions"].cpu().numpy()
    lp, bound = lr.log_prob64(mean, log_std, raw)
    slack = lr.check_log_prob(out["log_prob"], lp, bound, f"{family} {width}: mlp_sample")
    _check_stream(raw, mean, std, z[:, 0], f"{family} {width}: mlp_sample")
    roll = invsim.policies.collect_rollout(env, agent, Kk, obs0)
    inputs = torch.cat([obs0[None], roll["obs"][:-1]])
    mean = torch.stack([env.mlp_actions(agent, o, raw=True)[1] for o in inputs]).cpu().numpy()
    raw = roll["raw_actions"].cpu().numpy()
    lp, bound = lr.log_prob64(mean, log_std, raw)
    slack = max(slack, lr.check_log_prob(roll["log_prob"], lp, bound, f"{family} {width}: collect_rollout"))
    _check_stream(raw, mean, std, z[:, 1:].transpose(1, 0, 2), f"{family} {width}: collect_rollout")
    low, high, adt = _space(env)
    assert np.array_equal(roll["actions"].cpu().numpy(), _convert(env)(raw.astype(F64))), "actions are the converted samples"
    print(f"{family} A={A} width {width}: max bound {bound.max():.3e}, error / bound <= {slack:.3f}")


# ---------------------------------------------------------------- (c) GAE
def _features(c):
    te, tr, d0 = c["terminated"].astype(bool), c["truncated"].astype(bool), c["done0"].astype(bool)
    done = te | tr
    checks = ((done[0].any(), "done at row 0"), (done[-1].any(), "done at row K - 1"), ((te & ~tr).any(), "terminated alone"),
              ((tr & ~te).any(), "truncated alone"), ((te & tr).any(), "both"), ((done.sum(0) >= 2).any(), "two episodes end"),
              (d0.any(), "done0"), ((~d0).any(), "no done0"), ((np.abs(c["reward"]) == 1e3).any(), "+-1e3"))
    return {name for hit, name in checks if hit}


@pytest.mark.parametrize("K", [1, 2, 9, 31])
def test_gae_kernel_is_the_definition(gpu, K):
    import invsim
    n, seen = lr.N_ENVS[0], set()
    for seed, (gamma, lam) in enumerate(GL):
        c = lr.legal_block(K, n, seed)
        out = invsim.policies.gae(_dev(gpu, c["reward"]), _dev(gpu, c["terminated"]), _dev(gpu, c["truncated"]),
                                  _dev(gpu, c["value0"]), _dev(gpu, c["values"]), gamma, lam, done0=_dev(gpu, c["done0"]))
        lr.check_gae(out["returns"], out["valid"], out["advantages"], c, gamma, lam, f"K={K} gamma={gamma} lambda={lam}")
        seen |= _features(c)
    if K >= 9:
        assert seen == FEATURES, FEATURES - seen


# ---------------------------------------------------------------- (d) normalisation kernels
@pytest.mark.parametrize("dtype,cols", lr.MOMENT_CASES, ids=lr.MOMENT_IDS)
@pytest.mark.parametrize("rows", lr.MOMENT_ROWS)
def test_moments_kernel_is_running_mean_var(gpu, rows, dtype, cols):
    """one call, a masked call, two calls chained, and the input rows made from them"""
    import invsim
    x, y = lr.moment_data(dtype, cols, rows, seed=rows), lr.moment_data(dtype, cols, rows, seed=rows + 1)
    mask = np.random.default_rng(rows).random(rows) < 0.6
    mask[0] = True
    xd, yd, md = _dev(gpu, x), _dev(gpu, y), _dev(gpu, mask)
    rm = invsim.RunningMoments(cols, gpu).update(xd)
    lr.check_moments(rm.stats, [x], None, B, f"rows={rows}")
    lr.check_moments(invsim.RunningMoments(cols, gpu).update(xd, mask=md).stats, [x], [mask], B, f"rows={rows} masked")
    rm.update(yd, mask=md)
    lr.check_moments(rm.stats, [x, y], [None, mask], B, f"rows={rows}: two calls")
    count, mean, var = lr.running_mean_var([x, y], [None, mask])
    for eps in (1e-8, 1e-2):
        lr.check_scale_shift(*rm.scale_shift(eps), mean, var, eps, f"rows={rows} eps={eps}")


@pytest.mark.parametrize("K", [1, 2, 9, 31])
def test_returns_and_reward_kernels_are_the_definitions(gpu, K):
    import invsim
    from invsim import policies
    n = lr.N_ENVS[0]
    for seed, gamma in enumerate((0.99, 1.0, 0.5, 0.97)):
        c = lr.legal_block(K, n, seed)
        ret0 = np.where(c["done0"], 0.0, np.random.default_rng(seed).uniform(-1e3, 1e3, n))
        ret = _dev(gpu, ret0)
        out, valid = policies.discounted_returns(_dev(gpu, c["reward"]), _dev(gpu, c["terminated"]), _dev(gpu, c["truncated"]),
                                                 ret, gamma, done0=_dev(gpu, c["done0"]))
        lr.check_returns(out, valid, c, gamma, ret0, f"K={K} gamma={gamma}", new_ret=ret)
        rms = invsim.RunningMoments(1, gpu).update(out, mask=valid)
        ref, mask, _ = lr.returns_by_definition(c["reward"], c["terminated"], c["truncated"], c["done0"], ret0, gamma)
        lr.check_moments(rms.stats, [ref.reshape(-1, 1)], [mask.reshape(-1)], B, f"K={K}: statistics of the returns")
        count, mean, var = lr.running_mean_var([ref.reshape(-1, 1)], [mask.reshape(-1)])
        for eps, clip in ((1e-8, 10.0), (1e-8, 0.5)):
            got = policies.normalize_rewards(_dev(gpu, c["reward"]), rms.stats, eps, clip)
            lr.check_reward_norm(got, c["reward"], var[0], eps, clip, f"K={K} clip={clip}")


# ---------------------------------------------------------------- (e) one PPO iteration
def _np(t):
    return None if t is None else t.detach().cpu().numpy()


@pytest.mark.parametrize("family", ["im", "nv", "net"])
def test_one_ppo_iteration_as_the_learner_sees_it(gpu, family):
    """two chained collect_rollout(critic=, normalize=) calls with a truncation and a
    reset row inside each, then one Adam step written back with update_from_module"""
    import invsim
    n = lr.N_ENVS[0]
    gamma, lam = 0.98, 0.9
    env, obs0 = _make(gpu, family, n)
    Kk = (7 if family == "im" else 6) + 2
    f = lr.FAMILIES[family]
    A, O = len(f["high"]), f["O"]
    i = [c[1] for c in lr.NETWORKS].index(family)
    a_mod = lr.make_module([O] + lr.OWN[family] + [A], "relu", lr.module_seed(i, "relu"))
    c_mod = lr.make_module([O] + lr.OWN[family] + [1], "relu", lr.module_seed(i, "relu", True))
    a_out = {k: v for k, v in lr.affines(family).items() if k.startswith("out")}
    c_out = {k: v for k, v in lr.affines(family, value=True).items() if k.startswith("out")}
    log_std = torch.nn.Parameter(torch.from_numpy(np.log(0.2 * np.asarray(f["high"])).astype(F32)))
    norm = invsim.Normalizer(env, gamma=0.97)
    norm.observe(obs0)
    # the rows the first call begins with: saved statistics, as a learner that resumes would load (the rows of
    # observe(obs0) alone, N near-identical reset observations, would scale the first steps by 1 / sqrt(1e-4 / N))
    rows = tuple(_dev(gpu, lr.affines(family)[k]) for k in ("in_scale", "in_shift"))
    actor = invsim.GaussianMLPPolicyAgent.from_module(a_mod, log_std=_np(log_std), seed=3, in_scale=_np(rows[0]),
                                                      in_shift=_np(rows[1]), **a_out)
    critic = invsim.ValueMLP.from_module(c_mod, in_scale=_np(rows[0]), in_shift=_np(rows[1]), **c_out)
    z = lr.action_normals(3, 0, n, A * 2 * Kk).reshape(n, 2 * Kk, A).transpose(1, 0, 2)
    std = _std32(_np(log_std))
    obs_batches, ret_batches, ret_masks, rewards, flags = [_np(obs0)], [], [], [], []
    cur, done = obs0, None
    for call in range(2):
        what = f"{family} call {call}"
        began = rows
        out = invsim.policies.collect_rollout(env, actor, Kk, cur, critic=critic, gamma=gamma, gae_lambda=lam, done0=done,
                                              normalize=norm)
        inputs = torch.cat([cur[None], out["obs"][:-1]])
        te, tr = _np(out["terminated"]), _np(out["truncated"])
        # log-probability under the rows the call began with
        mref, mcond = lr.forward64(a_mod, inputs, rows[0], rows[1], **a_out)
        raw = _np(out["raw_actions"])
        lp, bound = lr.log_prob64(mref, _np(log_std), raw)
        zabs = np.abs(raw.astype(F64) - mref) / std.astype(F64)
        extra = (zabs * lr.MLP_TOL * mcond / std.astype(F64)).sum(-1)
        # the mean is not compared itself here; its conditioning shows in the widening, which must leave the
        # comparison its teeth (0.919 per action for a dropped constant, |log_std| for a flipped sign)
        assert float((bound + extra).max()) <= 1e-2, f"{what}: the widened bound reaches {float((bound + extra).max()):.3e}"
        slack = lr.check_log_prob(out["log_prob"], lp, bound, f"{what}: log_prob under the old rows", extra=extra)
        print(f"{what}: log_prob bound {bound.max():.3e} + widening {extra.max():.3e}, error / bound <= {slack:.3f}")
        # the sample is the stream around the reference's mean, up to the mean's own tolerance
        want = mref + std.astype(F64) * z[call * Kk:(call + 1) * Kk].astype(F32).astype(F64)
        assert (np.abs(raw - want) <= lr.MLP_TOL * mcond + np.spacing(np.abs(want).astype(F32))).all(), f"{what}: the samples"
        # statistics
        obs_batches.append(_np(out["obs"]).reshape(Kk * n, O))
        lr.check_moments(norm.obs_rms.stats, obs_batches, None, B, f"{what}: obs_rms")
        _, omean, ovar = lr.running_mean_var(obs_batches)
        lr.check_scale_shift(out["obs_scale"], out["obs_shift"], omean, ovar, norm.epsilon, f"{what}: input rows")
        rewards.append(_np(out["reward"]))
        flags.append((te, tr))
        allr, allte, alltr = np.concatenate(rewards), np.concatenate([x[0] for x in flags]), np.concatenate([x[1] for x in flags])
        dref, dmask, _ = lr.returns_by_definition(allr, allte, alltr, None, np.zeros(n), norm.gamma)
        ret_batches.append(dref[call * Kk:].reshape(-1, 1))
        ret_masks.append(dmask[call * Kk:].reshape(-1))
        lr.check_moments(norm.ret_rms.stats, ret_batches, ret_masks, B, f"{what}: ret_rms")
        _, _, rvar = lr.running_mean_var(ret_batches, ret_masks)
        lr.check_reward_norm(out["reward_norm"], rewards[-1], rvar[0], norm.epsilon, norm.clip_reward, what)
        assert float(out["reward_norm"].abs().max()) > 0
        # values under the new rows
        allobs = torch.cat([cur[None], out["obs"]])
        vref, vcond = lr.forward64(c_mod, allobs, out["obs_scale"], out["obs_shift"], **c_out)
        lr.check_condition(vref, vcond, f"{what}: values")
        v = torch.cat([out["values"], out["last_value"][None]])
        lr.check_forward(v, vref[..., 0], vcond[..., 0], f"{what}: values under the new rows")
        # advantages from the library's own values, over reward_norm and the flags
        c = dict(reward=_np(out["reward_norm"]), terminated=te, truncated=tr, done0=_np(done), value0=_np(v[0]),
                 values=_np(v[1:]))
        lr.check_gae(out["returns"], out["valid"], out["advantages"], c, gamma, lam, what)
        k_tr = np.argwhere(tr[:-1])
        assert len(k_tr) and not te.any(), "a truncation inside the call"
        ob = _np(out["obs"])
        assert (ob[k_tr[:, 0], k_tr[:, 1]] != ob[k_tr[:, 0] + 1, k_tr[:, 1]]).any(-1).all(), \
            f"{what}: a truncated row holds the final observation, not the reset one after it"
        assert not _np(out["valid"])[k_tr[:, 0] + 1, k_tr[:, 1]].any()
        rows, cur, done = (out["obs_scale"], out["obs_shift"]), out["obs"][-1], out["done"]
    # one Adam step on the clipped surrogate and the value loss, from the library's tensors of the last call
    opt = torch.optim.Adam(list(a_mod.parameters()) + list(c_mod.parameters()) + [log_std], lr=1e-2)
    valid = out["valid"].cpu()
    x = inputs.cpu().float()
    s0, h0 = (t.cpu() for t in began)                           # the rows the last rollout ran with
    mean = a_mod(x * s0 + h0) * torch.from_numpy(a_out["out_scale"]) + torch.from_numpy(a_out["out_shift"])
    new_lp = torch.distributions.Normal(mean, log_std.exp()).log_prob(out["raw_actions"].cpu()).sum(-1)
    ratio = (new_lp - out["log_prob"].cpu()).exp()
    adv = out["advantages"].cpu()
    adv = (adv - adv[valid].mean()) / (adv[valid].std() + 1e-8)
    pg = -torch.minimum(ratio * adv, ratio.clamp(0.8, 1.2) * adv)[valid].mean()
    s1, h1 = out["obs_scale"].cpu(), out["obs_shift"].cpu()
    value = c_mod(x * s1 + h1)[..., 0] * float(c_out["out_scale"][0]) + float(c_out["out_shift"][0])
    loss = pg + 0.5 * ((out["returns"].cpu() - value) ** 2)[valid].mean()
    assert abs(float(ratio[valid].mean().detach()) - 1) < 1e-3, "the first epoch's ratio is 1 under the rows the rollout ran with"
    last = out["obs"][-1]
    before_mean, before_v = env.mlp_actions(actor, last, raw=True)[1], env.mlp_values(critic, last)
    opt.zero_grad()
    loss.backward()
    opt.step()
    actor.update_from_module(env, a_mod, log_std=log_std)
    critic.update_from_module(env, c_mod)
    got = env.mlp_sample(actor, last)
    mref, mcond = lr.forward64(a_mod, last, s1, h1, **a_out)
    lr.check_forward(got["mean"], mref, mcond, f"{family}: mean after the update")
    lp, bound = lr.log_prob64(_np(got["mean"]), _np(log_std), _np(got["raw_actions"]))
    lr.check_log_prob(got["log_prob"], lp, bound, f"{family}: log_prob after the update")
    vref, vcond = lr.forward64(c_mod, last, s1, h1, **c_out)
    lr.check_forward(env.mlp_values(critic, last), vref[:, 0], vcond[:, 0], f"{family}: values after the update")
    moved = np.abs(_np(got["mean"]).astype(F64) - _np(before_mean)) > lr.MLP_TOL * mcond
    moved_v = np.abs(_np(env.mlp_values(critic, last)).astype(F64) - _np(before_v)) > lr.MLP_TOL * vcond[:, 0]
    assert moved.mean() > 0.9 and moved_v.mean() > 0.9, "the step moved the outputs by more than the tolerance"
