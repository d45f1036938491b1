"""GPU: the running-normalisation calls (include/invsim.h "Running
normalisation") against tests/norm_model.py, bit for bit (a NaN equals any NaN):
invsim_moments over every leaf / tree shape, dtype, mask and kernel path, the
discounted-return scan, reward normalisation and input-row parameters,
invsim_mlp_set_input_norm against an object created with the same rows, and
collect_rollout(normalize=...) composed from the model over what it returned,
with a captured moments -> norm_params -> set_input_norm -> values chain."""
import numpy as np
import pytest
import torch

import gae_model
import mlp_model
import norm_model as nm
from test_gpu_gae import KEYS, N, _actor, _critic, _dev, _layers, _make, _obs, _same

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
B = nm.BLOCK
EINVAL = -22
ROWS = [1, B - 1, B, B + 1, 2 * B + 1, 5 * B + 3, 37 * B + 5]
NP_DTYPES = {"i64": np.int64, "f32": np.float32, "f64": np.float64}


def _data(rows, cols, dtype, seed):
    """int64: values float32 cannot hold, as _obs of tests/test_gpu_gae.py makes; floats: +-0, +-inf and NaN entries"""
    rng = np.random.default_rng(seed)
    if dtype == np.int64:
        x = rng.integers(0, 400, (rows, cols))
        x[::23, min(1, cols - 1)] = 2 ** 24 + 1
        x[::31, 0] = -(2 ** 40) - 2 ** 15 - 1
        return x
    x = rng.uniform(-50, 400, (rows, cols)).astype(dtype)
    vals = np.array([0.0, -0.0, np.inf, -np.inf, np.nan])
    hit = rng.random((rows, cols)) < 0.002
    x[hit] = vals[rng.integers(0, len(vals), int(hit.sum()))].astype(dtype)
    return x


def _masks(rows, seed):
    off = np.ones(rows, np.uint8)
    off[B:2 * B] = 0                       # one whole block off (where there is a second block)
    return {"none": None, "random": (np.random.default_rng(seed).random(rows) < 0.6).astype(np.uint8), "block": off,
            "all": np.zeros(rows, np.uint8)}


# ---------------------------------------------------------------- 1. invsim_moments
@pytest.mark.parametrize("cols", [1, 3, 33, 68, 311])
@pytest.mark.parametrize("dt", ["i64", "f32", "f64"])
def test_moments_bit_exact(gpu, dt, cols):
    """a single leaf, a ragged last block, odd node counts at several levels; several
    leaves per pass (cols 1, 3), one (33; 68 in f32) and column chunks (68 in 8 bytes,
    311); every mask; a second call on the result, which is the running merge; the prior"""
    import invsim
    seen_nan = False
    for rows in ROWS:
        x = _data(rows, cols, NP_DTYPES[dt], seed=rows + cols)
        xd = _dev(gpu, x)
        for name, mask in _masks(rows, rows).items():
            rm = invsim.RunningMoments(cols, gpu)
            _same(rm.stats, nm.prior(cols), "the prior")
            rm.update(xd, mask=_dev(gpu, mask))
            want = nm.moments(x, mask)
            _same(rm.stats, want, f"{dt} rows={rows} cols={cols} mask={name}", nan_ok=True)
            if name == "all":
                _same(rm.stats, nm.prior(cols), "a fully masked call leaves the statistics as they were")
            rm.update(xd.flip(0).contiguous(), mask=None if mask is None else _dev(gpu, mask[::-1].copy()).bool())
            want2 = nm.moments(x[::-1], None if mask is None else mask[::-1], want)
            _same(rm.stats, want2, f"{dt} rows={rows} cols={cols} mask={name}: second call", nan_ok=True)
            seen_nan |= bool(np.isnan(want2).any())
    if dt == "i64":
        assert not seen_nan
    elif cols >= 3:
        assert seen_nan, "NaN / inf entries reach the statistics of the float dtypes"


@pytest.mark.parametrize("dt,cols", [("i64", 33), ("f32", 3), ("f64", 1)])
def test_moments_unaligned_rows(gpu, dt, cols):
    """x that does not start on a 16-byte boundary (a row-slice of a tensor) takes the element-wise loads"""
    import invsim
    rows = 5 * B + 3
    x = _data(rows + 1, cols, NP_DTYPES[dt], seed=9)
    xd = _dev(gpu, x)[1:]
    assert xd.is_contiguous() and (xd.data_ptr() % 16 != 0 or cols * x.itemsize % 16 == 0)
    rm = invsim.RunningMoments(cols, gpu).update(xd)
    _same(rm.stats, nm.moments(x[1:]), f"{dt} cols={cols} from row 1", nan_ok=True)


@pytest.mark.parametrize("dt,rows,cols", [("i64", 70001, 33), ("f64", 256 * 256 * B + 77, 1), ("f32", 197 * 31, 68)])
def test_moments_several_workgroups_and_tree_launches(gpu, dt, rows, cols):
    """more than 256 workgroup nodes (two tree launches), a [K, N, O] block passed as it is, a mask"""
    import invsim
    x = _data(rows, cols, NP_DTYPES[dt], seed=3)
    if dt != "i64":
        x = np.nan_to_num(x, nan=1.0, posinf=2.0, neginf=-2.0)
    mask = (np.random.default_rng(1).random(rows) < 0.9).astype(np.uint8)
    xd = _dev(gpu, x)
    if cols == 68:
        xd = xd.reshape(31, 197, cols)
    rm = invsim.RunningMoments(cols, gpu).update(xd)
    _same(rm.stats, nm.moments(x), f"{dt} rows={rows} cols={cols}")
    rm.update(xd, mask=_dev(gpu, mask))
    _same(rm.stats, nm.moments(x, mask, nm.moments(x)), f"{dt} rows={rows} cols={cols}: masked second call")
    assert bool((rm.count == 1e-4 + rows + int(mask.sum())).all())
    assert torch.allclose(rm.var, rm.stats[2] / rm.stats[0]) and rm.mean.shape == (cols,)


def test_moments_at_31_times_2_20_rows(gpu):
    """the largest row count the contract names, one column: 507 904 leaves, three tree launches"""
    import invsim
    rows = 31 * 1048576
    xd = torch.randint(-400, 400, (rows,), device=gpu, generator=torch.Generator(device=gpu).manual_seed(0))
    rm = invsim.RunningMoments(1, gpu).update(xd)
    _same(rm.stats, nm.moments(xd.cpu().numpy()[:, None]), "31 x 2^20 rows")


# ---------------------------------------------------------------- 2. returns, rewards, parameters
@pytest.mark.parametrize("K", [1, 2, 9, 31])
def test_returns_rewards_params_bit_exact(gpu, K):
    import invsim
    from invsim import _capi, policies
    n = 197
    for seed, gamma in enumerate((0.99, 1.0, 0.0, 0.5)):
        c = gae_model.synthetic(K, n, seed=seed)
        ret0 = np.random.default_rng(seed).uniform(-1e3, 1e3, n)
        for drop in (None, "terminated", "truncated", "done0"):
            d = dict(c, **({drop: None} if drop else {}))
            ret = _dev(gpu, ret0)
            out, valid = policies.discounted_returns(_dev(gpu, d["reward"]), _dev(gpu, d["terminated"]),
                                                     _dev(gpu, d["truncated"]), ret, gamma, done0=_dev(gpu, d["done0"]))
            w_out, w_valid, w_ret = nm.discounted_returns(d["reward"], d["terminated"], d["truncated"], d["done0"], gamma, ret0)
            what = f"K={K} gamma={gamma} without {drop}"
            assert valid.dtype == torch.bool
            _same(valid, w_valid, f"{what}: valid")
            _same(out, w_out, f"{what}: out", nan_ok=True)
            _same(ret, w_ret, f"{what}: ret", nan_ok=True)
        # the statistics of the valid returns, the normalised rewards (into a new tensor and in place)
        rms = invsim.RunningMoments(1, gpu).update(out, mask=valid)
        w_stats = nm.moments(w_out.reshape(-1, 1), w_valid.reshape(-1))
        _same(rms.stats, w_stats, f"K={K}: return statistics", nan_ok=True)
    cs = gae_model.synthetic(K, n, seed=5, specials=False)
    o2, v2, _ = nm.discounted_returns(cs["reward"], cs["terminated"], cs["truncated"], cs["done0"], 0.99, np.zeros(n))
    stats = nm.moments(o2.reshape(-1, 1), v2.reshape(-1))
    rew = _dev(gpu, c["reward"])                                 # with NaN, +-inf and +-0.0 entries
    for st, eps, clip in ((stats, 1e-8, 10.0), (stats, 1e-8, 0.5), (np.zeros((3, 1)), 0.0, 1e9)):
        want = nm.normalize_rewards(c["reward"], st, eps, clip)
        got = policies.normalize_rewards(rew, _dev(gpu, st), eps, clip)
        _same(got, want, f"K={K} clip={clip} cnt={st[0, 0]}", nan_ok=True)
        alias = rew.clone()
        assert policies.normalize_rewards(alias, _dev(gpu, st), eps, clip, out=alias) is alias
        _same(alias, want, f"K={K} clip={clip}: out aliasing reward", nan_ok=True)
    assert np.isnan(want).any() or K < 9
    # valid = NULL: out and ret all the same, nothing else written
    lib, s = _capi.lib(), torch.cuda.current_stream(gpu).cuda_stream
    ret, out = _dev(gpu, ret0), torch.zeros((K, n), dtype=torch.float64, device=gpu)
    assert lib.invsim_discounted_returns(rew.data_ptr(), None, None, None, K, n, 0.99, ret.data_ptr(), out.data_ptr(),
                                         None, s) == 0
    w_out, _, w_ret = nm.discounted_returns(c["reward"], None, None, None, 0.99, ret0)
    _same(out, w_out, "no flags, valid = NULL: out", nan_ok=True), _same(ret, w_ret, "ret", nan_ok=True)
    # input-row parameters: columns with data, the bare prior, cnt == 0; shift = NULL
    obs = _data(K * n, 6, np.int64, seed=K)
    st = nm.moments(obs)
    st[:, 4] = nm.prior(1)[:, 0]
    st[:, 5] = 0.0
    rm = invsim.RunningMoments(6, gpu)
    rm.stats.copy_(_dev(gpu, st))
    for eps in (1e-8, 0.0, 1.0):
        scale, shift = rm.scale_shift(eps)
        w_scale, w_shift = nm.norm_params(st, eps)
        _same(scale, w_scale, f"scale eps={eps}"), _same(shift, w_shift, f"shift eps={eps}")
    only = torch.zeros(6, dtype=torch.float32, device=gpu)
    assert lib.invsim_norm_params(rm.stats.data_ptr(), 6, 1.0, only.data_ptr(), None, s) == 0
    _same(only, w_scale, "shift = NULL")


# ---------------------------------------------------------------- 3. invsim_mlp_set_input_norm
def _with_rows(invsim, net, scale, shift, **kw):
    """a new agent with net's parameters and the given input rows on the host"""
    cls = type(net)
    if isinstance(net, invsim.GaussianMLPPolicyAgent):
        kw = dict(kw, log_std=net.log_std, seed=net.seed, out_activation=net.out_activation, clip=net.clip)
    elif not isinstance(net, invsim.ValueMLP):
        kw = dict(kw, out_activation=net.out_activation, clip=net.clip)
    return cls(list(zip(net.weights, net.biases)), activation=net.activation, in_scale=scale, in_shift=shift,
               out_scale=net.out_scale, out_shift=net.out_shift, **kw)


@pytest.mark.parametrize("name", ["im", "nv"])
def test_set_input_norm_equals_a_fresh_object(gpu, name):
    import invsim
    from invsim import _capi
    (env, obs0), (other, _) = _make(gpu, name), _make(gpu, name)
    obs = _obs(env, N)
    O = env.obs_dim
    rng = np.random.default_rng(17)
    scale, shift = (0.02 * (1 + 0.2 * rng.standard_normal(O))).astype(F32), (0.3 * rng.standard_normal(O)).astype(F32)
    sd, hd = _dev(gpu, scale), _dev(gpu, shift)
    actor, critic = _actor(env), _critic(env, (64, 64))
    env.mlp_sample(actor, obs), env.mlp_values(critic, obs)                 # both objects have been used
    before = env.mlp_actions(actor, obs, raw=True)[1]
    actor.set_input_norm(env, sd, hd), critic.set_input_norm(env, sd, hd)
    f_actor, f_critic = _with_rows(invsim, actor, scale, shift), _with_rows(invsim, critic, scale, shift)
    actor._bufs.pop(env)                                                     # both sample from a newly seeded buffer
    got, (act_got, raw_got) = env.mlp_sample(actor, obs), env.mlp_actions(actor, obs, raw=True)
    want, (act_want, raw_want) = env.mlp_sample(f_actor, obs), env.mlp_actions(f_actor, obs, raw=True)
    for k in ("actions", "raw_actions", "mean", "log_prob"):
        _same(got[k], want[k], f"{name}: sample after set_input_norm: {k}")
    _same(act_got, act_want, "actions"), _same(raw_got, raw_want, "raw")
    _same(raw_got, mlp_model.forward(f_actor, obs.cpu().numpy()), "and they are the model's")
    assert not torch.equal(raw_got, before), "the rows changed something"
    _same(env.mlp_values(critic, obs), env.mlp_values(f_critic, obs), "values")
    _same(env.mlp_values(critic, obs), mlp_model.forward(f_critic, obs.cpu().numpy())[:, 0], "values: the model's")
    with pytest.raises(RuntimeError, match="update_from_module"):
        other.mlp_values(critic, obs)                                        # the host arrays are the old rows
    # the three refusals; the object stays usable and unchanged
    lib, s = env._lib, env._stream()
    bare = invsim.MLPPolicyAgent(_layers([O, 16, env.action_dim], rng), activation="relu")
    b_obj, a_obj = bare.device_object(env), actor.device_object(env)
    o_obj = _critic(other).device_object(other)
    keep = env.mlp_actions(bare, obs, raw=True)[1]
    assert lib.invsim_mlp_set_input_norm(env._h, b_obj, sd.data_ptr(), hd.data_ptr(), s) == EINVAL
    assert "in_scale" in _capi.last_error(env._h)
    assert lib.invsim_mlp_set_input_norm(env._h, o_obj, sd.data_ptr(), hd.data_ptr(), s) == EINVAL
    assert "another handle" in _capi.last_error(env._h)
    assert lib.invsim_mlp_set_input_norm(env._h, a_obj, None, hd.data_ptr(), s) == EINVAL
    assert lib.invsim_mlp_set_input_norm(env._h, a_obj, sd.data_ptr(), None, s) == EINVAL
    _same(env.mlp_actions(bare, obs, raw=True)[1], keep, "an object without rows: unchanged")
    _same(env.mlp_actions(actor, obs, raw=True)[1], raw_want, "the actor: unchanged by the refusals")
    with pytest.raises(ValueError, match="in_scale"):
        bare.set_input_norm(env, sd, hd)


# ---------------------------------------------------------------- 4. collect_rollout(normalize=...)
def _np(t):
    return None if t is None else t.cpu().numpy()


def _check_normalized(invsim, env, critic, norm, before, out, obs0, done0, gamma, lam, what):
    """every key normalize adds or changes, composed from the model over the returned obs / reward / flags"""
    obs_stats0, ret_stats0, ret0 = before
    Kk, n = out["reward"].shape
    obs = _np(out["obs"]).reshape(Kk * n, env.obs_dim)
    obs_stats = nm.moments(obs, None, obs_stats0)
    scale, shift = nm.norm_params(obs_stats, norm.epsilon)
    _same(norm.obs_rms.stats, obs_stats, f"{what}: obs statistics")
    _same(out["obs_scale"], scale, f"{what}: obs_scale"), _same(out["obs_shift"], shift, f"{what}: obs_shift")
    assert out["obs_scale"] is norm.obs_scale and out["obs_shift"] is norm.obs_shift
    rew, te, tr, d0 = _np(out["reward"]), _np(out["terminated"]), _np(out["truncated"]), _np(done0)
    dr, dr_valid, ret = nm.discounted_returns(rew, te, tr, d0, norm.gamma, ret0)
    ret_stats = nm.moments(dr.reshape(-1, 1), dr_valid.reshape(-1), ret_stats0)
    _same(norm.ret, ret, f"{what}: running return"), _same(norm.ret_rms.stats, ret_stats, f"{what}: return statistics")
    rn = nm.normalize_rewards(rew, ret_stats, norm.epsilon, norm.clip_reward)
    _same(out["reward_norm"], rn, f"{what}: reward_norm")
    assert float(np.abs(rn).max()) <= norm.clip_reward and float(np.abs(rn).max()) > 0
    allobs = np.concatenate([_np(obs0)[None], _np(out["obs"])]).reshape((Kk + 1) * n, env.obs_dim)
    v = mlp_model.forward(_with_rows(invsim, critic, scale, shift), allobs)[:, 0].reshape(Kk + 1, n)
    _same(out["values"], v[:Kk], f"{what}: values under the new rows"), _same(out["last_value"], v[Kk], f"{what}: last_value")
    adv, retn, valid = gae_model.gae(rn, te, tr, d0, v[0], v[1:], gamma, lam)
    _same(out["advantages"], adv, f"{what}: advantages"), _same(out["returns"], retn, f"{what}: returns")
    _same(out["valid"], valid, f"{what}: valid"), _same(out["valid"], dr_valid, f"{what}: valid is the returns' too")
    return obs_stats, ret_stats, ret


@pytest.mark.parametrize("name", ["im", "nv"])
def test_collect_rollout_normalize(gpu, name):
    """int64 and f32 observations, K = periods + 2 (a reset row inside), two calls chained with done0"""
    import invsim
    collect = invsim.policies.collect_rollout
    (env, obs0), (twin, obs0_t) = _make(gpu, name), _make(gpu, name)
    Kk = (7 if name == "im" else 6) + 2
    actor, actor_t, critic = _actor(env), _actor(twin), _critic(env, (16,))
    norm = invsim.Normalizer(env, gamma=0.97, clip_reward=5.0)
    _same(norm.obs_scale, nm.norm_params(nm.prior(env.obs_dim), 1e-8)[0], "rows of the prior")
    norm.observe(obs0)
    state = (nm.moments(_np(obs0)), nm.prior(1), np.zeros(N))
    _same(norm.obs_rms.stats, state[0], "observe(obs0)")
    base = ("values", "last_value", "advantages", "returns", "valid", "done")
    cur, cur_t, done = obs0, obs0_t, None
    for call in range(2):
        out = collect(env, actor, Kk, cur, critic=critic, gamma=0.98, gae_lambda=0.9, done0=done, normalize=norm)
        ref = collect(twin, actor_t, Kk, cur_t)
        assert sorted(out) == sorted(KEYS + base + ("reward_norm", "obs_scale", "obs_shift"))
        for k in KEYS:                                           # the rollout ran under the rows the call began with
            _same(out[k], ref[k], f"{name} call {call}: {k} with and without normalize")
        assert out["reward"].dtype == torch.float64 and out["reward_norm"].dtype == torch.float64
        state = _check_normalized(invsim, env, critic, norm, state, out, cur, done, 0.98, 0.9, f"{name} call {call}")
        resets = (~out["valid"]).all(1)
        assert bool(resets.any()), "a reset row inside the call"
        actor_t.set_input_norm(twin, out["obs_scale"], out["obs_shift"])     # the twin's next call: the same input rows
        cur, cur_t, done = out["obs"][-1], ref["obs"][-1], out["done"]
    assert torch.equal(env.get_state(), twin.get_state())
    # without a critic: the statistics advance, no values; norm_obs / norm_reward off: nothing of that kind moves
    out = collect(env, actor, 3, cur, done0=done, normalize=norm)
    assert sorted(out) == sorted(KEYS + ("reward_norm", "obs_scale", "obs_shift", "done"))
    off = invsim.Normalizer(env, norm_obs=False, norm_reward=False)
    o2 = collect(env, actor, 3, out["obs"][-1], critic=critic, done0=out["done"], normalize=off)
    assert o2["reward_norm"] is o2["reward"]
    _same(off.obs_rms.stats, nm.prior(env.obs_dim), "norm_obs off"), _same(off.ret_rms.stats, nm.prior(1), "norm_reward off")
    with pytest.raises(ValueError, match="in_scale"):
        collect(env, actor, 3, cur, critic=_critic(env, scales=False), normalize=norm)


def test_collect_rollout_normalize_callable_critic(gpu):
    """a torch module as the critic gets float32 observations already normalised"""
    import invsim
    env, obs0 = _make(gpu, "nv")
    actor = _actor(env)
    norm = invsim.Normalizer(env)
    seen = {}

    def critic(x):
        seen["x"] = x
        return x.sum(-1)
    out = invsim.policies.collect_rollout(env, actor, 4, obs0, critic=critic, normalize=norm)
    allobs = torch.cat([obs0[None], out["obs"]]).float()
    want = allobs * out["obs_scale"] + out["obs_shift"]
    assert seen["x"].dtype == torch.float32 and torch.allclose(seen["x"], want, rtol=1e-5, atol=1e-5)
    assert torch.equal(seen["x"], norm.normalize_obs(torch.cat([obs0[None], out["obs"]])))


# ---------------------------------------------------------------- 5. capture
def test_graph_of_moments_params_rows_values(gpu):
    """invsim_moments -> invsim_norm_params -> invsim_mlp_set_input_norm -> invsim_mlp_values captured on one
    stream and replayed twice: the statistics are the model's two merges, the values those of the second rows"""
    import invsim
    env, obs0 = _make(gpu, "im")
    critic = _critic(env, (16,))
    critic.device_object(env)                     # the first meeting synchronises: before the capture
    rows = 5 * N
    x = _obs(env, rows, seed=4)
    rm = invsim.RunningMoments(env.obs_dim, gpu)
    v = torch.zeros(rows, dtype=torch.float32, device=gpu)

    def fn():
        rm.update(x, stream=env._stream())
        scale, shift = rm.scale_shift(1e-8, stream=env._stream())
        critic.set_input_norm(env, scale, shift)
        env._mlp_values_into(critic, x, rows, v)
        return scale, shift
    g = env.capture(fn, warmup=1)
    assert g.steps == 0
    rm.stats.copy_(_dev(gpu, nm.prior(env.obs_dim)))             # the warm-up run merged once: start again
    want = nm.prior(env.obs_dim)
    xn = x.cpu().numpy()
    for rep in range(2):
        v.zero_()
        scale, shift = g.replay()
        torch.cuda.synchronize(gpu)
        want = nm.moments(xn, None, want)
        _same(rm.stats, want, f"replay {rep}: statistics")
        w_scale, w_shift = nm.norm_params(want, 1e-8)
        _same(scale, w_scale, f"replay {rep}: scale"), _same(shift, w_shift, f"replay {rep}: shift")
        _same(v, mlp_model.forward(_with_rows(invsim, critic, w_scale, w_shift), xn)[:, 0], f"replay {rep}: values")
    assert bool((rm.count == (1e-4 + rows) + rows).all())
