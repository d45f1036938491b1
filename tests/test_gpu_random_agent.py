"""The in-kernel RandomAgent (INVSIM_POLICY_RANDOM, include/invsim.h
"RandomAgent") against its numpy model (tests/random_agent_model.py), bit for
bit: the drawn actions and the generators' final states, the trajectory those
actions give through the ordinary rollout on a twin env and through the C
oracle, the evaluate_agent metrics, sample_actions, chained launches, the
launch-choice knobs, per-env periods, shards, the fast demand stream, the
episode sink and the error paths.

Shapes: N = 200 is three full waves and a partial one (four 64-env groups),
N = 130 an odd group count; K is one NEXT_STEP cycle plus two steps, so a
reset step (whose action the env ignores, but which draws and records one) is
crossed.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import net_graphs
import random_agent_model as model
from conftest import knob_envs

pytestmark = pytest.mark.gpu

DSEED, ASEED = 321, 77        # demand seed (reset(seed=)), action seed (RandomAgent(seed=))


def _two_retailer_graph():
    """test_policies.py's graph outside the compiled specialisations (generic
    kernel): the default network with a second retailer off distributor 3."""
    from invsim.topology import default_graph
    g = default_graph()
    g.add_nodes_from([9], I0=60, h=0.025)
    g.add_edge(9, 0, p=2.5, b=0.2, demand_dist_func="poisson", dist_param={"lam": 7})
    g.add_edge(3, 9, L=2, p=1.4, g=0.012)
    return g


def _graph(name):
    from invsim.topology import custom_graph, default_graph
    return {"default": default_graph, "custom": custom_graph, "two_retailer": _two_retailer_graph}[name]()


# name -> (class, constructor arguments, K)
CONFIGS = {
    "im_backlog": ("InvManagementBacklogEnv", {}, 33),
    "im_lostsales": ("InvManagementLostSalesEnv", {}, 33),
    "nv_L5": ("NewsvendorEnv", {"lead_time": 5}, 43),
    "nv_L0": ("NewsvendorEnv", {"lead_time": 0}, 43),
    "net_default": ("NetInvMgmtBacklogEnv", {"graph": "default"}, 33),
    "net_custom": ("NetInvMgmtLostSalesEnv", {"graph": "custom"}, 33),
    "net_generic": ("NetInvMgmtBacklogEnv", {"graph": "two_retailer", "num_periods": 12}, 14),
}


def _make(gpu, name, n, seed=DSEED, **vec):
    import invsim
    cls, kw, _ = CONFIGS[name]
    kw = dict(kw)
    if "graph" in kw:
        kw["graph"] = _graph(kw["graph"])
    env = getattr(invsim, cls)(n, device=gpu, **kw, **vec)
    if name == "net_generic":
        assert env.kernel_variant == 0
    if seed is not None:
        env.reset(seed=seed)
    return env


def _np_dtype(env):
    return np.int64 if env.act_dtype == torch.int64 else np.float32


def _bits(t):
    t = t.detach().cpu()
    if t.dtype == torch.float64:
        return t.view(torch.int64).numpy()
    if t.dtype == torch.float32:
        return t.view(torch.int32).numpy()
    return t.numpy()


def _same(a, b, what):
    assert np.array_equal(_bits(a), _bits(b)), what


def _same_np(t, exp, what):
    got = t.detach().cpu().numpy()
    assert got.dtype == exp.dtype and got.shape == exp.shape, what
    w = {8: np.int64, 4: np.int32, 1: np.uint8}[got.dtype.itemsize]
    assert np.array_equal(got.view(w), exp.view(w)), what


def _expected(env, n, K, first=0, skip=0, seed=ASEED):
    return model.expected_actions(seed, first, n, K, env._action_high(), _np_dtype(env), skip=skip)


def _check_rng(env, n, st, what):
    got = env.action_rng_state()
    assert got.dtype == torch.int64 and got.shape[0] == 4 and got.shape[1] >= n
    assert np.array_equal(got[:, :n].cpu().numpy().view(np.uint64), st), what


def _run(env, agent, K, met=None):
    out = env.rollout_policy(agent, K, obs=True, actions=True, metrics=met)
    return out


def _compare_out(a, b, what):
    for k in ("actions", "obs", "reward", "terminated", "truncated"):
        _same(a[k], b[k], f"{what}: {k}")


def _metrics(env):
    import invsim
    return torch.zeros((env.num_envs, invsim.policies.metrics_dim(env)), dtype=torch.float64, device=env.device)


# ---------------------------------------------------------------- 1. actions and replay
@pytest.mark.parametrize("name,n", [("im_backlog", 130), ("im_backlog", 200), ("im_lostsales", 130),
                                    ("im_lostsales", 200), ("nv_L5", 200), ("nv_L0", 200), ("net_default", 200),
                                    ("net_custom", 200), ("net_generic", 200)])
def test_actions_and_replay(gpu, name, n):
    import invsim
    K = CONFIGS[name][2]
    env, twin = _make(gpu, name, n), _make(gpu, name, n)
    out = _run(env, invsim.RandomAgent(seed=ASEED), K)
    exp, st = _expected(env, n, K)
    _same_np(out["actions"], exp, "recorded actions == numpy model")
    _check_rng(env, n, st, "final action generator states == numpy model")
    high = torch.as_tensor(env._action_high(), device=gpu)
    assert bool((out["actions"] >= 0).all()) and bool((out["actions"] <= high).all())
    # the reset step was crossed: reward 0, no flag, and an action recorded all the same
    T = env._horizon()
    assert bool((out["reward"][T] == 0).all()) and bool(out["truncated"][T - 1].all())
    assert bool((out["actions"][T] != 0).any())
    obs, rew, te, tr = twin.rollout(out["actions"])
    _same(obs, out["obs"], "obs"), _same(rew, out["reward"], "reward")
    _same(te, out["terminated"], "terminated"), _same(tr, out["truncated"], "truncated")
    assert torch.equal(env.get_state(), twin.get_state())


def test_invmgmt_vs_oracle(gpu, oracle):
    """obs and reward bits of a RANDOM rollout against OracleInvMgmt.step driven
    by the model's actions, across the NEXT_STEP reset step."""
    import invsim
    n, K = 130, 33
    env = _make(gpu, "im_backlog", n)
    out = _run(env, invsim.RandomAgent(seed=ASEED), K)
    exp, _ = _expected(env, n, K)
    orc = _oracle_env(oracle, "im_backlog", n, DSEED)
    t = 0
    for k in range(K):
        if t == 30:                                  # the reset step: reset obs, reward 0, action ignored
            e_obs, e_rew, t = orc.reset(), np.zeros(n), 0
        else:
            e_obs, e_rew, _ = orc.step(exp[k])
            t += 1
        _same_np(out["obs"][k], e_obs, f"obs step {k}")
        _same_np(out["reward"][k], e_rew, f"reward step {k}")


# ---------------------------------------------------------------- 2. metrics
def _oracle_env(oracle, name, n, seed):
    kw = CONFIGS[name][1]
    if name.startswith("im"):
        orc = oracle.OracleInvMgmt(n, backlog=name == "im_backlog")
    elif name.startswith("nv"):
        orc = oracle.OracleNewsvendor(n, lead_time=kw["lead_time"])
    else:
        orc = oracle.OracleNet(n, graph=_graph(kw["graph"]), num_periods=kw.get("num_periods", 30))
    orc.seed(range(seed, seed + n))
    orc.reset()
    return orc


@pytest.mark.parametrize("name", ["im_backlog", "nv_L5", "net_default"])
def test_metrics_and_evaluate_agent(gpu, oracle, name):
    import invsim
    n = 130
    env = _make(gpu, name, n, seed=0, autoreset_mode="disabled")
    T = env._horizon()
    met = _metrics(env)
    out = _run(env, invsim.RandomAgent(seed=5), T, met)
    exp, st = _expected(env, n, T, seed=5)
    _same_np(out["actions"], exp, "actions")
    orc = _oracle_env(oracle, name, n, 0)
    fn = {"im": model.sums_invmgmt, "nv": model.sums_newsvendor, "ne": model.sums_net}[name[:2]]
    sums, e_rew, e_obs = fn(orc, exp)
    _same_np(out["reward"], e_rew, "reward == oracle")
    _same_np(out["obs"], e_obs, "obs == oracle")
    _same_np(met, sums, "metrics == the model's sums")
    cls, kw, _ = CONFIGS[name]
    cfg = dict(kw)
    if "graph" in cfg:
        cfg["graph"] = _graph(cfg["graph"])
    res = invsim.evaluate_agent(invsim.RandomAgent(seed=5), getattr(invsim, cls), cfg, n_episodes=n, device=gpu)
    cols = invsim.policies.summarize(env.family, sums)
    assert res["Agent"] == ["Random"] * n and res["Seed"].tolist() == list(range(n))
    for k, v in cols.items():
        assert np.array_equal(np.asarray(res[k]), np.asarray(v)), k


# ---------------------------------------------------------------- 3. sample_actions and chaining
@pytest.mark.parametrize("name", ["im_lostsales", "nv_L5", "net_custom", "net_generic"])
def test_sample_actions_and_chaining(gpu, name):
    import invsim
    n, K = 200, 12
    one, two, three = (_make(gpu, name, n) for _ in range(3))
    m1, m2 = _metrics(one), _metrics(two)
    full = _run(one, invsim.RandomAgent(seed=ASEED), K, m1)
    ag = invsim.RandomAgent(seed=ASEED)
    p1 = _run(two, ag, 5, m2)
    p2 = _run(two, ag, 7, m2)
    _compare_out(full, {k: torch.cat([p1[k], p2[k]]) for k in full}, "5 + 7 steps == 12 steps")
    _same(m1, m2, "metrics")
    _same(one.action_rng_state(), two.action_rng_state(), "generator state")
    assert torch.equal(one.get_state(), two.get_state())
    three.seed_actions(ASEED)
    st0 = three.action_rng_state()
    sa = three.sample_actions(K)
    _same(sa, full["actions"], "sample_actions == the rollout's recorded actions")
    _same(three.action_rng_state(), one.action_rng_state(), "sample_actions advances as the rollout")
    _same_np(three.sample_actions(3), _expected(one, n, 3, skip=K)[0], "the stream continues")
    three.set_action_rng_state(st0)
    _same(three.sample_actions(K), sa, "a restored state replays the same actions")
    assert three.get_state().equal(_make(gpu, name, n).get_state())      # env state and demand rng untouched


# ---------------------------------------------------------------- 4. fused == generic
# default path -> path with the knob: im_roll3o two-group (N = 200, four groups) and
# one-group (N = 130, three groups) -> im_run_kernel; im_roll3o -> im_roll3_kernel's
# policy form (IM_ROLL3O_MAX_N = 0), and that one -> im_run_kernel; nv_roll ->
# nv_run; net_roll3o -> net_spec
@pytest.mark.parametrize("name,n,var,val,base", [
    ("im_backlog", 200, "INVSIM_IM_POL_ROLL", "0", None), ("im_backlog", 130, "INVSIM_IM_POL_ROLL", "0", None),
    ("im_lostsales", 200, "INVSIM_IM_POL_ROLL", "0", None), ("im_lostsales", 130, "INVSIM_IM_POL_ROLL", "0", None),
    ("im_backlog", 200, "INVSIM_IM_ROLL3O_MAX_N", "0", None),
    ("im_lostsales", 200, "INVSIM_IM_POL_ROLL", "0", ("INVSIM_IM_ROLL3O_MAX_N", "0")),
    ("nv_L5", 200, "INVSIM_NV_POL_ROLL", "0", None), ("net_default", 200, "INVSIM_NET_POL_ROLL", "0", None),
    ("net_custom", 200, "INVSIM_NET_POL_ROLL", "0", None)])
@pytest.mark.parametrize("stream", ["numpy", "philox"])
def test_knobs_do_not_change_results(gpu, monkeypatch, name, n, var, val, base, stream):
    """The default launch path (the fused rollout kernels' RANDOM variants) and
    the path with the knob set give identical outputs, metrics, env state and
    action generator state, under both demand streams (7: the fast stream's
    rollout equals the generic kernel).  base: a knob both envs are made with."""
    import invsim
    K = CONFIGS[name][2]
    if base:
        monkeypatch.setenv(*base)
    a, b = knob_envs(monkeypatch, var, [None, val], lambda: _make(gpu, name, n, demand_stream=stream))
    ma, mb = _metrics(a), _metrics(b)
    oa = _run(a, invsim.RandomAgent(seed=ASEED), K, ma)
    ob = _run(b, invsim.RandomAgent(seed=ASEED), K, mb)
    _compare_out(oa, ob, f"{var}={val}")
    _same(ma, mb, "metrics")
    _same(a.action_rng_state(), b.action_rng_state(), "action generators")
    assert torch.equal(a.get_state(), b.get_state())
    _same_np(oa["actions"], _expected(a, n, K)[0], "actions == numpy model")


# ---------------------------------------------------------------- 5. staggered periods
@pytest.mark.parametrize("name", ["im_backlog", "nv_L0", "nv_L5", "net_default", "net_generic"])
def test_staggered_periods(gpu, name):
    """After a masked reset of half the envs mid-episode (per-env periods: the
    run kernels' TU = false instantiations) the actions are the model continued,
    and the twin replay still matches."""
    import invsim
    n = 200
    env, twin = _make(gpu, name, n), _make(gpu, name, n)
    T = env._horizon()
    K1, K2 = T // 3, T                                # the unreset half crosses its reset step in launch 2
    ag = invsim.RandomAgent(seed=ASEED)
    mask = (torch.arange(n, device=gpu) % 2 == 0)
    o1 = _run(env, ag, K1)
    env.reset(options={"reset_mask": mask})
    o2 = _run(env, ag, K2)
    exp, st = _expected(env, n, K1 + K2)
    _same_np(torch.cat([o1["actions"], o2["actions"]]), exp, "actions == numpy model, continued")
    _check_rng(env, n, st, "generator states")
    r0 = o2["reward"][T - K1]                         # the unreset envs' reset step
    assert bool((r0[1::2] == 0).all()) and bool((r0[0::2] != 0).any())
    for o, first in ((o1, True), (o2, False)):
        if not first:
            twin.reset(options={"reset_mask": mask})
        obs, rew, te, tr = twin.rollout(o["actions"])
        _same(obs, o["obs"], "obs"), _same(rew, o["reward"], "reward")
        _same(te, o["terminated"], "terminated"), _same(tr, o["truncated"], "truncated")
    assert torch.equal(env.get_state(), twin.get_state())


# ---------------------------------------------------------------- 6. shard invariance
@pytest.mark.parametrize("name", ["im_backlog", "nv_L5", "net_default"])
def test_shard_invariance(gpu, name):
    import invsim
    K = CONFIGS[name][2]
    full, part = _make(gpu, name, 200), _make(gpu, name, 72, global_offset=64)
    of = _run(full, invsim.RandomAgent(seed=ASEED), K)
    op = _run(part, invsim.RandomAgent(seed=ASEED), K)
    for k in ("actions", "obs", "reward", "truncated"):
        _same(op[k], of[k][:, 64:136], f"rows 64..135: {k}")
    _same(part.action_rng_state()[:, :72], full.action_rng_state()[:, 64:136], "generator states")


# ---------------------------------------------------------------- 7. philox demand stream
@pytest.mark.parametrize("name", ["im_backlog", "nv_L5", "nv_L0", "net_default", "net_generic"])
def test_philox_demand_stream_same_actions(gpu, name):
    import invsim
    n, K = 200, CONFIGS[name][2]
    env = _make(gpu, name, n, demand_stream="philox")
    rng0 = env.state_fields()["rng"].clone()
    out = _run(env, invsim.RandomAgent(seed=ASEED), K)
    exp, st = _expected(env, n, K)
    _same_np(out["actions"], exp, "actions == numpy model under the fast demand stream")
    _check_rng(env, n, st, "generator states")
    assert torch.equal(env.state_fields()["rng"], rng0), "the demand generators' rows are untouched"


def test_two_agents_keep_their_own_streams(gpu):
    """An agent continues the generators it seeded for an env, also after
    another agent or seed_actions attached others in between."""
    import invsim
    n = 130
    env = _make(gpu, "im_backlog", n)
    a, b = invsim.RandomAgent(seed=ASEED), invsim.RandomAgent(seed=ASEED + 1)
    a1 = _run(env, a, 4)["actions"]
    b1 = _run(env, b, 4)["actions"]
    env.seed_actions(999)
    a2 = _run(env, a, 5)["actions"]
    b2 = _run(env, b, 5)["actions"]
    _same_np(torch.cat([a1, a2]), _expected(env, n, 9)[0], "first agent")
    _same_np(torch.cat([b1, b2]), _expected(env, n, 9, seed=ASEED + 1)[0], "second agent")


# ---------------------------------------------------------------- 8. episode sink
def test_sink_random_rollout_equals_fold(gpu):
    import invsim
    from invsim.distributed import EpisodeStats
    n = 200
    a, b = _make(gpu, "im_backlog", n), _make(gpu, "im_backlog", n)
    sa, sb = EpisodeStats(n, gpu), EpisodeStats(n, gpu)
    sa.attach(a)
    aa, ab = invsim.RandomAgent(seed=ASEED), invsim.RandomAgent(seed=ASEED)
    for K in (30, 31, 7):
        a.rollout_policy(aa, K)
        out = b.rollout_policy(ab, K)
        sb.update_block(out["reward"].contiguous(), out["terminated"].contiguous(), out["truncated"].contiguous())
        torch.cuda.synchronize()
        _same(sa.ret, sb.ret, f"running returns K={K}")
        _same(sa.part, sb.part, f"group partials K={K}")
    assert float(sa.acc[2]) == 2 * n


# ---------------------------------------------------------------- 9. errors
def test_errors(gpu):
    import invsim
    from invsim import _capi
    env = _make(gpu, "im_backlog", 130)
    high = env._action_high()
    spec = _capi.PolicySpec(_capi.POLICY_KINDS["random"], 0, 0.0, 0.0, high.ctypes.data)
    rc = env._lib.invsim_rollout_policy(env._h, 3, C.byref(spec), None, None, None, None, None, None, env._stream())
    assert rc == -22 and "invsim_set_action_rng" in _capi.last_error(env._h)
    acts = torch.zeros((3, 130, 3), dtype=torch.int64, device=gpu)
    rc = env._lib.invsim_sample_actions(env._h, 3, high.ctypes.data, acts.data_ptr(), env._stream())
    assert rc == -22 and "invsim_set_action_rng" in _capi.last_error(env._h)
    with pytest.raises(RuntimeError, match="seed_actions"):
        env.action_rng_state()
    env.seed_actions(1)
    env._attach_action_rng(None)                       # NULL detaches
    rc = env._lib.invsim_rollout_policy(env._h, 3, C.byref(spec), None, None, None, None, None, None, env._stream())
    assert rc == -22
    same = _make(gpu, "im_backlog", 130, autoreset_mode="same_step")
    with pytest.raises(_capi.InvsimError, match=r"\(-22\)"):
        same.rollout_policy(invsim.RandomAgent(seed=1), 3)
    wide = invsim.NetInvMgmtMasterEnv(130, device=gpu, graph=net_graphs.wide(), num_periods=8)
    assert wide.action_dim > 32
    wide.reset(seed=1)
    with pytest.raises(_capi.InvsimError, match=r"\(-34\)"):
        wide.rollout_policy(invsim.RandomAgent(seed=1), 3)
    with pytest.raises(_capi.InvsimError, match=r"\(-34\)"):
        wide.rollout_policy(invsim.ConstantOrderAgent(0.1), 3)             # as CONSTANT does
    # the env still steps after the refusals
    out = _run(env, invsim.RandomAgent(seed=ASEED), 4)
    _same_np(out["actions"], _expected(env, 130, 4)[0], "after the refusals")
