"""invsim_rollout_metrics (caller-supplied actions with evaluate_agent's per-env
sums) and the TorchPolicyAgent closed loop built on it, bit for bit: against
the in-kernel agents whose recorded actions are replayed on a twin env, against
the C oracle with the sums of oracle/agents.py run_*, across chained calls,
per-env periods, both demand streams, the optional outputs, the episode sink
and the error paths.

Shapes: N = 197 is three full 64-env waves and a partial one (the replay also
runs N = 1 and N = 65); the horizons are short (InvMgmt periods = 7, Newsvendor
step_limit = 6, NetInvMgmt num_periods = 6) and K = 17 under NEXT_STEP
autoreset, so two episode ends and their reset steps fall inside one launch.
"""
import numpy as np
import pytest
import torch

import net_graphs
import random_agent_model as model
import staggered

pytestmark = pytest.mark.gpu

N, K = 197, 17
SEED, ASEED = 400, 77
UNKNOWN = 0xFFFFFFFF          # invsim_position's low word when the periods differ per env

# name -> (oracle family, device env arguments, oracle arguments)
CASES = {
    "im_backlog": ("im", dict(periods=7, backlog=True), dict(periods=7, backlog=True)),
    "im_lostsales": ("im", dict(periods=7, backlog=False), dict(periods=7, backlog=False)),
    "nv": ("nv", dict(step_limit=6), dict(step_limit=6)),
    "net_default": ("net", dict(graph="default", num_periods=6, backlog=True), None),
    "net_mixed": ("net", dict(graph="mixed", num_periods=6, backlog=True), None),
}


def _graph(name):
    from invsim.topology import default_graph
    return default_graph() if name == "default" else net_graphs.mixed(net_graphs.by_name, 6)


def _make(gpu, name, n=N, seed=SEED, **vec):
    """(env, obs0): a freshly seeded and reset device env of the case"""
    import invsim
    fam, kw, _ = CASES[name]
    kw = dict(kw)
    if fam == "im":
        cls = invsim.InvManagementBacklogEnv if kw.pop("backlog") else invsim.InvManagementLostSalesEnv
    elif fam == "nv":
        cls = invsim.NewsvendorEnv
    else:
        cls = invsim.NetInvMgmtMasterEnv
        kw["graph"] = _graph(kw["graph"])
    env = cls(n, device=gpu, **kw, **vec)
    if fam == "net":
        assert env.kernel_variant == (1 if name == "net_default" else 0)     # specialised / generic kernels
    obs0, _ = env.reset(seed=seed)
    return env, obs0


def _agent(name, random=False):
    import invsim
    if random:
        return invsim.RandomAgent(seed=ASEED)
    fam = CASES[name][0]
    if fam == "im":
        return invsim.BaseStockAgent(1.0)
    if fam == "nv":
        return invsim.OrderUpToHeuristicAgent(1.0)
    return invsim.ConstantOrderAgent(0.1)


def _metrics(env, fill=0.0):
    import invsim
    return torch.full((env.num_envs, invsim.policies.metrics_dim(env)), fill, dtype=torch.float64, device=env.device)


def _bits(t):
    t = t.detach().cpu()
    if t.dtype == torch.float64:
        return t.view(torch.int64).numpy()
    if t.dtype == torch.float32:
        return t.view(torch.int32).numpy()
    return t.numpy()


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert np.array_equal(_bits(a), _bits(b)), what


def _same_np(t, exp, what):
    got = t.detach().cpu().numpy()
    assert got.dtype == exp.dtype and got.shape == exp.shape, f"{what}: {got.dtype}{got.shape} vs {exp.dtype}{exp.shape}"
    w = {8: np.int64, 4: np.int32, 1: np.uint8}[got.dtype.itemsize]
    if not np.array_equal(got.view(w), exp.view(w)):
        bad = np.argwhere(got.view(w) != exp.view(w))[:4].tolist()
        pytest.fail(f"{what}: first mismatches at {bad}")


def _same_out(a, b, what, keys=("obs", "reward", "terminated", "truncated")):
    for k in keys:
        _same(a[k], b[k], f"{what}: {k}")


# ---------------------------------------------------------------- the oracle side
def _oracle(oracle, name, n=N, masks=None, mode="next_step"):
    """the cohort harness over pyoracle (tests/staggered.py): one oracle per reset history"""
    fam, kw, okw = CASES[name]
    if okw is None:
        okw = dict(graph=_graph(kw["graph"]), num_periods=kw["num_periods"], backlog=kw["backlog"])
    masks = np.zeros((1, n), bool) if masks is None else np.asarray(masks, bool).reshape(-1, n)
    h = staggered.CohortOracle(oracle, fam, n, SEED, masks, mode, **okw)
    h.reset()
    return h


def _oracle_rows(h, acts, met):
    """Step the oracle (info=True) with acts [K, N, A] and keep evaluate_agent's
    sums as oracle/agents.py run_invmgmt / run_newsvendor / run_net keep them,
    in `met` [N, M] (+=): a NEXT_STEP reset row adds nothing.  Returns the
    expected obs / reward / truncated rows and the stepped-row counts."""
    rows = [h.row(actions=np.ascontiguousarray(a), metrics=met) for a in acts]
    assert not any(r.raises for r in rows)
    return (np.stack([r.obs for r in rows]), np.stack([r.reward for r in rows]),
            np.stack([r.truncated for r in rows]), sum(r.stepped.astype(np.float64) for r in rows))


def _check_rows(out, exp, what):
    obs, rew, trunc, _ = exp
    _same_np(out["obs"], obs, f"{what}: obs == oracle")
    _same_np(out["reward"], rew, f"{what}: reward == oracle")
    _same_np(out["truncated"], trunc, f"{what}: truncated == oracle")
    assert not bool(out["terminated"].any()), f"{what}: terminated"


def _random_actions(env, k, edge=True):
    """env.sample_actions with some rows overwritten by negative and over-capacity orders"""
    if env._arng is None:
        env.seed_actions(ASEED)
    a = env.sample_actions(k)
    if edge:
        high = torch.as_tensor(env._action_high(), device=env.device)
        a[:, 3::7] = -5
        a[:, 5::11] = high * 4 + 1000
        a[1::3, 2::13, 0] = -1
    return a


# ---------------------------------------------------------------- 1. replay of the in-kernel agents
def _replay(gpu, name, n, random, **vec):
    (env, _), (twin, _) = _make(gpu, name, n, **vec), _make(gpu, name, n, **vec)
    met, met2 = _metrics(env), _metrics(twin)
    out = env.rollout_policy(_agent(name, random), K, obs=True, actions=True, metrics=met)
    T = env._horizon()
    assert bool(out["truncated"][T - 1].all()) and bool((out["reward"][T] == 0).all()), "a reset step is crossed"
    assert bool((met[:, 1] == K - 2).all()), "two reset steps add nothing"
    rep = twin.rollout_metrics(out["actions"], metrics=met2)
    _same_out(rep, out, "replay")
    _same(met2, met, "metrics")
    assert torch.equal(env.get_state(), twin.get_state()), "state blob"


@pytest.mark.parametrize("n", [N, 1, 65])
@pytest.mark.parametrize("random", [False, True], ids=["heuristic", "random"])
@pytest.mark.parametrize("name", list(CASES))
def test_replay_of_in_kernel_agents(gpu, name, random, n):
    """BaseStock / OrderUpTo / Constant / Random in the kernel, then the recorded
    actions through rollout_metrics on a twin: the same obs, rewards, flags,
    metrics and state blob"""
    _replay(gpu, name, n, random)


# ---------------------------------------------------------------- 2. oracle
@pytest.mark.parametrize("name", list(CASES))
def test_metrics_against_oracle(gpu, oracle, name):
    env, _ = _make(gpu, name, record_demand=True)
    a = _random_actions(env, K)
    met = _metrics(env)
    out = env.rollout_metrics(a, metrics=met)
    emet = np.zeros(tuple(met.shape))
    exp = _oracle_rows(_oracle(oracle, name), a.cpu().numpy(), emet)
    _check_rows(out, exp, name)
    _same_np(met, emet, "every metric column == the oracle's sums")
    _same_np(met[:, 1], exp[3], "steps == stepped rows")


# ---------------------------------------------------------------- 3. chaining
@pytest.mark.parametrize("name", ["im_backlog", "im_lostsales", "nv", "net_default", "net_mixed"])
def test_chaining(gpu, name):
    """K = 17 in one call, 17 calls of K = 1 and 5 + 12: the same bits; metrics
    that start non-zero are added to"""
    (one, _), (two, _), (three, _) = (_make(gpu, name) for _ in range(3))
    a = _random_actions(one, K)
    start = torch.arange(N, device=gpu, dtype=torch.float64)[:, None] * 0.25 + 1000.0
    m0, m1, m2, m3 = _metrics(one), _metrics(one) + start, _metrics(two) + start, _metrics(three) + start
    full = one.rollout_metrics(a, metrics=m1)
    parts = [two.rollout_metrics(a[k:k + 1], metrics=m2) for k in range(K)]
    _same_out(full, {k: torch.cat([p[k] for p in parts]) for k in full}, "17 x 1 == 17")
    parts = [three.rollout_metrics(a[:5], metrics=m3), three.rollout_metrics(a[5:], metrics=m3)]
    _same_out(full, {k: torch.cat([p[k] for p in parts]) for k in full}, "5 + 12 == 17")
    _same(m2, m1, "metrics 17 x 1"), _same(m3, m1, "metrics 5 + 12")
    assert torch.equal(one.get_state(), two.get_state()) and torch.equal(one.get_state(), three.get_state())
    # from zero on a fourth env: the step counts are exact either way, the start is kept
    four, _ = _make(gpu, name)
    four.rollout_metrics(a, metrics=m0)
    assert bool((m0[:, 1] == K - 2).all()) and bool((m1[:, 1] == start[:, 0] + (K - 2)).all())
    assert bool((m1[:, 0] != m0[:, 0]).all())


# ---------------------------------------------------------------- 4. per-env periods
@pytest.mark.parametrize("name", ["im_backlog", "im_lostsales", "nv", "net_default", "net_mixed"])
def test_per_env_periods_against_oracle(gpu, oracle, name):
    """after a masked reset of half the envs mid-episode (the TU = false
    instantiations): outputs and metrics match the oracle"""
    env, _ = _make(gpu, name)
    mask = np.arange(N) % 2 == 0
    h = _oracle(oracle, name, masks=mask)
    a = _random_actions(env, 3 + K)
    an = a.cpu().numpy()
    met, emet = _metrics(env), np.zeros((N, h.met_dim))
    out = env.rollout_metrics(a[:3], metrics=met)
    _check_rows(out, _oracle_rows(h, an[:3], emet), "lock-step rows")
    env.reset(options={"reset_mask": torch.from_numpy(mask).to(gpu)})
    h.reset(mask)
    assert env.position() & UNKNOWN == UNKNOWN, "per-env periods after the mask"
    out = env.rollout_metrics(a[3:], metrics=met)
    exp = _oracle_rows(h, an[3:], emet)
    _check_rows(out, exp, "staggered rows")
    _same_np(met, emet, "metrics == the oracle's sums")
    T = env._horizon()
    r0 = out["reward"][T - 3]                       # the unreset envs' reset step, the reset ones step
    assert bool((r0[1::2] == 0).all()) and bool((r0[0::2] != 0).any())
    f = env.state_fields()
    _same_np(f["period"][0], h.periods(), "period row")


# ---------------------------------------------------------------- 5. the fast demand stream
@pytest.mark.parametrize("name", ["im_backlog", "nv"])
def test_replay_philox(gpu, name):
    _replay(gpu, name, N, False, demand_stream="philox")


# ---------------------------------------------------------------- 6. optional outputs and the sink
@pytest.mark.parametrize("name", ["im_lostsales", "nv", "net_default", "net_mixed"])
def test_optional_outputs(gpu, name):
    envs = [_make(gpu, name)[0] for _ in range(4)]
    a = _random_actions(envs[0], K)
    mets = [_metrics(e) for e in envs]
    full = envs[0].rollout_metrics(a, metrics=mets[0])
    no_obs = envs[1].rollout_metrics(a, metrics=mets[1], obs=False)
    no_rew = envs[2].rollout_metrics(a, metrics=mets[2], rewards=False)
    bare = envs[3].rollout_metrics(a, metrics=mets[3], obs=False, rewards=False)
    assert set(no_obs) == {"reward", "terminated", "truncated"} and set(no_rew) == {"obs"} and bare == {}
    _same_out(no_obs, full, "obs=False", keys=("reward", "terminated", "truncated"))
    _same(no_rew["obs"], full["obs"], "rewards=False: obs")
    for m, e in zip(mets[1:], envs[1:]):
        _same(m, mets[0], "metrics do not depend on the outputs asked for")
        assert torch.equal(e.get_state(), envs[0].get_state())
    # metrics=None: the dynamics alone
    env, _ = _make(gpu, name)
    _same_out(env.rollout_metrics(a), full, "metrics=None")
    with pytest.raises(ValueError, match="metrics"):
        env.rollout_metrics(a, metrics=torch.zeros((N, 1), dtype=torch.float64, device=gpu))


@pytest.mark.parametrize("name", ["im_backlog", "nv", "net_default"])
def test_episode_sink_equals_fold(gpu, name):
    """with EpisodeStats attached, ret / part equal invsim_episode_fold_groups over the returned rows"""
    from invsim import _capi
    from invsim.distributed import EpisodeStats
    (a, _), (b, _) = _make(gpu, name), _make(gpu, name)
    sa, sb = EpisodeStats(N, gpu), EpisodeStats(N, gpu)
    sa.attach(a)
    acts = _random_actions(a, K + 1 + 5)
    ma, mb = _metrics(a), _metrics(b)
    for lo, hi in ((0, K), (K, K + 1), (K + 1, K + 6)):
        oa = a.rollout_metrics(acts[lo:hi], metrics=ma)
        ob = b.rollout_metrics(acts[lo:hi], metrics=mb)
        _same_out(oa, ob, "the sink changes no output")
        sb.update_block(ob["reward"].contiguous(), ob["terminated"].contiguous(), ob["truncated"].contiguous())
        torch.cuda.synchronize()
        _same(sa.ret, sb.ret, f"running returns rows {lo}:{hi}")
        _same(sa.part, sb.part, f"group partials rows {lo}:{hi}")
    _same(ma, mb, "metrics")
    assert float(sa.acc[2]) == 3 * N, "three episode ends folded"
    with pytest.raises(_capi.InvsimError, match=r"\(-22\)"):      # the sink folds the reward outputs
        a.rollout_metrics(acts[:2], rewards=False)


# ---------------------------------------------------------------- 7. errors
def test_errors_refused_before_any_launch(gpu):
    from invsim import _capi
    same, _ = _make(gpu, "im_backlog", autoreset_mode="same_step")
    a = torch.zeros((3, N, 3), dtype=torch.int64, device=gpu)
    st = same.get_state()
    with pytest.raises(_capi.InvsimError, match=r"\(-22\)"):
        same.rollout_metrics(a)
    assert torch.equal(same.get_state(), st)
    env, _ = _make(gpu, "im_backlog", autoreset_mode="disabled")
    st = env.get_state()
    met = _metrics(env, 3.5)
    o = torch.empty((3, N, env.obs_dim), dtype=torch.int64, device=gpu)
    rc = env._lib.invsim_rollout_metrics(env._h, 3, None, o.data_ptr(), None, None, None, met.data_ptr(), env._stream())
    assert rc == -22 and "actions" in _capi.last_error(env._h)
    r = torch.empty((3, N), dtype=torch.float64, device=gpu)
    rc = env._lib.invsim_rollout_metrics(env._h, 3, a.data_ptr(), o.data_ptr(), r.data_ptr(), None, None,
                                         met.data_ptr(), env._stream())
    assert rc == -22 and "together" in _capi.last_error(env._h)
    assert env._lib.invsim_rollout_metrics(env._h, -1, a.data_ptr(), None, None, None, None, None, env._stream()) == -22
    assert env._lib.invsim_rollout_metrics(env._h, 0, None, None, None, None, None, None, env._stream()) == 0
    assert torch.equal(env.get_state(), st) and bool((met == 3.5).all())
    # a lock-step DISABLED env: K that crosses the horizon, then a step at the horizon
    T = env._horizon()
    acts = _random_actions(env, T + 2, edge=False)
    env.rollout_metrics(acts[:T - 2], metrics=met)
    st, m0 = env.get_state(), met.clone()
    with pytest.raises(IndexError):
        env.rollout_metrics(acts[T - 2:T + 1], metrics=met)
    assert torch.equal(env.get_state(), st), "refused on the host: nothing ran"
    _same(met, m0, "metrics untouched")
    env.rollout_metrics(acts[T - 2:T], metrics=met)
    st, m0 = env.get_state(), met.clone()
    with pytest.raises(IndexError):
        env.rollout_metrics(acts[T:T + 1], metrics=met)
    assert torch.equal(env.get_state(), st) and env.status() == 0
    _same(met, m0, "metrics untouched at the horizon")
    assert bool((met[:, 1] == 3.5 + T).all())


# ---------------------------------------------------------------- 8. closed loop
class _Actor(torch.nn.Module):
    """O -> 16 -> A, tanh, its outputs stretched over more than the action range
    (so the clip works on both sides)"""

    def __init__(self, obs_dim, high, obs_scale):
        super().__init__()
        self.body = torch.nn.Sequential(torch.nn.Linear(obs_dim, 16), torch.nn.Tanh(), torch.nn.Linear(16, len(high)),
                                        torch.nn.Tanh())
        self.register_buffer("high", torch.as_tensor(np.asarray(high, np.float32)))
        self.obs_scale = obs_scale

    def forward(self, o):
        return self.high * (0.5 + 1.5 * self.body(o * self.obs_scale))


@pytest.mark.parametrize("name", ["im_backlog", "nv"])
def test_closed_loop_torch_actor(gpu, oracle, name):
    import invsim
    from invsim.policies import TorchPolicyAgent, convert_actions
    fam, kw, okw = CASES[name]
    env, obs0 = _make(gpu, name, seed=0, autoreset_mode="disabled")
    T = env._horizon()
    torch.manual_seed(0)
    net = _Actor(env.obs_dim, env._action_high(), 0.01 if fam == "im" else 0.02).to(gpu)
    agent = TorchPolicyAgent(net, name="Actor")
    met = _metrics(env)
    out = env.rollout_policy(agent, T, obs=True, actions=True, metrics=met, obs0=obs0)
    sp = env.single_action_space
    low, high = torch.as_tensor(sp.low, device=gpu), torch.as_tensor(sp.high, device=gpu)
    acts = out["actions"]
    assert acts.dtype == env.act_dtype and tuple(acts.shape) == (T, N, env.action_dim)
    with torch.no_grad():
        for k in range(T):
            src = obs0 if k == 0 else out["obs"][k - 1]
            _same(acts[k], convert_actions(net(src.to(torch.float32)), low, high, env.act_dtype).reshape(N, -1),
                  f"recorded action of step {k}")
    assert bool((acts == low).any()) and bool((acts == high).any()), "the clip works on both sides"
    assert bool(((acts > low) & (acts < high)).any())
    # the oracle, stepped with the recorded actions
    if fam == "im":
        orc = oracle.OracleInvMgmt(N, **okw)
    else:
        orc = oracle.OracleNewsvendor(N, **okw)
    orc.seed(range(0, N))
    _same_np(obs0, orc.reset(), "obs0")
    sums, e_rew, e_obs = (model.sums_invmgmt if fam == "im" else model.sums_newsvendor)(orc, acts.cpu().numpy())
    _same_np(out["reward"], e_rew, "reward == oracle")
    _same_np(out["obs"], e_obs, "obs == oracle")
    _same_np(met, sums, "metrics == oracle sums")
    assert bool(out["truncated"][T - 1].all())
    # evaluate_agent takes the agent unchanged
    cfg = dict(kw)
    cfg.pop("backlog", None)
    res = invsim.evaluate_agent(agent, type(env), cfg, n_episodes=N, seed_offset=0, device=gpu)
    cols = invsim.policies.summarize(env.family, sums)
    assert res["Agent"] == ["Actor"] * N and res["Seed"].tolist() == list(range(N))
    for k, v in cols.items():
        assert np.array_equal(np.asarray(res[k]), np.asarray(v)), k
    # the chain continues from the last row: 3 + (T - 3) steps == T steps
    env2, o0 = _make(gpu, name, seed=0, autoreset_mode="disabled")
    m2 = _metrics(env2)
    p1 = env2.rollout_policy(agent, 3, obs=True, metrics=m2, obs0=o0)
    p2 = env2.rollout_policy(agent, T - 3, obs=True, metrics=m2, obs0=p1["obs"][-1])
    _same(torch.cat([p1["reward"], p2["reward"]]), out["reward"], "chained closed loop")
    _same(m2, met, "chained metrics")
    with pytest.raises(ValueError, match="obs0"):
        env2.rollout_policy(agent, 2)
