"""The in-library MLP actor (include/invsim.h "MLP actor"): invsim_mlp_actions
against the CPU restatement of the arithmetic contract (tests/mlp_model.py), bit
for bit for ReLU / linear networks and within the float32 restatement's own
error for tanh ones; invsim_rollout_mlp against the single launch and against
a replay of its recorded actions through invsim_rollout_metrics on a twin env;
chained calls, optional outputs, both demand streams, per-env periods, the
episode sink, refusals, graph capture and evaluate_agent.

Shapes: N = 197 is three full 64-env waves and a partial one (the single launch
also runs N = 1 and N = 65); the horizons are short (InvMgmt periods = 7,
Newsvendor step_limit = 6, NetInvMgmt num_periods = 6) and K = 17 under
NEXT_STEP autoreset, so two episode ends and their reset steps fall inside one
call.  Widths: [64, 64]; [] (one linear layer); [5] (no multiple of the 4-unit
chunk or of the 4 waves); [256] * 4 (both limits); [3, 200] (unequal: the LDS
buffers follow the widest, 200 = 12 chunks of 16 and 2 of 4).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import mlp_model
import net_graphs

pytestmark = pytest.mark.gpu

N, K = 197, 17
SEED = 400
UNKNOWN = 0xFFFFFFFF          # invsim_position's low word when the periods differ per env
F32 = np.float32

CASES = {
    "im_backlog": ("im", dict(periods=7, backlog=True)),
    "im_lostsales": ("im", dict(periods=7, backlog=False)),
    "nv": ("nv", dict(step_limit=6)),
    "net_default": ("net", dict(graph="default", num_periods=6, backlog=True)),
    "net_mixed": ("net", dict(graph="mixed", num_periods=6, backlog=True)),
}
WIDTHS = {"64x64": [64, 64], "linear": [], "5": [5], "256x4": [256] * 4, "3x200": [3, 200]}


def _cls_kw(name):
    import invsim
    fam, kw = CASES[name]
    kw = dict(kw)
    if fam == "im":
        cls = invsim.InvManagementBacklogEnv if kw.pop("backlog") else invsim.InvManagementLostSalesEnv
    elif fam == "nv":
        cls = invsim.NewsvendorEnv
    else:
        from invsim.topology import default_graph
        cls = invsim.NetInvMgmtMasterEnv
        kw["graph"] = default_graph() if kw["graph"] == "default" else net_graphs.mixed(net_graphs.by_name, 6)
    return cls, kw


def _make(gpu, name, n=N, seed=SEED, **vec):
    """(env, obs0): a freshly seeded and reset device env of the case"""
    cls, kw = _cls_kw(name)
    env = cls(n, device=gpu, **kw, **vec)
    obs0, _ = env.reset(seed=seed)
    return env, obs0


def _metrics(env):
    import invsim
    return torch.zeros((env.num_envs, invsim.policies.metrics_dim(env)), dtype=torch.float64, device=env.device)


def _bits(t):
    t = t.detach().cpu() if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    if t.dtype == torch.float64:
        return t.view(torch.int64).numpy()
    if t.dtype == torch.float32:
        return t.view(torch.int32).numpy()
    return t.numpy()


def _same(a, b, what, nan_ok=False):
    """the same bits (nan_ok: a NaN equals any NaN, whose payload the contract leaves open)"""
    assert tuple(a.shape) == tuple(b.shape), f"{what}: {tuple(a.shape)} vs {tuple(b.shape)}"
    x, y = _bits(a), _bits(b)
    assert x.dtype == y.dtype, f"{what}: {x.dtype} vs {y.dtype}"
    ne = x != y
    if nan_ok:
        fa = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
        fb = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else b
        ne &= ~(np.isnan(fa) & np.isnan(fb))
    if ne.any():
        pytest.fail(f"{what}: {int(ne.sum())} of {ne.size} differ, first at {np.argwhere(ne)[:4].tolist()}")


def _same_out(a, b, what, keys=("obs", "reward", "terminated", "truncated")):
    for k in keys:
        _same(a[k], b[k], f"{what}: {k}")


def _bounds(env):
    sp = env.single_action_space
    return (np.asarray(sp.low, dtype=sp.dtype).reshape(-1), np.asarray(sp.high, dtype=sp.dtype).reshape(-1))


def _np_act(env):
    return np.int64 if env.act_dtype == torch.int64 else np.float32


def _agent(env, widths, seed=0, activation="relu", out_activation=None, bias=True, in_scale=True, out_scale=True,
           clip=True, name="MLP"):
    """a random network O -> widths -> A whose rescaled outputs cross both action bounds"""
    import invsim
    rng = np.random.default_rng(seed)
    dims = [env.obs_dim] + list(widths) + [env.action_dim]
    layers = []
    for i, o in zip(dims[:-1], dims[1:]):
        w = (rng.standard_normal((o, i)) / np.sqrt(i)).astype(F32)
        layers.append((w, (rng.standard_normal(o) * 0.25).astype(F32) if bias else None))
    high = _bounds(env)[1].astype(np.float64)
    high = np.where(np.isfinite(high), high, 1000.0)
    kw = {}
    if in_scale:
        kw["in_scale"] = (0.01 * (1 + 0.1 * rng.standard_normal(dims[0]))).astype(F32)
        kw["in_shift"] = (0.1 * rng.standard_normal(dims[0])).astype(F32)
    if out_scale:
        kw["out_scale"] = (1.5 * high).astype(F32)
        kw["out_shift"] = (0.5 * high).astype(F32)
    return invsim.MLPPolicyAgent(layers, activation=activation, out_activation=out_activation, clip=clip, name=name, **kw)


def _stretch(env, agent, obs):
    """give `agent` (built without an output scale, not yet on the device) the output
    scale and shift that put the 20th / 80th percentile of each of its outputs on `obs`
    at low - w / 4 / high + w / 4, w = high - low (an infinite bound counts as 1000):
    a fifth of the batch lies below the lower bound and a fifth above the upper one"""
    y = mlp_model.forward(agent, obs.cpu().numpy()).astype(np.float64)
    lo, hi = (b.astype(np.float64) for b in _bounds(env))
    hi = np.where(np.isfinite(hi), hi, 1000.0)
    y20, y80 = np.percentile(y, 20, axis=0), np.percentile(y, 80, axis=0)
    assert (y80 > y20).all(), "every output varies over the batch"
    scale = 1.5 * (hi - lo) / (y80 - y20)
    agent.out_scale = scale.astype(F32)
    agent.out_shift = (lo - (hi - lo) / 4 - y20 * scale).astype(F32)
    return agent


def _obs(env, seed=1):
    """synthetic observations of the env's dtype: int64 ones include values float32 cannot hold"""
    rng = np.random.default_rng(seed)
    n, O = env.num_envs, env.obs_dim
    if env.obs_dtype == torch.int64:
        o = rng.integers(0, 400, (n, O))
        o[::23, 1] = 2 ** 24 + 1            # rounds to even
        o[::29, 2] = 2 ** 24 + 3            # rounds up
        o[::31, 0] = -(2 ** 40) - 2 ** 15 - 1
        return torch.from_numpy(o).to(env.device)
    return torch.from_numpy(rng.uniform(0, 400, (n, O)).astype(F32)).to(env.device)


def _expect(env, agent, obs, tanh=np.tanh):
    """(raw, actions) of the CPU restatement"""
    raw = mlp_model.forward(agent, obs.cpu().numpy(), tanh=tanh)
    low, high = _bounds(env)
    return raw, mlp_model.convert(raw, low, high, _np_act(env), agent.clip)


# ---------------------------------------------------------------- 1. single launch, exact
SINGLE = [(name, w, N) for name in ("im_backlog", "nv", "net_default") for w in WIDTHS] + [
    (name, w, n) for name in ("im_backlog", "nv") for w in ("64x64", "5") for n in (1, 65)]


@pytest.mark.parametrize("name,widths,n", SINGLE)
def test_single_launch_bit_exact(gpu, name, widths, n):
    """ReLU and linear networks: raw and actions equal the restatement bit for bit"""
    env, _ = _make(gpu, name, n)
    obs = _obs(env)
    low, high = _bounds(env)
    # everything on; the outputs stretched past both bounds (one env has no spread to stretch)
    full = _stretch(env, _agent(env, WIDTHS[widths], seed=3, out_scale=False), obs) if n > 1 else _agent(
        env, WIDTHS[widths], seed=3)
    bare = _agent(env, WIDTHS[widths], seed=4, bias=False, in_scale=False, out_scale=False, clip=False)
    for what, agent in (("bias, scales, clip", full), ("no bias, no scales, no clip", bare)):
        act, raw = env.mlp_actions(agent, obs, raw=True)
        e_raw, e_act = _expect(env, agent, obs)
        _same(raw, e_raw, f"{what}: raw")
        _same(act, e_act, f"{what}: actions")
        assert act.dtype == env.act_dtype and tuple(act.shape) == (n, env.action_dim)
    if n == N:
        act = env.mlp_actions(full, obs).cpu().numpy()
        fin = np.isfinite(high.astype(np.float64))
        assert (act == low).any(0).all() and (act[:, fin] == high[fin]).any(0).all(), "every output crosses both bounds"
        assert ((act > low) & (act < high)).any()


@pytest.mark.parametrize("name", ["im_backlog", "nv"])
def test_single_launch_edges(gpu, name):
    """NaN weights, -0.0 at a zero bound, and either output alone"""
    import invsim
    env, _ = _make(gpu, name)
    obs = _obs(env)
    A, O = env.action_dim, env.obs_dim
    i64 = env.act_dtype == torch.int64
    # a NaN in the last layer (the output is NaN) and in one hidden unit (ReLU gives +0.0)
    agent = _agent(env, [5], seed=6)
    agent.weights[1][0, 2] = np.nan
    agent.weights[0][4, 0] = np.nan
    act, raw = env.mlp_actions(agent, obs, raw=True)
    e_raw, e_act = _expect(env, agent, obs)
    assert np.isnan(e_raw[:, 0]).all() and (np.isfinite(e_raw[:, 1:]).all() if A > 1 else True)
    _same(raw, e_raw, "NaN weight: raw", nan_ok=True)
    _same(act, e_act, "NaN weight: actions", nan_ok=True)
    a0 = act[:, 0].cpu().numpy()
    assert (a0 == 0).all() if i64 else np.isnan(a0).all(), "int64: NaN -> 0; float32: NaN passes"
    # raw == -0.0 exactly: (-0.0) * x + (-0.0) for x > 0; the lower bound is 0
    neg0 = invsim.MLPPolicyAgent([(np.full((A, O), -0.0, F32), np.full(A, -0.0, F32))])
    pos = obs.abs() + 1
    act, raw = env.mlp_actions(neg0, pos, raw=True)
    assert np.signbit(raw.cpu().numpy()).all() and (raw == 0).all(), "raw is -0.0"
    _same(act, _expect(env, neg0, pos)[1], "-0.0: actions")
    assert (act == 0).all() and (i64 or not np.signbit(act.cpu().numpy()).any()), "a value equal to a bound becomes the bound"
    # raw alone and actions alone
    agent = _agent(env, [64, 64], seed=7)
    act, raw = env.mlp_actions(agent, obs, raw=True)
    obj = agent.device_object(env)
    a1, r1 = torch.full_like(act, 7), torch.full_like(raw, 7.0)
    assert env._lib.invsim_mlp_actions(env._h, obj, obs.data_ptr(), a1.data_ptr(), None, env._stream()) == 0
    assert env._lib.invsim_mlp_actions(env._h, obj, obs.data_ptr(), None, r1.data_ptr(), env._stream()) == 0
    _same(a1, act, "actions alone"), _same(r1, raw, "raw alone")


# ---------------------------------------------------------------- 2. single launch, tanh
@pytest.mark.parametrize("name", ["im_backlog", "nv", "net_default"])
@pytest.mark.parametrize("kind", ["hidden", "squashed"])
def test_single_launch_tanh(gpu, name, kind):
    """tanh networks are defined up to the device's tanhf.  Actions are exactly
    the conversion of the kernel's own raw outputs; raw is held against a
    float64 evaluation F64 of the same network: with d_ref = max |R32 - F64|
    (R32 = the float32 restatement with numpy's tanh, computed here), the
    kernel must satisfy max |raw - F64| <= 4 d_ref: both are float32
    evaluations of one graph in one accumulation order and differ in the last
    ulps of tanhf only, while a wrong index, a missing bias or swapped layers
    are five or more orders above d_ref."""
    env, _ = _make(gpu, name)
    obs = _obs(env)
    agent = _agent(env, [64, 64], seed=8, activation="tanh", out_activation="tanh" if kind == "squashed" else None,
                   out_scale=kind == "squashed" or name != "im_backlog")
    act, raw = env.mlp_actions(agent, obs, raw=True)
    low, high = _bounds(env)
    _same(act, mlp_model.convert(raw.cpu().numpy(), low, high, _np_act(env), True), "actions == convert(kernel raw)",
          nan_ok=True)
    o = obs.cpu().numpy()
    f64 = mlp_model.forward_f64(agent, o)
    d_ref = float(np.abs(mlp_model.forward(agent, o).astype(np.float64) - f64).max())
    d_gpu = float(np.abs(raw.cpu().numpy().astype(np.float64) - f64).max())
    print(f"tanh {name} {kind}: d_ref = {d_ref:.6e}  kernel = {d_gpu:.6e}  scale = {float(np.abs(f64).max()):.4e}")
    assert d_ref > 0
    assert d_gpu <= 4 * d_ref, (d_gpu, d_ref)


# ---------------------------------------------------------------- 3. closed loop
def _loop_agent(env, seed=11):
    return _agent(env, [64, 64], seed=seed)


def _closed_loop(gpu, name, **vec):
    """K steps in one invsim_rollout_mlp call with every output, checked against the
    single launch, the restatement and a replay of the recorded actions on a twin"""
    (env, obs0), (twin, _) = (_make(gpu, name, record_demand=True, record_info=True, **vec) for _ in range(2))
    agent = _loop_agent(env)
    met, met2 = _metrics(env), _metrics(twin)
    out = env.rollout_policy(agent, K, obs=True, actions=True, metrics=met, obs0=obs0)
    T = env._horizon()
    assert bool(out["truncated"][T - 1].all()) and bool((out["reward"][T] == 0).all()), "a reset step is crossed"
    assert bool((met[:, 1] == K - 2).all()), "two reset steps add nothing"
    acts = out["actions"]
    assert acts.dtype == env.act_dtype and tuple(acts.shape) == (K, env.num_envs, env.action_dim)
    for k in range(K):
        src = obs0 if k == 0 else out["obs"][k - 1]
        _same(acts[k], env.mlp_actions(agent, src), f"recorded action of step {k} == the single launch")
        _same(acts[k], _expect(env, agent, src)[1], f"recorded action of step {k} == the restatement")
    rep = twin.rollout_metrics(acts, metrics=met2)
    _same_out(rep, out, "replay")
    _same(met2, met, "metrics")
    assert torch.equal(env.get_state(), twin.get_state()), "state blob"
    _same(env._demand, twin._demand, "info_demand")
    _same(env._rec, twin._rec, "info record")
    return agent, out, met, env.get_state()


@pytest.mark.parametrize("name", list(CASES))
def test_closed_loop(gpu, name):
    agent, full, met, state = _closed_loop(gpu, name)
    a = full["actions"].cpu().numpy()
    assert (a.min((0, 1)) < a.max((0, 1))).any(), "the policy is not a constant"
    # 5 + 12 steps in two calls
    env, obs0 = _make(gpu, name)
    m = _metrics(env)
    p1 = env.rollout_policy(agent, 5, obs=True, actions=True, metrics=m, obs0=obs0)
    p2 = env.rollout_policy(agent, 12, obs=True, actions=True, metrics=m, obs0=p1["obs"][-1])
    _same_out({k: torch.cat([p1[k], p2[k]]) for k in full}, full, "5 + 12 == 17", keys=tuple(full))
    _same(m, met, "metrics 5 + 12")
    assert torch.equal(env.get_state(), state)
    # obs, the reward triple and actions NULL in turn (the loop then runs on the object's scratch rows)
    for kw in (dict(obs=False, actions=True), dict(obs=True, rewards=False, actions=True), dict(obs=True, actions=False),
               dict(obs=False, rewards=False, actions=False)):
        env, obs0 = _make(gpu, name)
        m = _metrics(env)
        part = env.rollout_policy(agent, K, metrics=m, obs0=obs0, **kw)
        _same_out(part, full, str(kw), keys=tuple(part))
        _same(m, met, f"metrics with {kw}")
        assert torch.equal(env.get_state(), state), kw
    with pytest.raises(ValueError, match="obs0"):
        env.rollout_policy(agent, 2)


@pytest.mark.parametrize("name", ["im_backlog", "nv"])
def test_closed_loop_philox(gpu, name):
    _closed_loop(gpu, name, demand_stream="philox")


@pytest.mark.parametrize("name", list(CASES))
def test_closed_loop_per_env_periods(gpu, name):
    """after a masked reset of half the envs mid-episode the loop equals the replay on a twin"""
    (env, obs0), (twin, _) = _make(gpu, name), _make(gpu, name)
    agent = _loop_agent(env)
    met, met2 = _metrics(env), _metrics(twin)
    mask = torch.arange(N, device=gpu) % 2 == 0
    first = env.rollout_policy(agent, 3, obs=True, actions=True, metrics=met, obs0=obs0)
    r_obs, _ = env.reset(options={"reset_mask": mask})
    assert env.position() & UNKNOWN == UNKNOWN, "per-env periods after the mask"
    cur = torch.where(mask[:, None], r_obs, first["obs"][-1])
    out = env.rollout_policy(agent, K, obs=True, actions=True, metrics=met, obs0=cur)
    _same(out["actions"][0], env.mlp_actions(agent, cur), "first action after the masked reset")
    twin.rollout_metrics(first["actions"], metrics=met2)
    twin.reset(options={"reset_mask": mask})
    rep = twin.rollout_metrics(out["actions"], metrics=met2)
    _same_out(rep, out, "staggered replay")
    _same(met2, met, "metrics")
    assert torch.equal(env.get_state(), twin.get_state())
    T = env._horizon()
    r0 = out["reward"][T - 3]                       # the unreset envs' reset step; the reset ones step
    assert bool((r0[1::2] == 0).all()) and bool((r0[0::2] != 0).any())


@pytest.mark.parametrize("name", ["im_backlog", "nv", "net_default"])
def test_episode_sink_equals_fold(gpu, name):
    """with EpisodeStats attached, ret / part equal invsim_episode_fold_groups over the output rows"""
    from invsim import _capi
    from invsim.distributed import EpisodeStats
    (a, oa0), (b, ob0) = _make(gpu, name), _make(gpu, name)
    agent = _loop_agent(a)
    sa, sb = EpisodeStats(N, gpu), EpisodeStats(N, gpu)
    sa.attach(a)
    ma, mb = _metrics(a), _metrics(b)
    for k in (K, 1, 5):
        oa = a.rollout_policy(agent, k, obs=True, metrics=ma, obs0=oa0)
        ob = b.rollout_policy(agent, k, obs=True, metrics=mb, obs0=ob0)
        oa0, ob0 = oa["obs"][-1], ob["obs"][-1]
        _same_out(oa, ob, "the sink changes no output")
        sb.update_block(ob["reward"].contiguous(), ob["terminated"].contiguous(), ob["truncated"].contiguous())
        torch.cuda.synchronize()
        _same(sa.ret, sb.ret, f"running returns after {k} steps")
        _same(sa.part, sb.part, f"group partials after {k} steps")
    _same(ma, mb, "metrics")
    assert float(sa.acc[2]) == 3 * N, "three episode ends folded"
    st = a.get_state()
    with pytest.raises(_capi.InvsimError, match=r"\(-22\)"):      # the sink folds the reward outputs
        a.rollout_policy(agent, 2, rewards=False, obs0=oa0)
    assert torch.equal(a.get_state(), st)


# ---------------------------------------------------------------- 4. refusals
def test_refusals_leave_the_state_alone(gpu):
    from invsim import _capi
    env, obs0 = _make(gpu, "im_backlog", autoreset_mode="disabled")
    other, _ = _make(gpu, "im_backlog", autoreset_mode="disabled")
    agent = _loop_agent(env)
    obj, obj_other = agent.device_object(env), agent.device_object(other)
    assert obj.value != obj_other.value and agent.device_object(env) is obj, "one object per env, built once"
    lib, s = env._lib, env._stream()
    met = _metrics(env) + 3.5
    st = env.get_state()
    acts = torch.zeros((3, N, 3), dtype=torch.int64, device=gpu)
    args = (None, None, None, None, acts.data_ptr(), met.data_ptr(), s)
    assert lib.invsim_rollout_mlp(env._h, 3, obj, None, *args) == -22 and "obs0" in _capi.last_error(env._h)
    assert lib.invsim_rollout_mlp(env._h, 3, obj_other, obs0.data_ptr(), *args) == -22
    assert "another handle" in _capi.last_error(env._h)
    assert lib.invsim_mlp_actions(env._h, obj_other, obs0.data_ptr(), acts.data_ptr(), None, s) == -22
    assert lib.invsim_rollout_mlp(env._h, -1, obj, obs0.data_ptr(), *args) == -22
    assert lib.invsim_rollout_mlp(env._h, 0, obj, None, *args) == 0
    r = torch.empty((3, N), dtype=torch.float64, device=gpu)
    assert lib.invsim_rollout_mlp(env._h, 3, obj, obs0.data_ptr(), None, r.data_ptr(), None, None, None, None, s) == -22
    assert "together" in _capi.last_error(env._h)
    assert torch.equal(env.get_state(), st) and bool((met == 3.5).all()) and bool((acts == 0).all())
    # DISABLED autoreset, K past the horizon: refused for all K steps before the first launch
    T = env._horizon()
    first = env.rollout_policy(agent, T - 2, obs=True, metrics=met, obs0=obs0)
    st, m0 = env.get_state(), met.clone()
    with pytest.raises(IndexError):
        env.rollout_policy(agent, 3, metrics=met, obs0=first["obs"][-1])
    assert torch.equal(env.get_state(), st) and env.status() == 0, "refused on the host: nothing ran"
    _same(met, m0, "metrics untouched")
    env.rollout_policy(agent, 2, metrics=met, obs0=first["obs"][-1])
    assert bool((met[:, 1] == 3.5 + T).all())
    # SAME_STEP
    same, o_same = _make(gpu, "im_backlog", autoreset_mode="same_step")
    st = same.get_state()
    with pytest.raises(_capi.InvsimError, match=r"\(-22\)"):
        same.rollout_policy(agent, 3, obs0=o_same)
    assert torch.equal(same.get_state(), st)
    # create and destroy inside a capture bracket
    nd, o_nd = _make(gpu, "im_backlog")
    known = _loop_agent(nd, seed=12)
    k_obj = known.device_object(nd)
    before = nd.mlp_actions(known, o_nd)
    st = nd.get_state()
    _capi.check(lib.invsim_capture_begin(nd._h), nd._h, "capture_begin")
    try:
        with pytest.raises(_capi.InvsimError, match=r"\(-22\)"):
            _loop_agent(nd, seed=13).device_object(nd)
        lib.invsim_mlp_destroy(k_obj)
        assert "mlp_destroy" in _capi.last_error(nd._h), "refused: the object stays valid"
    finally:
        steps = C.c_int64(-1)
        assert lib.invsim_capture_end(nd._h, C.byref(steps)) == 0 and steps.value == 0
    assert torch.equal(nd.get_state(), st)
    _same(nd.mlp_actions(known, o_nd), before, "the object survived the refused destroy")
    # per-env periods with DISABLED autoreset: the status word is read once, after the loop
    mask = torch.arange(N, device=gpu) % 2 == 0
    r_obs, _ = other.reset(options={"reset_mask": mask})         # `other` is at period 0: every env stays there
    o1 = other.rollout_policy(agent, T, obs=True, obs0=r_obs)
    with pytest.raises(IndexError):
        other.rollout_policy(agent, 2, obs0=o1["obs"][-1])
    assert other.status() == 0, "the call cleared the status word it reported"


def test_create_validation(gpu):
    """invsim_mlp_create checks the spec on the host: dimension and layer-count
    violations are INVSIM_ERANGE, everything else INVSIM_EINVAL"""
    from invsim import _capi
    env, _ = _make(gpu, "im_backlog", 4)
    O, A = env.obs_dim, env.action_dim
    low, high = _bounds(env)

    def create(dims, act=1, out_act=0, clip=1, in_scale=True, in_shift=True, bounds=True, n=None):
        n = len(dims) - 1 if n is None else n
        ws = [np.zeros((max(o, 1), max(i, 1)), F32) for i, o in zip(dims[:-1], dims[1:])]
        W = (C.c_void_p * len(ws))(*[w.ctypes.data for w in ws])
        d = np.asarray(dims, np.int32)
        sc = np.ones(O, F32)
        spec = _capi.MLPSpec(n, act, out_act, clip, d.ctypes.data, C.cast(W, C.c_void_p), None,
                             sc.ctypes.data if in_scale else None, sc.ctypes.data if in_shift else None, None, None,
                             low.ctypes.data if bounds else None, high.ctypes.data if bounds else None)
        obj = C.c_void_p()
        rc = env._lib.invsim_mlp_create(env._h, C.byref(spec), C.byref(obj))
        if rc == 0:
            env._mlps.append(obj)
        else:
            assert not obj.value
        return rc

    assert create([O, 8, A]) == 0 and create([O, A]) == 0 and create([O, 256, 1, A]) == 0
    assert create([O, 4, 4, 4, 4, A]) == 0
    for dims in ([O, 4, 4, 4, 4, 4, A], [O + 1, 8, A], [O, 8, A + 1], [O, 257, A], [O, 0, A]):
        assert create(dims) == -34, dims
    assert create([O, A], n=0) == -34
    assert create([O, 8, A], act=0) == -22 and create([O, 8, A], act=3) == -22
    assert create([O, A], act=0) == 0, "the hidden kind is ignored without a hidden layer"
    assert create([O, 8, A], out_act=1) == -22
    assert create([O, 8, A], in_shift=False) == -22 and create([O, 8, A], in_scale=False) == -22
    assert create([O, 8, A], bounds=False) == -22 and create([O, 8, A], bounds=False, clip=0) == 0
    assert env._lib.invsim_mlp_create(env._h, None, None) == -22


# ---------------------------------------------------------------- 5. capture
@pytest.mark.parametrize("name", ["im_lostsales", "net_default"])
def test_graph_of_closed_loop(gpu, name):
    """one episode cycle (horizon + 1 steps under NEXT_STEP) captured and replayed twice == three eager calls"""
    (env, o_g), (twin, o_e) = _make(gpu, name), _make(gpu, name)
    agent = _loop_agent(env)
    Cy = env._horizon() + 1
    m_g, m_e = _metrics(env), _metrics(twin)
    o_g, o_e = o_g.clone(), o_e.clone()

    def loop(e, o, m):
        def fn():
            out = e.rollout_policy(agent, Cy, obs=True, actions=True, metrics=m, obs0=o)
            o.copy_(out["obs"][-1])
            return out
        return fn
    g = env.capture(loop(env, o_g, m_g), warmup=1)
    assert g.steps == Cy
    eager = loop(twin, o_e, m_e)
    eager()
    for rep in range(2):
        og, oe = g.replay(), eager()
        torch.cuda.synchronize(gpu)
        _same_out(og, oe, f"replay {rep}", keys=("obs", "reward", "terminated", "truncated", "actions"))
        _same(m_g, m_e, f"metrics after replay {rep}")
    assert torch.equal(env.get_state(), twin.get_state()) and env.position() == twin.position()
    assert bool((m_g[:, 1] == 3 * (Cy - 1)).all())


# ---------------------------------------------------------------- 6. evaluate_agent
@pytest.mark.parametrize("name", ["im_backlog", "nv", "net_default"])
def test_evaluate_agent(gpu, name):
    import invsim
    cls, cfg = _cls_kw(name)
    (env, obs0), (twin, _) = (_make(gpu, name, seed=0, autoreset_mode="disabled") for _ in range(2))
    agent = _agent(env, [64, 64], seed=11, name="Actor")
    T = env._horizon()
    met = _metrics(twin)
    out = env.rollout_policy(agent, T, actions=True, obs0=obs0)
    twin.rollout_metrics(out["actions"], metrics=met)                 # the replay's metrics
    res = invsim.evaluate_agent(agent, cls, cfg, n_episodes=N, seed_offset=0, device=gpu)
    cols = invsim.policies.summarize(env.family, met.cpu().numpy())
    assert res["Agent"] == ["Actor"] * N and res["Seed"].tolist() == list(range(N))
    for k, v in cols.items():
        assert np.array_equal(np.asarray(res[k]), np.asarray(v)), k
    assert (np.asarray(res["Steps"]) == T).all()
    import pandas as pd
    table = invsim.policies.summary_table([res, invsim.evaluate_agent(invsim.ConstantOrderAgent(0.1), cls, cfg,
                                                                      n_episodes=N, device=gpu)])
    assert isinstance(table, pd.DataFrame) and "Actor" in table.index and len(table) == 2
    assert table.loc["Actor", "AvgReward"] == pytest.approx(float(np.mean(cols["TotalReward"])), rel=1e-12)
