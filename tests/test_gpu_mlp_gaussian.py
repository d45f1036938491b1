"""The Gaussian MLP actor on the device (include/invsim.h "Gaussian MLP actor"):
invsim_mlp_sample and invsim_rollout_mlp_sample against tests/mlp_model.py for
the mean, numpy's own standard_normal for the noise and the float32
restatement of the two formulas (tests/gaussian_model.py), bit for bit.

Shapes: N = 1024 (16 workgroups) and one ragged N = 1000; ReLU networks with
hidden [16] and [64, 64].  Every case takes its normals through
gaussian_model.normals, whose table of seeds and draw counts the CPU test
(tests/test_mlp_gaussian.py) checks against the restated draw.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import gaussian_model as gm
import mlp_model
import net_graphs

pytestmark = pytest.mark.gpu

N = gm.N
SEED = 400                    # demand seed
F32 = np.float32
KEYS = ("obs", "reward", "terminated", "truncated", "actions", "raw_actions", "log_prob")


def _cls_kw(name):
    import invsim
    if name == "im":
        return invsim.InvManagementBacklogEnv, {}
    if name == "im7":
        return invsim.InvManagementBacklogEnv, dict(periods=7)
    if name == "im5":
        return invsim.InvManagementBacklogEnv, dict(periods=5)
    if name == "nv":
        return invsim.NewsvendorEnv, dict(step_limit=6)
    from invsim.topology import default_graph
    graph = default_graph() if name == "net" else net_graphs.mixed(net_graphs.by_name, 6)
    return invsim.NetInvMgmtMasterEnv, dict(graph=graph, num_periods=6, backlog=True)


def _make(gpu, name, n=N, **vec):
    cls, kw = _cls_kw(name)
    env = cls(n, device=gpu, **kw, **vec)
    obs0, _ = env.reset(seed=SEED)
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


def _same(a, b, what):
    assert tuple(a.shape) == tuple(b.shape), f"{what}: {tuple(a.shape)} vs {tuple(b.shape)}"
    x, y = _bits(a), _bits(b)
    assert x.dtype == y.dtype, f"{what}: {x.dtype} vs {y.dtype}"
    ne = x != y
    if ne.any():
        pytest.fail(f"{what}: {int(ne.sum())} of {ne.size} differ, first at {np.argwhere(ne)[:4].tolist()}")


def _same_out(a, b, what, keys):
    for k in keys:
        _same(a[k], b[k], f"{what}: {k}")


def _bounds(env):
    sp = env.single_action_space
    return (np.asarray(sp.low, dtype=sp.dtype).reshape(-1), np.asarray(sp.high, dtype=sp.dtype).reshape(-1))


def _np_act(env):
    return np.int64 if env.act_dtype == torch.int64 else np.float32


def _params(env, widths, seed):
    """a random ReLU-sized network O -> widths -> A whose rescaled outputs cross both
    action bounds, and a log_std that puts the noise at a fifth of the action range"""
    rng = np.random.default_rng(seed)
    dims = [env.obs_dim] + list(widths) + [env.action_dim]
    layers = [((rng.standard_normal((o, i)) / np.sqrt(i)).astype(F32), (rng.standard_normal(o) * 0.25).astype(F32))
              for i, o in zip(dims[:-1], dims[1:])]
    high = _bounds(env)[1].astype(np.float64)
    high = np.where(np.isfinite(high), high, 1000.0)
    kw = dict(in_scale=(0.01 * (1 + 0.1 * rng.standard_normal(dims[0]))).astype(F32),
              in_shift=(0.1 * rng.standard_normal(dims[0])).astype(F32),
              out_scale=(1.5 * high).astype(F32), out_shift=(0.5 * high).astype(F32))
    log_std = np.log(0.2 * high * (1 + 0.1 * rng.random(dims[-1]))).astype(F32)
    return layers, log_std, kw


def _agent(env, widths=(16,), seed=11, aseed=0, activation="relu", log_std=None):
    import invsim
    layers, ls, kw = _params(env, widths, seed)
    return invsim.GaussianMLPPolicyAgent(layers, log_std=ls if log_std is None else log_std, seed=aseed,
                                         activation=activation, **kw)


def _arng(env, n=None):
    """the attached generators' rows [4, n] as uint64"""
    return env._arng[:, :env.num_envs if n is None else n].cpu().numpy().view(np.uint64)


def _expect(env, agent, src, z):
    """(mean, raw, log_prob, actions) of the contract for obs `src` and normals z [n, A]"""
    mean = mlp_model.forward(agent, src.cpu().numpy())
    raw = gm.sample(mean, z, agent.std)
    low, high = _bounds(env)
    return mean, raw, gm.log_prob(z, agent.log_std), mlp_model.convert(raw, low, high, _np_act(env), agent.clip)


def _check_rows(env, agent, out, obs0, z, what):
    """every step's raw, log_prob and actions recomputed from the kernel's own obs rows"""
    A = env.action_dim
    K = out["actions"].shape[0]
    for k in range(K):
        src = obs0 if k == 0 else out["obs"][k - 1]
        _, raw, lp, act = _expect(env, agent, src, z[:, k * A:(k + 1) * A])
        _same(out["raw_actions"][k], raw, f"{what}: raw of step {k}")
        _same(out["log_prob"][k], lp, f"{what}: log_prob of step {k}")
        _same(out["actions"][k], act, f"{what}: actions of step {k}")


def _replay(twin, out, met):
    """the recorded actions through invsim_rollout_metrics on a twin without any sampling"""
    return twin.rollout_metrics(out["actions"], metrics=met)


# ---------------------------------------------------------------- 1. single launch
@pytest.mark.parametrize("name,widths,n", [("im", (64, 64), N), ("nv", (16,), N), ("net", (64, 64), N),
                                           ("im", (16,), 1000)])
def test_single_launch_bit_exact(gpu, name, widths, n):
    env, obs = _make(gpu, name, n)
    A = env.action_dim
    agent = _agent(env, widths, seed=3, aseed=7)
    obj = agent.device_object(env)
    start = env.action_rng_state()
    _same(_arng(env), gm.state_rows(7, 0, n, 0), "seeded generators")
    got = env.mlp_sample(agent, obs)
    mean, raw, lp, act = _expect(env, agent, obs, gm.normals(7, 0, n, A))
    _same(got["mean"], mean, "mean"), _same(got["raw_actions"], raw, "raw")
    _same(got["log_prob"], lp, "log_prob"), _same(got["actions"], act, "actions")
    _same(got["mean"], env.mlp_actions(agent, obs, raw=True)[1], "mean == invsim_mlp_actions' raw")
    assert got["actions"].dtype == env.act_dtype and tuple(got["log_prob"].shape) == (n,)
    low, high = _bounds(env)
    a = got["actions"].cpu().numpy()
    assert ((a == low) | (a == high)).any() and ((a > low) & (a < high)).any(), "samples at a bound and inside"
    _same(_arng(env), gm.state_rows(7, 0, n, A), "generators after A normals")
    after = env._arng.clone()
    npad = start.shape[1]
    assert torch.equal(after[:, n:], start[:, n:]) and torch.equal(after[2:], start[2:]), "lanes past N, increments"
    # each output alone == the same output requested together; guard rows past N stay untouched
    lib, s = env._lib, env._stream()
    bufs = {"actions": torch.full((npad + 1, A), 7, dtype=env.act_dtype, device=gpu),
            "raw_actions": torch.full((npad + 1, A), 7.0, dtype=torch.float32, device=gpu),
            "mean": torch.full((npad + 1, A), 7.0, dtype=torch.float32, device=gpu),
            "log_prob": torch.full((npad + 1,), 7.0, dtype=torch.float32, device=gpu)}
    for key in bufs:
        env._arng.copy_(start)
        ptr = {k: (bufs[k].data_ptr() if k == key else None) for k in bufs}
        assert lib.invsim_mlp_sample(env._h, obj, obs.data_ptr(), ptr["actions"], ptr["raw_actions"], ptr["mean"],
                                     ptr["log_prob"], s) == 0
        _same(bufs[key][:n], got[key], f"{key} alone")
        assert bool((bufs[key][n:] == 7).all()), f"{key}: rows past N"
        assert torch.equal(env._arng, after), f"{key} alone: the generators advance all the same"


def test_tanh_network(gpu):
    """a tanh network is defined up to the device's tanhf: the sample is exact around the kernel's own mean"""
    env, obs = _make(gpu, "im")
    agent = _agent(env, (64, 64), seed=8, aseed=7, activation="tanh")
    got = env.mlp_sample(agent, obs)
    z = gm.normals(7, 0, N, env.action_dim)
    raw = gm.sample(got["mean"].cpu().numpy(), z, agent.std)
    _same(got["raw_actions"], raw, "raw == fmaf(std, zf, kernel mean)")
    low, high = _bounds(env)
    _same(got["actions"], mlp_model.convert(raw, low, high, np.int64, True), "actions == convert(raw)")
    _same(got["log_prob"], gm.log_prob(z, agent.log_std), "log_prob")
    _same(got["mean"], env.mlp_actions(agent, obs, raw=True)[1], "mean == the deterministic launch")


# ---------------------------------------------------------------- 2. closed loop
def test_closed_loop_main(gpu):
    """InvMgmt Backlog, N = 1024, K = 24 from a reset (72 normals per env, every
    slow path of the ziggurat: tests/test_mlp_gaussian.py asserts the counts)"""
    import invsim
    m = gm.MAIN
    K, A = m["K"], m["A"]
    (env, obs0), (twin, obs0_t) = _make(gpu, "im"), _make(gpu, "im")
    assert env.action_dim == A and env.num_envs == m["n"]
    agent = _agent(env, aseed=m["seed"])
    met, met2 = _metrics(env), _metrics(twin)
    out = invsim.policies.collect_rollout(env, agent, K, obs0, metrics=met)
    assert sorted(out) == sorted(KEYS)
    _check_rows(env, agent, out, obs0, gm.normals(m["seed"], 0, N, K * A), "main")
    _same(_arng(env), gm.state_rows(m["seed"], 0, N, K * A), "generators after 72 normals")
    # == K single launches, each followed by a one-step invsim_rollout_metrics
    rows, cur = [], obs0_t
    for k in range(K):
        s = twin.mlp_sample(agent, cur)
        o = twin.rollout_metrics(s["actions"][None], metrics=met2)
        rows.append({**{kk: o[kk][0] for kk in ("obs", "reward", "terminated", "truncated")},
                     "actions": s["actions"], "raw_actions": s["raw_actions"], "log_prob": s["log_prob"]})
        cur = o["obs"][0]
    _same_out({k: torch.stack([r[k] for r in rows]) for k in KEYS}, out, "K single launches", KEYS)
    _same(met2, met, "metrics")
    assert torch.equal(env.get_state(), twin.get_state()), "state blob"
    assert torch.equal(env._arng, twin._arng)
    a = out["actions"].cpu().numpy()
    assert (a.std((0, 1)) > 0).all(), "the policy is not a constant"


def test_autoreset_next_step(gpu):
    """NEXT_STEP across two episode ends (periods = 5, K = 12): reset steps draw and record, metrics add nothing"""
    import invsim
    K = 12
    (env, obs0), (twin, _) = _make(gpu, "im5"), _make(gpu, "im5")
    agent = _agent(env)
    met, met2 = _metrics(env), _metrics(twin)
    out = invsim.policies.collect_rollout(env, agent, K, obs0, metrics=met)
    assert bool(out["truncated"][4].all()) and bool((out["reward"][5] == 0).all()) and bool((out["reward"][11] == 0).all())
    assert bool((met[:, 1] == K - 2).all()), "two reset steps add nothing"
    _check_rows(env, agent, out, obs0, gm.normals(0, 0, N, K * 3), "autoreset")
    _same(_arng(env), gm.state_rows(0, 0, N, K * 3), "generators: reset steps draw too")
    _same_out(_replay(twin, out, met2), out, "replay", KEYS[:4])
    _same(met2, met, "metrics")
    assert torch.equal(env.get_state(), twin.get_state())


def test_std_zero_equals_the_deterministic_loop(gpu):
    import invsim
    K = 12
    (env, obs0), (twin, obs0_t) = _make(gpu, "im5"), _make(gpu, "im5")
    agent = _agent(env, log_std=np.full(3, -200.0, F32))
    assert agent.std.tolist() == [0.0] * 3
    det = invsim.MLPPolicyAgent(list(zip(agent.weights, agent.biases)), activation="relu", in_scale=agent.in_scale,
                                in_shift=agent.in_shift, out_scale=agent.out_scale, out_shift=agent.out_shift)
    met, met2 = _metrics(env), _metrics(twin)
    out = invsim.policies.collect_rollout(env, agent, K, obs0, metrics=met)
    ref = twin.rollout_policy(det, K, obs=True, actions=True, metrics=met2, obs0=obs0_t)
    _same_out(out, ref, "std = 0", KEYS[:5])
    _same(met, met2, "metrics")
    assert torch.equal(env.get_state(), twin.get_state())
    _same(_arng(env), gm.state_rows(0, 0, N, K * 3), "the generators still advance by K * A normals")
    _same(out["log_prob"][3], gm.log_prob(gm.normals(0, 0, N, 3, skip=9), agent.log_std), "log_prob of step 3")


# ---------------------------------------------------------------- 3. streams, periods, graphs
def test_per_env_periods(gpu):
    """after a masked reset of half the envs mid-episode"""
    import invsim
    (env, obs0), (twin, _) = _make(gpu, "im7"), _make(gpu, "im7")
    agent = _agent(env)
    met, met2 = _metrics(env), _metrics(twin)
    mask = torch.arange(N, device=gpu) % 2 == 0
    first = invsim.policies.collect_rollout(env, agent, 3, obs0, metrics=met)
    r_obs, _ = env.reset(options={"reset_mask": mask})
    assert (env.position() & 0xFFFFFFFF) == 0xFFFFFFFF, "per-env periods after the mask"
    cur = torch.where(mask[:, None], r_obs, first["obs"][-1])
    K = 8
    out = invsim.policies.collect_rollout(env, agent, K, cur, metrics=met)
    _check_rows(env, agent, out, cur, gm.normals(0, 0, N, K * 3, skip=9), "staggered")
    _replay(twin, first, met2)
    twin.reset(options={"reset_mask": mask})
    _same_out(_replay(twin, out, met2), out, "staggered replay", KEYS[:4])
    _same(met2, met, "metrics")
    assert torch.equal(env.get_state(), twin.get_state())
    r0 = out["reward"][4]                       # the unreset envs' reset step (period 7); the reset ones step
    assert bool((r0[1::2] == 0).all()) and bool((r0[0::2] != 0).any())


@pytest.mark.parametrize("name", ["im7", "nv"])
def test_philox_demand_stream(gpu, name):
    """the action stream is PCG64 under the fast demand stream too, and `rng` and
    philox_step move exactly as in a replay without any sampling"""
    import invsim
    (env, obs0), (twin, _) = (_make(gpu, name, demand_stream="philox") for _ in range(2))
    A = env.action_dim
    agent = _agent(env)
    met, met2 = _metrics(env), _metrics(twin)
    K = 10
    out = invsim.policies.collect_rollout(env, agent, K, obs0, metrics=met)
    _check_rows(env, agent, out, obs0, gm.normals(0, 0, N, K * A), "philox")
    _same(_arng(env), gm.state_rows(0, 0, N, K * A), "action generators")
    _same_out(_replay(twin, out, met2), out, "replay", KEYS[:4])
    _same(met2, met, "metrics")
    assert torch.equal(env.get_state(), twin.get_state()), "state blob: rng rows and philox_step"
    assert env.demand_stream == "philox"


@pytest.mark.parametrize("name", ["net", "net_mixed"])
def test_net_graphs(gpu, name):
    """the default graph (specialised kernel) and a generic one"""
    import invsim
    (env, obs0), (twin, _) = _make(gpu, name), _make(gpu, name)
    A = env.action_dim
    K = min(5, gm.DRAWS[0] // A)
    assert K >= 2 and (env.kernel_variant == 0) == (name == "net_mixed")
    agent = _agent(env)
    met, met2 = _metrics(env), _metrics(twin)
    out = invsim.policies.collect_rollout(env, agent, K, obs0, metrics=met)
    _check_rows(env, agent, out, obs0, gm.normals(0, 0, N, K * A), name)
    _same(_arng(env), gm.state_rows(0, 0, N, K * A), "action generators")
    _same_out(_replay(twin, out, met2), out, "replay", KEYS[:4])
    _same(met2, met, "metrics")
    assert torch.equal(env.get_state(), twin.get_state())


# ---------------------------------------------------------------- 4. stream ownership, sharding
def test_stream_ownership_and_sharding(gpu):
    import invsim
    collect = invsim.policies.collect_rollout
    (env, obs0), (two, obs0_2) = _make(gpu, "im7"), _make(gpu, "im7")
    shard, obs0_s = _make(gpu, "im7", 512, global_offset=512)
    agent = _agent(env)
    full = collect(env, agent, 12, obs0)
    # 5 steps then 7 equal 12, with another agent's generators attached in between
    p1 = collect(two, agent, 5, obs0_2)
    two.seed_actions(99)
    p2 = collect(two, agent, 7, p1["obs"][-1])
    assert two._arng is agent._bufs[two], "the agent put its own buffer back"
    _same_out({k: torch.cat([p1[k], p2[k]]) for k in KEYS}, full, "5 + 7 == 12", KEYS)
    assert torch.equal(two._arng, env._arng) and torch.equal(two.get_state(), env.get_state())
    # a shard at global_offset = 512 reproduces envs 512 .. 1023 of the full batch
    _same(obs0_s, obs0[512:], "the shard's reset")
    part = collect(shard, agent, 12, obs0_s)
    _same_out(part, {k: v[:, 512:] for k, v in full.items()}, "shard", KEYS)
    _same(_arng(shard), gm.state_rows(0, 512, 512, 36), "the shard's generators")
    # action_rng_state / set_action_rng_state: a checkpoint replays through the C call
    obs = full["obs"][-1]
    st = env.action_rng_state()
    s1 = env.mlp_sample(agent, obs)
    _same(s1["raw_actions"], _expect(env, agent, obs, gm.normals(0, 0, N, 3, skip=36))[1], "the stream continues")
    env.set_action_rng_state(st)
    assert env._arng is not agent._bufs[env]
    raw = torch.empty_like(s1["raw_actions"])
    lp = torch.empty_like(s1["log_prob"])
    obj = agent._objs[env][1]
    assert env._lib.invsim_mlp_sample(env._h, obj, obs.data_ptr(), None, raw.data_ptr(), None, lp.data_ptr(),
                                      env._stream()) == 0
    _same(raw, s1["raw_actions"], "replay from the checkpoint"), _same(lp, s1["log_prob"], "replay: log_prob")
    s2 = env.mlp_sample(agent, obs)
    assert env._arng is agent._bufs[env]
    _same(s2["raw_actions"], _expect(env, agent, obs, gm.normals(0, 0, N, 3, skip=39))[1], "the agent's own stream")


# ---------------------------------------------------------------- 5. capture
def test_graph_of_closed_loop(gpu):
    """one episode cycle (periods + 1 = 8 steps) captured and replayed twice == eager calls"""
    import invsim
    (env, o_g), (twin, o_e) = _make(gpu, "im7"), _make(gpu, "im7")
    agent = _agent(env)
    agent.device_object(env), agent.device_object(twin)      # the first meeting synchronises: before the capture
    Cy = 8
    m_g, m_e = _metrics(env), _metrics(twin)
    o_g, o_e = o_g.clone(), o_e.clone()

    def loop(e, o, m):
        def fn():
            out = invsim.policies.collect_rollout(e, agent, Cy, o, metrics=m)
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
        _same_out(og, oe, f"replay {rep}", KEYS)
        _same(m_g, m_e, f"metrics after replay {rep}")
    assert torch.equal(env.get_state(), twin.get_state()) and env.position() == twin.position()
    _same(_arng(env), gm.state_rows(0, 0, N, 3 * Cy * 3), "a replay continues the stream")
    assert torch.equal(env._arng, twin._arng)


# ---------------------------------------------------------------- 6. refusals
def test_refusals_leave_state_and_generators_alone(gpu):
    import invsim
    from invsim import _capi
    (env, obs0), (other, _) = _make(gpu, "im7"), _make(gpu, "im7")
    same, o_same = _make(gpu, "im7", autoreset_mode="same_step")
    agent = _agent(env)
    obj, obj_other, obj_same = agent.device_object(env), agent.device_object(other), agent.device_object(same)
    plain = invsim.MLPPolicyAgent(list(zip(agent.weights, agent.biases)), activation="relu").device_object(env)
    lib, s = env._lib, env._stream()
    A = env.action_dim
    act = torch.zeros((2, N, A), dtype=torch.int64, device=gpu)
    raw = torch.zeros((2, N, A), dtype=torch.float32, device=gpu)
    lp = torch.zeros((2, N), dtype=torch.float32, device=gpu)
    buf = env._arng
    st, gen = env.get_state(), buf.clone()

    def sample(o, h=env, obs=obs0):
        return lib.invsim_mlp_sample(h._h, o, obs.data_ptr(), act.data_ptr(), raw.data_ptr(), None, lp.data_ptr(), s)

    def loop(o, h=env, obs=obs0):
        return lib.invsim_rollout_mlp_sample(h._h, 2, o, obs.data_ptr(), None, None, None, None, act.data_ptr(),
                                             raw.data_ptr(), lp.data_ptr(), None, s)

    def untouched(what):
        assert torch.equal(env.get_state(), st) and torch.equal(buf, gen), what
        assert bool((act == 0).all()) and bool((raw == 0).all()) and bool((lp == 0).all()), what

    # no Gaussian set on the object
    for call in (sample, loop):
        assert call(plain) == -22 and "Gaussian" in _capi.last_error(env._h)
    # another handle's object
    for call in (sample, loop):
        assert call(obj_other) == -22 and "another handle" in _capi.last_error(env._h)
    assert lib.invsim_mlp_set_gaussian(env._h, obj_other, agent.std.ctypes.data, agent.log_std.ctypes.data) == -22
    # every output NULL
    assert lib.invsim_mlp_sample(env._h, obj, obs0.data_ptr(), None, None, None, None, s) == -22
    # no generators attached
    env._attach_action_rng(None)
    for call in (sample, loop):
        assert call(obj) == -22 and "action generators" in _capi.last_error(env._h)
    env._attach_action_rng(buf)
    untouched("refused on the host")
    # SAME_STEP
    st_same, gen_same = same.get_state(), same._arng.clone()
    assert loop(obj_same, same, o_same) == -22 and "final_obs" in _capi.last_error(same._h)
    assert torch.equal(same.get_state(), st_same) and torch.equal(same._arng, gen_same)
    # invsim_mlp_set_gaussian: validation, and not during capture
    good_s, good_l = agent.std.copy(), agent.log_std.copy()
    for i, v in ((0, -1.0), (1, np.nan), (2, np.inf), (0, -np.inf)):
        bad = good_s.copy()
        bad[i] = v
        assert lib.invsim_mlp_set_gaussian(env._h, obj, bad.ctypes.data, good_l.ctypes.data) == -22, v
    for v in (np.nan, np.inf, -np.inf):
        bad = good_l.copy()
        bad[1] = v
        assert lib.invsim_mlp_set_gaussian(env._h, obj, good_s.ctypes.data, bad.ctypes.data) == -22, v
    assert lib.invsim_mlp_set_gaussian(env._h, obj, good_s.ctypes.data, None) == -22
    _capi.check(lib.invsim_capture_begin(env._h), env._h, "capture_begin")
    try:
        assert lib.invsim_mlp_set_gaussian(env._h, obj, good_s.ctypes.data, good_l.ctypes.data) == -22
        assert "capture" in _capi.last_error(env._h)
    finally:
        steps = C.c_int64(-1)
        assert lib.invsim_capture_end(env._h, C.byref(steps)) == 0 and steps.value == 0
    untouched("refused set_gaussian calls")
    # a refused set leaves the Gaussian that was set; NULL clears it; setting it again restores it
    assert sample(obj) == 0
    torch.cuda.synchronize(gpu)
    first = raw[0].clone()
    _same(first, _expect(env, agent, obs0, gm.normals(0, 0, N, A))[1], "the object still samples with its Gaussian")
    assert lib.invsim_mlp_set_gaussian(env._h, obj, None, None) == 0
    assert sample(obj) == -22 and "Gaussian" in _capi.last_error(env._h)
    assert lib.invsim_mlp_set_gaussian(env._h, obj, good_s.ctypes.data, good_l.ctypes.data) == 0
    buf.copy_(gen)
    assert sample(obj) == 0
    _same(raw[0], first, "set again")


# ---------------------------------------------------------------- 7. Python surface
def test_evaluate_agent_and_collect_rollout(gpu):
    import invsim
    cls, cfg = _cls_kw("im7")
    env = cls(N, device=gpu, autoreset_mode="disabled", **cfg)
    obs0, _ = env.reset(seed=0)
    agent = _agent(env)
    T = env._horizon()
    met = _metrics(env)
    out = invsim.policies.collect_rollout(env, agent, T, obs0, metrics=met)
    O, A = env.obs_dim, env.action_dim
    want = {"obs": ((T, N, O), env.obs_dtype), "actions": ((T, N, A), env.act_dtype),
            "raw_actions": ((T, N, A), torch.float32), "log_prob": ((T, N), torch.float32),
            "reward": ((T, N), torch.float64), "terminated": ((T, N), torch.bool), "truncated": ((T, N), torch.bool)}
    assert {k: (tuple(v.shape), v.dtype) for k, v in out.items()} == want
    # rollout_policy: the existing keys, the same numbers (a twin env, the agent's stream on it starts afresh)
    twin = cls(N, device=gpu, autoreset_mode="disabled", **cfg)
    o_t, _ = twin.reset(seed=0)
    met2 = _metrics(twin)
    rp = twin.rollout_policy(agent, T, obs=True, actions=True, metrics=met2, obs0=o_t)
    assert sorted(rp) == ["actions", "obs", "reward", "terminated", "truncated"]
    _same_out(rp, out, "rollout_policy", sorted(rp))
    _same(met2, met, "metrics")
    assert sorted(twin.rollout_policy(agent, 0, rewards=False, obs0=rp["obs"][-1])) == []
    # evaluate_agent: a fresh env inside, so the agent's stream starts afresh there too
    res = invsim.evaluate_agent(agent, cls, cfg, n_episodes=N, seed_offset=0, device=gpu)
    cols = invsim.policies.summarize(env.family, met.cpu().numpy())
    assert res["Agent"] == ["GaussianMLP"] * N
    for k, v in cols.items():
        assert np.array_equal(np.asarray(res[k]), np.asarray(v)), k
    assert (np.asarray(res["Steps"]) == T).all()
    with pytest.raises(ValueError, match="obs0"):
        invsim.policies.collect_rollout(env, agent, 2, None)
