"""INVSIM_POLICY_LEVELS on the GPU: per-env order-up-to levels (and reorder
points) read by the step kernels from attached device arrays.

Every launch path BaseStock has is pinned through the launch switches
(libinvsim reads them when a handle is made):

  default                                      3-role fused kernel (im_roll3o_kernel)
  INVSIM_IM_ROLL3O_MAX_N=0                     2-role fused kernel (im_roll3_kernel)
  INVSIM_IM_ROLL3O_MAX_N=0 INVSIM_IM_ROLL_SUB=128   the same as two sub-launches, a partial group
  INVSIM_IM_POL_ROLL=0                         the one-wave run kernel (im_run_kernel)

N = 200 is three full waves of 64 envs and a partial one of 8: the smallest
batch with a padded tail and more than one workgroup.  Checkers: the oracle's
BaseStockAgent with an array safety factor (oracle/agents.py) where the levels
are (L + 1) * mu * sf, tests/levels_model.py otherwise (closed loop: the action
recorded at step k is the model's on the observation of step k - 1), and a
replay of the recorded actions through rollout_metrics on a twin env for the
dynamics and the metrics.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import agents
import levels_model
from conftest import im_kwargs, knob_envs, load_golden

pytestmark = pytest.mark.gpu

N, K, T = 200, 30, 30
PATHS = {
    "roll3o": ({}, None, None),
    "roll3": ({}, "INVSIM_IM_ROLL3O_MAX_N", "0"),
    "roll3_sub": ({"INVSIM_IM_ROLL3O_MAX_N": "0"}, "INVSIM_IM_ROLL_SUB", "128"),
    "run": ({}, "INVSIM_IM_POL_ROLL", "0"),
}


def _envs(monkeypatch, path, gpu, cls_name, count=1, n=N, **kw):
    """`count` envs of one launch path (conftest.knob_envs sets the path's switch)."""
    import invsim
    pre, var, val = PATHS[path]
    for k, v in pre.items():
        monkeypatch.setenv(k, v)
    make = lambda: getattr(invsim, cls_name)(n, device=gpu, **kw)  # noqa: E731
    envs = knob_envs(monkeypatch, var or "INVSIM_IM_POL_ROLL", [val] * count, make)
    for k in pre:
        monkeypatch.delenv(k, raising=False)
    return envs


def _bits(t):
    t = t.contiguous()
    return t.view(torch.uint8) if t.dtype == torch.bool else t.view(torch.int64)


def _same(a, b, what):
    assert torch.equal(_bits(a), _bits(b)), what


def _metrics(env):
    import invsim
    return torch.zeros((env.num_envs, invsim.policies.metrics_dim(env)), dtype=torch.float64, device=env.device)


def _run(env, agent, k=K):
    met = _metrics(env)
    out = env.rollout_policy(agent, k, obs=True, actions=True, metrics=met)
    out["metrics"] = met
    return out


def _closed_loop(env, obs0, t0, out, levels, reorder=None):
    """Every recorded action is the model's on the observation before it, at the
    env's own period; a NEXT_STEP reset step keeps the zeros rollout_policy wrote.
    Returns the number of applied steps per env."""
    acts, obs = out["actions"].cpu().numpy(), out["obs"].cpu().numpy()
    prev = obs0.cpu().numpy()
    t = np.broadcast_to(np.asarray(t0, np.int64), (env.num_envs,)).copy()
    applied = np.zeros(env.num_envs, np.int64)
    lv = np.asarray(levels, np.float64)
    ro = None if reorder is None else np.asarray(reorder, np.float64)
    for k in range(acts.shape[0]):
        exp = levels_model.action(prev, np.minimum(t, env.num_periods - 1), env.lead_time, env.supply_capacity, lv, ro)
        reset = t >= env.num_periods
        exp[reset] = 0
        bad = np.flatnonzero((acts[k] != exp).any(axis=1))
        assert bad.size == 0, f"step {k}: envs {bad[:4].tolist()} ordered {acts[k][bad[:2]].tolist()}, " \
                              f"model {exp[bad[:2]].tolist()}"
        applied += ~reset
        t = np.where(reset, 0, t + 1)
        prev = obs[k]
    return applied


def _replay(twin, out):
    """The recorded actions through rollout_metrics on a twin env at the same
    state: the bits of obs, rewards, flags, metrics and the state blob."""
    met = _metrics(twin)
    rep = twin.rollout_metrics(out["actions"], metrics=met)
    for k in ("obs", "reward", "terminated", "truncated"):
        _same(rep[k], out[k], f"replay {k}")
    _same(met, out["metrics"], "replay metrics")


_ORACLE = {}


def _oracle_run(oracle, cls_name, sf_key, sf, seed, n=N):
    """agents.run_invmgmt on the default config, once per case (shared by the paths)."""
    key = (cls_name, sf_key, seed, n)
    if key not in _ORACLE:
        orc = oracle.OracleInvMgmt(n, backlog=cls_name.endswith("BacklogEnv"))
        orc.seed(range(seed, seed + n))
        o0 = orc.reset()
        res = agents.run_invmgmt(orc, o0, K, np.array([1, 5, 10], np.int64), 20, sf, np.array([100, 200, 230], np.int64))
        for a in res:
            a.setflags(write=False)
        _ORACLE[key] = res
    return _ORACLE[key]


def _against_oracle(out, exp):
    e_act, e_rew, e_obs, e_sum = exp
    assert np.array_equal(out["actions"].cpu().numpy(), e_act), "actions"
    assert np.array_equal(out["obs"].cpu().numpy(), e_obs), "obs"
    assert np.array_equal(out["reward"].cpu().numpy().view(np.uint64), e_rew.view(np.uint64)), "reward"
    assert np.array_equal(out["metrics"].cpu().numpy().view(np.uint64), e_sum.view(np.uint64)), "metrics"


CASES = [("InvManagementBacklogEnv", 1.37), ("InvManagementLostSalesEnv", 1.0)]


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("cls_name,sf", CASES)
def test_identity_with_base_stock_and_oracle(gpu, oracle, monkeypatch, path, cls_name, sf):
    import invsim
    env, twin = _envs(monkeypatch, path, gpu, cls_name, 2, autoreset_mode="disabled")
    env.reset(seed=500)
    twin.reset(seed=500)
    out = _run(env, invsim.LevelsAgent.from_safety_factor(env, sf))
    ref = _run(twin, invsim.BaseStockAgent(sf))
    for k in ("actions", "obs", "reward", "terminated", "truncated", "metrics"):
        _same(out[k], ref[k], f"{k} against BaseStockAgent")
    _same(env.get_state(), twin.get_state(), "state blob (RNG state included) against BaseStockAgent")
    _against_oracle(out, _oracle_run(oracle, cls_name, sf, sf, 500))


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("cls_name", [c for c, _ in CASES])
def test_per_env_levels_against_oracle(gpu, oracle, monkeypatch, path, cls_name):
    """no two envs share levels: a lane or row mix-up cannot pass"""
    import invsim
    sf = np.random.default_rng(20261).uniform(0.2, 2.5, size=(N, 3))
    (env,) = _envs(monkeypatch, path, gpu, cls_name, autoreset_mode="disabled")
    env.reset(seed=900)
    agent = invsim.LevelsAgent.from_safety_factor(env, sf)
    assert np.array_equal(np.asarray(agent.levels), (np.array([1, 5, 10]) + 1) * 20 * sf)
    out = _run(env, agent)
    _against_oracle(out, _oracle_run(oracle, cls_name, "per-env", sf, 900))


def _edge_levels(rng, n=N, a=3, hi=700.0):
    lv = rng.uniform(0.0, hi, size=(n, a))
    edge = [0.0, -3.5, 1e12, np.inf, np.nan, -np.inf]
    for r, v in enumerate(edge):                 # each edge value in every stage, on rows of several waves
        for i in range(a):
            lv[(7 + 31 * r + 67 * i) % n, i] = v
    lv[n - 1] = np.resize([np.nan, np.inf, 0.0], a)          # the last env (of the partial wave)
    return lv


@pytest.mark.parametrize("path", list(PATHS))
def test_edge_values_against_model(gpu, monkeypatch, path):
    import invsim
    env, twin = _envs(monkeypatch, path, gpu, "InvManagementBacklogEnv", 2, autoreset_mode="disabled")
    obs0, _ = env.reset(seed=41)
    twin.reset(seed=41)
    lv = _edge_levels(np.random.default_rng(3))
    out = _run(env, invsim.LevelsAgent(lv))
    _closed_loop(env, obs0, 0, out, lv)
    acts = out["actions"].cpu().numpy()
    assert (acts[:, N - 1, 0] == 0).all() and (acts[:, N - 1, 2] == 0).all()     # NaN and 0 never order
    assert acts[0, N - 1, 1] == 200                                               # +inf clips to c
    _replay(twin, out)
    _same(env.get_state(), twin.get_state(), "state blob after the replay")


@pytest.mark.parametrize("path", list(PATHS))
def test_reorder_points(gpu, monkeypatch, path):
    import invsim
    rng = np.random.default_rng(8)
    lv = rng.uniform(50.0, 700.0, size=(N, 3))
    ro = lv * rng.uniform(0.3, 1.0, size=(N, 3))
    ro[5, 0], ro[70, 1], ro[199, 2] = np.nan, np.inf, -np.inf
    envs = _envs(monkeypatch, path, gpu, "InvManagementLostSalesEnv", 5, autoreset_mode="disabled")
    obs0 = [e.reset(seed=77)[0] for e in envs]
    out = _run(envs[0], invsim.LevelsAgent(lv, ro))
    _closed_loop(envs[0], obs0[0], 0, out, lv, ro)
    assert bool((out["actions"] == 0).any()) and bool((out["actions"] > 0).any())
    _replay(envs[1], out)
    _same(envs[0].get_state(), envs[1].get_state(), "state blob after the replay")
    plain = _run(envs[2], invsim.LevelsAgent(lv))
    inf = _run(envs[3], invsim.LevelsAgent(lv, np.full((N, 3), np.inf)))
    for k in plain:
        _same(inf[k], plain[k], f"{k}: reorder = +inf against no reorder")
    _same(envs[3].get_state(), envs[2].get_state(), "state blob: reorder = +inf against no reorder")
    never = _run(envs[4], invsim.LevelsAgent(lv, np.full(3, -np.inf)))
    assert not bool(never["actions"].any())


@pytest.mark.parametrize("path", ["roll3o", "roll3"])
@pytest.mark.parametrize("n,stream", [(136, "numpy"), (136, "philox"), (200, "philox")])
def test_one_group_form_and_fast_stream_fused(gpu, oracle, monkeypatch, path, n, stream):
    """The fused instantiations the other tests do not launch.  N = 136 is three
    64-env groups (the last of 8 envs): an odd count, so the 3-role kernel runs
    its one-group-per-workgroup form (im_roll3o_kernel<.., 1>; an even count
    takes the two-group form).  demand_stream="philox" on the default lead
    times runs the PhiloxGen instantiations of im_roll3o_kernel (both forms)
    and im_roll3_kernel."""
    import invsim
    cls_name = "InvManagementBacklogEnv" if path == "roll3o" else "InvManagementLostSalesEnv"
    envs = _envs(monkeypatch, path, gpu, cls_name, 4, n=n, autoreset_mode="disabled", demand_stream=stream)
    obs0 = [e.reset(seed=640)[0] for e in envs]
    # the identity with BaseStock, state blob included
    out = _run(envs[0], invsim.LevelsAgent.from_safety_factor(envs[0], 1.37))
    ref = _run(envs[1], invsim.BaseStockAgent(1.37))
    for k in ("actions", "obs", "reward", "terminated", "truncated", "metrics"):
        _same(out[k], ref[k], f"{k} against BaseStockAgent")
    _same(envs[0].get_state(), envs[1].get_state(), "state blob against BaseStockAgent")
    if stream == "numpy":
        _against_oracle(out, _oracle_run(oracle, cls_name, 1.37, 1.37, 640, n))
    # per-env levels and reorder points, edge values included, against the model
    lv = _edge_levels(np.random.default_rng(n), n=n)
    ro = lv * np.random.default_rng(n + 1).uniform(0.5, 1.2, size=(n, 3))
    out = _run(envs[2], invsim.LevelsAgent(lv, ro))
    _closed_loop(envs[2], obs0[2], 0, out, lv, ro)
    assert bool((out["actions"] > 0).any())
    _replay(envs[3], out)
    _same(envs[2].get_state(), envs[3].get_state(), "state blob after the replay")


def test_in_place_condition_and_graph_keep_alive(gpu):
    """Which tensors a LevelsAgent reads in place, and that a captured graph
    keeps the tensors it recorded alive after another agent attaches."""
    import gc
    import weakref
    import invsim
    env = invsim.InvManagementLostSalesEnv(N, device=gpu)
    env.reset(seed=3)
    base = torch.full((N, 3), 90.0, dtype=torch.float64, device=gpu)
    assert invsim.LevelsAgent(base).tensors(env)[0] is base
    assert invsim.LevelsAgent(base.to(torch.device("cuda", gpu.index or 0))).tensors(env)[0].data_ptr() == base.data_ptr()
    for other in (base.float(), base.t().contiguous().t(), base[0], base.cpu()):   # dtype, stride, shape [A], host
        t = invsim.LevelsAgent(other).tensors(env)[0]
        assert t.data_ptr() != other.data_ptr() and t.dtype == torch.float64 and t.is_contiguous()
        assert tuple(t.shape) == (N, 3) and t.device == env.device and bool((t == 90.0).all())
    lv = torch.full((N, 3), 250.0, dtype=torch.float64, device=gpu)
    agent = invsim.LevelsAgent(lv)
    cyc = env._horizon() + 1
    g = env.capture(lambda: env.rollout_policy(agent, cyc, actions=True))
    first = g.replay()["actions"].clone()
    ref = weakref.ref(lv)
    del lv, agent
    env.rollout_policy(invsim.LevelsAgent(base), cyc)          # another agent attaches its own tensor
    gc.collect()
    assert ref() is not None, "the graph must keep the tensor it recorded"
    env.reset(seed=3)
    env.rollout_policy(invsim.LevelsAgent(base), cyc)          # the warm-up cycle the capture ran
    again = g.replay()["actions"]
    _same(again, first, "a replay after another agent attached reads the recorded tensor")


def _geometry(name):
    if name == "2stage":
        return "InvManagementBacklogEnv", dict(I0=[100], r=[15, 10], k=[0.1, 0.075], h=[0.15], c=[100], L=[2]), {}
    if name == "9stage":
        _, cfg = load_golden("invmgmt_lostsales_9stage")
        return cfg["cls"], im_kwargs(cfg), {}
    if name == "L0":
        return "InvManagementLostSalesEnv", dict(I0=[100, 150], r=[15, 10, 7], k=[0.1, 0.075, 0.05], h=[0.15, 0.1],
                                                 c=[100, 200], L=[0, 3]), {}
    if name == "dist3":
        return "InvManagementBacklogEnv", dict(dist=3, dist_param={"low": 3, "high": 41}), {}
    return "InvManagementBacklogEnv", {}, dict(demand_stream="philox")


@pytest.mark.parametrize("name", ["2stage", "9stage", "L0", "dist3", "philox"])
def test_other_geometries(gpu, monkeypatch, name):
    import invsim
    cls_name, cfg, vkw = _geometry(name)
    env, twin = _envs(monkeypatch, "run", gpu, cls_name, 2, autoreset_mode="disabled", **cfg, **vkw)
    obs0, _ = env.reset(seed=13)
    twin.reset(seed=13)
    A = env.action_dim
    base = (env.lead_time + 1) * env.dist_param.get("mu", 10)
    lv = _edge_levels(np.random.default_rng(17), a=A, hi=1.0) * 2.5 * base
    ro = lv * np.random.default_rng(18).uniform(0.5, 1.2, size=(N, A))
    out = _run(env, invsim.LevelsAgent(lv, ro), k=env.num_periods)
    _closed_loop(env, obs0, 0, out, lv, ro)
    assert bool((out["actions"] > 0).any())
    _replay(twin, out)
    _same(env.get_state(), twin.get_state(), "state blob after the replay")


@pytest.mark.parametrize("path", ["roll3o", "roll3_sub", "run"])
def test_next_step_autoreset(gpu, monkeypatch, path):
    """K = 62 from a reset: periods 0..29, the reset step (row 30), periods 0..29
    again and the second reset step (row 61).  (Two horizons and both reset
    steps are 62 rows: 61 would end before the second reset step.)"""
    import invsim
    env, twin = _envs(monkeypatch, path, gpu, "InvManagementBacklogEnv", 2)
    obs0, _ = env.reset(seed=21)
    twin.reset(seed=21)
    lv = np.random.default_rng(4).uniform(0.0, 700.0, size=(N, 3))
    out = _run(env, invsim.LevelsAgent(lv), k=2 * T + 2)
    applied = _closed_loop(env, obs0, 0, out, lv)
    assert (applied == 2 * T).all()
    for row in (T, 2 * T + 1):
        assert not bool(out["actions"][row].any()), f"reset row {row} was written"
        assert not bool(out["reward"][row].any()) and not bool(out["truncated"][row].any())
    assert bool(out["actions"][T + 1].any())
    assert bool((out["metrics"][:, 1] == 2 * T).all()), "a reset step added to the step count"
    _replay(twin, out)
    _same(env.get_state(), twin.get_state(), "state blob after the replay")


def test_per_env_periods(gpu, monkeypatch):
    """a masked reset of every third env after 7 steps: K = 30 then runs with
    per-env periods (im_run_kernel), each env's rule at its own period"""
    import invsim
    env, twin = _envs(monkeypatch, "roll3o", gpu, "InvManagementBacklogEnv", 2)
    lv = np.random.default_rng(6).uniform(0.0, 700.0, size=(N, 3))
    agent = invsim.LevelsAgent(lv)
    mask = torch.arange(N, device=gpu) % 3 == 0
    o_first = {}
    for e in (env, twin):
        e.reset(seed=33)
        o_first[e] = e.rollout_policy(agent, 7, obs=True)["obs"][-1].clone()
        o_reset, _ = e.reset(options={"reset_mask": mask})
        o_first[e][mask] = o_reset[mask]
    _same(o_first[env], o_first[twin], "the twins before the launch")
    t0 = np.where(mask.cpu().numpy(), 0, 7)
    out = _run(env, agent)
    applied = _closed_loop(env, o_first[env], t0, out, lv)
    assert (applied == np.where(t0 == 0, K, K - 1)).all()
    assert not bool(out["actions"][T - 7][~mask].any()), "reset rows of the envs at period 30"
    _replay(twin, out)
    _same(env.get_state(), twin.get_state(), "state blob after the replay")


def test_device_residency(gpu, monkeypatch):
    import invsim
    (env,) = _envs(monkeypatch, "roll3o", gpu, "InvManagementBacklogEnv", autoreset_mode="disabled")
    obs0, _ = env.reset(seed=55)
    rng = np.random.default_rng(9)
    lv1, lv2 = rng.uniform(0.0, 300.0, size=(N, 3)), rng.uniform(300.0, 700.0, size=(N, 3))
    dev = torch.from_numpy(lv1).to(gpu)
    agent = invsim.LevelsAgent(dev)
    a = _run(env, agent, k=15)
    assert env._levels[0] is dev, "a device tensor is used in place"
    dev.copy_(torch.from_numpy(lv2))
    b = _run(env, agent, k=15)
    _closed_loop(env, obs0, 0, a, lv1)
    _closed_loop(env, a["obs"][-1], 15, b, lv2)
    assert not np.array_equal(levels_model.action(a["obs"][-1].cpu().numpy(), 15, env.lead_time, env.supply_capacity, lv1),
                              b["actions"][0].cpu().numpy()), "the second launch must differ from the old levels' orders"


def test_captured_graph_reads_current_levels(gpu):
    import invsim
    n = 4096
    env = invsim.InvManagementLostSalesEnv(n, device=gpu)
    twin = invsim.InvManagementLostSalesEnv(n, device=gpu)
    rng = np.random.default_rng(10)
    lv1, lv2 = rng.uniform(0.0, 700.0, size=(n, 3)), rng.uniform(0.0, 700.0, size=(n, 3))
    devs = [torch.from_numpy(lv1).to(gpu) for _ in range(2)]
    ag, ag_t = invsim.LevelsAgent(devs[0]), invsim.LevelsAgent(devs[1])
    env.reset(seed=2)
    twin.reset(seed=2)
    cyc = env._horizon() + 1
    g = env.capture(lambda: env.rollout_policy(ag, cyc, obs=True, actions=True))    # (warm-up: one eager cycle)
    twin.rollout_policy(ag_t, cyc, obs=True, actions=True)
    for lv in (lv1, lv2, lv1):
        for d in devs:
            d.copy_(torch.from_numpy(lv))
        og = g.replay()
        oe = twin.rollout_policy(ag_t, cyc, obs=True, actions=True)
        torch.cuda.synchronize(gpu)
        for k in oe:
            _same(og[k], oe[k], f"{k}: replay against an eager run with the same values")
    assert not torch.equal(og["actions"], torch.zeros_like(og["actions"]))


def test_refusals(gpu):
    import invsim
    from invsim import _capi
    lib = _capi.lib()
    spec = _capi.PolicySpec(_capi.POLICY_KINDS["levels"], 0, 0.0, 0.0, None)

    def launch(env, k=3):
        met = _metrics(env)
        return lib.invsim_rollout_policy(env._h, k, C.byref(spec), None, None, None, None, None, met.data_ptr(),
                                         env._stream())

    env = invsim.InvManagementBacklogEnv(N, device=gpu, autoreset_mode="disabled")
    obs0, _ = env.reset(seed=1)
    assert launch(env) == -22 and "no levels attached" in _capi.last_error(env._h)
    lv = torch.full((N, 3), 100.0, dtype=torch.float64, device=gpu)
    for other in (invsim.NewsvendorEnv(N, device=gpu), invsim.NetInvMgmtBacklogEnv(N, device=gpu)):
        other.reset(seed=1)
        assert launch(other) == -22 and "InvMgmt" in _capi.last_error(other._h)
        assert lib.invsim_set_policy_levels(other._h, lv.data_ptr(), None) == -22
        assert "InvMgmt" in _capi.last_error(other._h)
        with pytest.raises(TypeError, match="InvManagement"):
            other.rollout_policy(invsim.LevelsAgent([1.0]), 3)
        other.step(torch.zeros((N, other.action_dim), device=gpu))          # still usable
    same = invsim.InvManagementBacklogEnv(N, device=gpu, autoreset_mode="same_step")
    same.reset(seed=1)
    with pytest.raises(_capi.InvsimError, match="SAME_STEP|final_obs"):
        same.rollout_policy(invsim.LevelsAgent(lv), 3)
    same.step(torch.zeros((N, 3), dtype=torch.int64, device=gpu))
    assert lib.invsim_capture_begin(env._h) == 0
    try:
        assert lib.invsim_set_policy_levels(env._h, lv.data_ptr(), None) == -22
        assert "cannot be captured" in _capi.last_error(env._h)
    finally:
        assert lib.invsim_capture_end(env._h, None) == 0
    assert launch(env) == -22, "the refused attach must not have attached"
    with pytest.raises(ValueError, match="shape"):
        env.rollout_policy(invsim.LevelsAgent(np.zeros((N, 2))), 3)
    out = _run(env, invsim.LevelsAgent(lv))                                 # the env is still at its reset
    _closed_loop(env, obs0, 0, out, np.full((N, 3), 100.0))
    assert lib.invsim_set_policy_levels(env._h, None, None) == 0           # detach
    assert launch(env) == -22


def test_evaluate_levels(gpu):
    import invsim
    from invsim.policies import evaluate_levels
    Cn, R, off = 4, 50, 1000
    lv = np.array([[40.0, 120.0, 220.0], [55.5, 180.0, 300.0], [40.0, 120.0, 220.0], [90.0, 400.0, 650.0]])
    res = evaluate_levels(lv, invsim.InvManagementBacklogEnv, n_episodes=R, seed_offset=off, device=gpu)
    for k in ("TotalReward", "Steps", "AvgServiceLevel", "TotalStockoutQty", "AvgEndingInv"):
        assert res[k].shape == (Cn, R), k
    cand = res["candidates"]
    for k in ("AvgReward", "StdReward", "AvgServiceLevel", "AvgEndingInv"):
        assert cand[k].shape == (Cn,), k
    tot = res["TotalReward"]
    assert np.array_equal(tot[0].view(np.uint64), tot[2].view(np.uint64)), "identical candidates, common seeds"
    assert not np.array_equal(tot[0], tot[1])
    assert (res["Steps"] == 30).all()
    for c in range(Cn):
        one = invsim.evaluate_agent(invsim.LevelsAgent(lv[c]), invsim.InvManagementBacklogEnv, n_episodes=R,
                                    seed_offset=off, device=gpu)
        assert np.array_equal(one["TotalReward"].view(np.uint64), tot[c].view(np.uint64)), f"candidate {c}"
        assert np.array_equal(one["AvgServiceLevel"], res["AvgServiceLevel"][c])
        assert cand["AvgReward"][c] == np.mean(one["TotalReward"])
        assert cand["StdReward"][c] == np.std(one["TotalReward"], ddof=1)
        assert cand["AvgServiceLevel"][c] == np.mean(one["AvgServiceLevel"])
        assert cand["AvgEndingInv"][c] == np.mean(one["AvgEndingInv"])


def test_tune_levels(gpu):
    import invsim
    from invsim.policies import tune_levels
    kw = dict(n_episodes=32, population=64, iterations=5, seed=3, seed_offset=200, device=gpu)
    res = tune_levels(invsim.InvManagementBacklogEnv, **kw)
    hist = res["history"]
    assert hist.shape == (5,) and res["levels"].shape == (3,) and res["TotalReward"].shape == (32,)
    assert (np.diff(hist) >= 0).all(), hist
    base = invsim.evaluate_agent(invsim.BaseStockAgent(1.0), invsim.InvManagementBacklogEnv, n_episodes=32,
                                 seed_offset=200, device=gpu)
    assert hist[-1] >= np.mean(base["TotalReward"]), (hist, np.mean(base["TotalReward"]))
    assert hist[-1] == np.mean(res["TotalReward"])
    again = tune_levels(invsim.InvManagementBacklogEnv, **kw)
    assert np.array_equal(again["levels"], res["levels"]) and np.array_equal(again["history"], hist)
    one = invsim.evaluate_agent(invsim.LevelsAgent(res["levels"]), invsim.InvManagementBacklogEnv, n_episodes=32,
                                seed_offset=200, device=gpu)
    assert np.array_equal(one["TotalReward"].view(np.uint64), res["TotalReward"].view(np.uint64))
