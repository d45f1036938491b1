"""INVSIM_POLICY_NET_LEVELS on the GPU: per-env order-up-to levels (and reorder
points) of every reorder link, read by the NetInvMgmt kernels from attached
device arrays (include/invsim.h, "Per-env order-up-to levels on a supply
network").

Every launch path CONSTANT has on NetInvMgmt is pinned through the launch
switches (libinvsim reads them when a handle is made):

  default                  the fused 3-role rollout (net_roll3o_kernel), default and custom graph
  INVSIM_NET_POL_ROLL=0    the one-wave specialised kernel (net_spec_kernel)
  INVSIM_NET_GENERIC=1     the table-walking kernel (net_run_kernel), which every other graph runs anyway

N = 200 is three full waves of 64 envs and a partial one of 8: more than one
workgroup in every kernel and a padded tail.  The checker is
tests/net_levels_model.py on the C oracle (the closed loop from the oracle's own
f64 X, U, Y), plus a replay of the recorded actions through rollout_metrics on a
twin env for the dynamics, the metrics and the state blob.  All comparisons are
by bit pattern.  Levels ~ U(0, 120): tests/test_net_levels.py shows without a
GPU that these inputs order strictly inside (0, high) and order 0 often enough,
and every test here asserts the same two shares on the recorded actions.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import net_graphs
import net_levels_model as model
from conftest import knob_envs

pytestmark = pytest.mark.gpu

N, SEED = 200, 3
PATHS = {"fused": ("INVSIM_NET_POL_ROLL", None), "spec": ("INVSIM_NET_POL_ROLL", "0"),
         "generic": ("INVSIM_NET_GENERIC", "1")}
# name -> (num_periods, alpha, reorder links)
GRAPHS = {"default": (30, 1.0, 11), "custom": (30, 1.0, 5), "mixed": (12, 0.93, 10), "chain": (10, 0.97, 4)}


def _graph(name, oracle=None):
    """the graph for the env (oracle None) or for the oracle, which names the samplers by method"""
    if name == "default":
        return None
    if name == "custom":
        if oracle is not None:
            return oracle.custom_graph()
        from invsim.topology import custom_graph
        return custom_graph()
    return net_graphs.GRAPHS[name](net_graphs.by_name, GRAPHS[name][0])


def _envs(monkeypatch, gpu, graph, path, cls_name="NetInvMgmtMasterEnv", count=1, n=N, **kw):
    import invsim
    T, alpha, _ = GRAPHS[graph]
    var, val = PATHS[path]
    make = lambda: getattr(invsim, cls_name)(n, device=gpu, graph=_graph(graph), num_periods=T, alpha=alpha, **kw)  # noqa: E731
    envs = knob_envs(monkeypatch, var, [val] * count, make)
    want = 0 if path == "generic" or graph in ("mixed", "chain") else {"default": 1, "custom": 2}[graph]
    assert all(e.kernel_variant == want for e in envs), (graph, path)
    return envs


def _loop(oracle, graph, backlog, levels, reorder=None, idx=None, n=N, stream="numpy"):
    """a ClosedLoop over the envs `idx` (default all n) of the batch seeded SEED .. SEED + n - 1"""
    T, alpha, _ = GRAPHS[graph]
    idx = np.arange(n) if idx is None else np.asarray(idx)
    g = _graph(graph, oracle)
    orc = oracle.OracleNet(len(idx), graph=g, num_periods=T, backlog=backlog, alpha=alpha, demand_stream=stream)
    orc.seed([SEED + int(e) for e in idx])
    high = model.action_high(oracle.default_graph() if g is None else g)
    lv = np.broadcast_to(np.asarray(levels, np.float64), (n, orc.act_dim))[idx]
    ro = None if reorder is None else np.broadcast_to(np.asarray(reorder, np.float64), (n, orc.act_dim))[idx]
    return model.ClosedLoop(orc, lv, ro, high)


_MODEL = {}


def _expected(oracle, key, graph, backlog, levels, reorder=None, K=None, autoreset=False, n=N, stream="numpy"):
    """the model's K rows from a reset, computed once per case and shared (read-only) by the paths"""
    key = (key, graph, backlog, K, autoreset, n, stream)
    if key not in _MODEL:
        loop = _loop(oracle, graph, backlog, levels, reorder, n=n, stream=stream)
        out = loop.run(GRAPHS[graph][0] if K is None else K, autoreset)
        out["obs0"], out["high"], out["xs"] = loop.obs0, loop.high, np.stack(loop.xs)
        for a in out.values():
            a.setflags(write=False)
        _MODEL[key] = out
    return _MODEL[key]


def _bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a)
    if a.dtype == np.bool_:
        return a.view(np.uint8)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(got, exp, what):
    g, e = _bits(got), _bits(exp)
    assert g.shape == e.shape, f"{what}: {g.shape} vs {e.shape}"
    if not np.array_equal(g, e):
        bad = np.argwhere(g != e)[:4].tolist()
        pytest.fail(f"{what}: {int((g != e).sum())} entries differ, first at {bad}")


def _metrics(env):
    import invsim
    return torch.zeros((env.num_envs, invsim.policies.metrics_dim(env)), dtype=torch.float64, device=env.device)


def _run(env, agent, K, met=None):
    met = _metrics(env) if met is None else met
    out = env.rollout_policy(agent, K, obs=True, actions=True, metrics=met)
    out["metrics"] = met
    return out


def _against(out, exp, what=""):
    for k in ("actions", "obs", "reward", "truncated", "metrics"):
        _same(out[k], exp[k], f"{what}{k} against the oracle model")
    assert not bool(out["terminated"].any()), f"{what}terminated"


def _shares(out, high):
    """at least 10 % of the recorded orders strictly inside (0, high), at least 10 % equal to 0"""
    inside, zero = model.shares(out["actions"].cpu().numpy(), high)
    assert inside >= 0.10 and zero >= 0.10, (inside, zero)


def _replay(twin, out):
    """The recorded actions through rollout_metrics on a twin env at the same
    state: the bits of obs, rewards, flags, metrics and then the state blob."""
    met = _metrics(twin)
    rep = twin.rollout_metrics(out["actions"], metrics=met)
    for k in ("obs", "reward", "terminated", "truncated"):
        _same(rep[k], out[k], f"replay {k}")
    _same(met, out["metrics"], "replay metrics")


def _levels(graph, n=N, seed=0):
    return np.random.default_rng(seed).uniform(0.0, 120.0, size=(n, GRAPHS[graph][2]))


LAUNCH_CASES = [("default", p, c) for c in ("NetInvMgmtBacklogEnv", "NetInvMgmtLostSalesEnv") for p in PATHS] + \
               [("custom", "fused", "NetInvMgmtMasterEnv"), ("custom", "spec", "NetInvMgmtMasterEnv")]


@pytest.mark.parametrize("graph,path,cls_name", LAUNCH_CASES)
def test_against_model_per_launch_path(gpu, oracle, monkeypatch, graph, path, cls_name):
    import invsim
    kw = dict(backlog=False) if cls_name.endswith("LostSalesEnv") else {}   # (the class alone keeps backlog=True)
    env, twin = _envs(monkeypatch, gpu, graph, path, cls_name, 2, autoreset_mode="disabled", **kw)
    assert env.backlog == (not kw)
    lv = _levels(graph)
    exp = _expected(oracle, "plain", graph, env.backlog, lv)
    assert np.array_equal(env._action_high(), exp["high"])
    obs0, _ = env.reset(seed=SEED)
    twin.reset(seed=SEED)
    _same(obs0, exp["obs0"], "reset obs")
    out = _run(env, invsim.NetLevelsAgent(lv), GRAPHS[graph][0])
    _against(out, exp)
    _shares(out, exp["high"])
    _replay(twin, out)
    _same(env.get_state(), twin.get_state(), "state blob after the replay")


@pytest.mark.parametrize("graph", ["mixed", "chain"])
def test_arbitrary_graphs(gpu, oracle, monkeypatch, graph):
    """mixed: yields 0.8 and 0.55 make the positions fractional, three markets of
    three kinds; chain: an L = 0 link, a market without a demand source"""
    import invsim
    env, twin = _envs(monkeypatch, gpu, graph, "fused", count=2, autoreset_mode="disabled")
    lv = _levels(graph)
    exp = _expected(oracle, "plain", graph, True, lv)
    if graph == "mixed":
        assert (exp["xs"] != np.rint(exp["xs"])).any(), "no fractional X: the summation order is not exercised"
    assert np.array_equal(env._action_high(), exp["high"])
    env.reset(seed=SEED)
    twin.reset(seed=SEED)
    out = _run(env, invsim.NetLevelsAgent(lv), GRAPHS[graph][0])
    _against(out, exp)
    _shares(out, exp["high"])
    _replay(twin, out)
    _same(env.get_state(), twin.get_state(), "state blob after the replay")


def _edge_levels(graph):
    """U(0, 120) with every edge value on every link, on rows of several waves, and the last env"""
    lv = _levels(graph, seed=5)
    n, a = lv.shape
    edge = [0.0, -3.5, 1e12, np.inf, np.nan, -np.inf, 57.25, 5000.0]   # (5000 > high = 1700)
    for r, v in enumerate(edge):
        for i in range(a):
            lv[(7 + 23 * r + 67 * i) % n, i] = v
    lv[n - 1] = np.resize([np.nan, np.inf, 0.0, 33.5], a)
    ro = 0.9 * _levels(graph, seed=6) + 20.0
    for r, v in enumerate([np.nan, np.inf, -np.inf]):
        for i in range(a):
            ro[(11 + 41 * r + 29 * i) % n, i] = v
    return lv, ro


@pytest.mark.parametrize("path", list(PATHS))
def test_edge_values(gpu, oracle, monkeypatch, path):
    import invsim
    env, twin = _envs(monkeypatch, gpu, "default", path, count=2, autoreset_mode="disabled")
    lv, ro = _edge_levels("default")
    exp = _expected(oracle, "edge", "default", True, lv, ro)
    env.reset(seed=SEED)
    twin.reset(seed=SEED)
    out = _run(env, invsim.NetLevelsAgent(lv, ro), 30)
    _against(out, exp)
    _shares(out, exp["high"])
    acts = out["actions"].cpu().numpy()
    assert (acts[:, N - 1, 0] == 0).all() and (acts[:, N - 1, 2] == 0).all()     # NaN and 0 never order
    assert (exp["actions"] == 1700.0).any(), "a +inf / 1e12 / 5000 level must order the cap somewhere"
    _replay(twin, out)
    _same(env.get_state(), twin.get_state(), "state blob after the replay")


@pytest.mark.parametrize("path", ["fused", "generic"])
def test_reorder_points(gpu, oracle, monkeypatch, path):
    import invsim
    envs = _envs(monkeypatch, gpu, "default", path, count=4, autoreset_mode="disabled")
    lv = _levels("default")
    ro = 0.8 * lv
    exp = _expected(oracle, "reorder", "default", True, lv, ro)
    for e in envs:
        e.reset(seed=SEED)
    out = _run(envs[0], invsim.NetLevelsAgent(lv, ro), 30)
    _against(out, exp)
    _shares(out, exp["high"])
    plain = _run(envs[1], invsim.NetLevelsAgent(lv), 30)
    assert not torch.equal(plain["actions"], out["actions"]), "the reorder points must change the orders"
    inf = _run(envs[2], invsim.NetLevelsAgent(lv, np.full((N, 11), np.inf)), 30)
    for k in plain:
        _same(inf[k], plain[k], f"{k}: reorder = +inf against no reorder")
    never = _run(envs[3], invsim.NetLevelsAgent(lv, np.full(11, -np.inf)), 30)
    assert not bool(never["actions"].any())


def test_next_step_autoreset(gpu, oracle, monkeypatch):
    """K = 2 T + 3 from a reset: periods 0..29, the reset step (row 30), periods
    0..29 again, the second reset step (row 61) and period 0 (row 62)."""
    import invsim
    T, K = 30, 63
    lv = _levels("default")
    exp = _expected(oracle, "plain", "default", True, lv, K=K, autoreset=True)
    assert exp["applied"].sum() == 2 * T + 1 and not exp["applied"][T] and not exp["applied"][2 * T + 1]
    outs = {}
    for path in PATHS:
        env, twin = _envs(monkeypatch, gpu, "default", path, count=2)
        env.reset(seed=SEED)
        twin.reset(seed=SEED)
        out = outs[path] = _run(env, invsim.NetLevelsAgent(lv), K)
        _against(out, exp, f"[{path}] ")
        for row in (T, 2 * T + 1):
            assert not bool(out["actions"][row].any()), f"[{path}] reset row {row} was written"
            assert not bool(out["reward"][row].any()) and not bool(out["truncated"][row].any())
        assert bool(out["actions"][T + 1].any())
        assert bool((out["metrics"][:, 1] == 2 * T + 1).all()), "a reset step added to the step count"
        _shares(out, exp["high"])
        _replay(twin, out)
        _same(env.get_state(), twin.get_state(), f"[{path}] state blob after the replay")
    for path in ("spec", "generic"):
        for k in outs["fused"]:
            _same(outs[path][k], outs["fused"][k], f"{k}: {path} against fused")


@pytest.mark.parametrize("path", ["spec", "generic"])
def test_per_env_periods(gpu, oracle, monkeypatch, path):
    """7 steps, a masked reset of every third env, then K = 30 with per-env
    periods (t_u = -1: the TU = false instantiations): the envs at period 7
    meet their reset row at row 23, the others run a whole episode."""
    import invsim
    env, twin = _envs(monkeypatch, gpu, "default", path, count=2)
    lv = _levels("default")
    agent = invsim.NetLevelsAgent(lv)
    mask = np.arange(N) % 3 == 0
    loops = {True: _loop(oracle, "default", True, lv, idx=np.flatnonzero(mask)),
             False: _loop(oracle, "default", True, lv, idx=np.flatnonzero(~mask))}
    first = {m: lp.run(7) for m, lp in loops.items()}
    loops[True].metrics[:] = 0.0
    loops[True].reset()
    loops[False].metrics[:] = 0.0
    rows = {m: lp.run(30, autoreset=True) for m, lp in loops.items()}
    assert rows[True]["applied"].all() and not rows[False]["applied"][23] and rows[False]["applied"].sum() == 29
    exp = {}
    for k in ("actions", "obs", "reward", "truncated"):
        a = np.zeros((30, N) + rows[True][k].shape[2:], rows[True][k].dtype)
        a[:, mask], a[:, ~mask] = rows[True][k], rows[False][k]
        exp[k] = a
    exp["metrics"] = np.zeros((N, 11))
    exp["metrics"][mask], exp["metrics"][~mask] = rows[True]["metrics"], rows[False]["metrics"]
    dmask = torch.from_numpy(mask).to(gpu)
    for e in (env, twin):
        e.reset(seed=SEED)
        pre = e.rollout_policy(agent, 7, obs=True, actions=True)
        e.reset(options={"reset_mask": dmask})
        assert e.position() & 0xFFFFFFFF == 0xFFFFFFFF, "per-env periods after a masked reset"
    _same(pre["actions"][:, ~dmask], first[False]["actions"], "the seven lock-step rows")
    out = _run(env, agent, 30)
    _against(out, exp)
    assert not bool(out["actions"][23][~dmask].any()), "reset rows of the envs that were at period 7"
    _shares(out, model.action_high(oracle.default_graph()))
    _replay(twin, out)
    _same(env.get_state(), twin.get_state(), "state blob after the replay")


def test_philox_demand_stream_fused(gpu, oracle, monkeypatch):
    import invsim
    env, twin = _envs(monkeypatch, gpu, "default", "fused", "NetInvMgmtBacklogEnv", 2, autoreset_mode="disabled",
                      demand_stream="philox")
    lv = _levels("default")
    exp = _expected(oracle, "plain", "default", True, lv, stream="philox")
    numpy_rows = _expected(oracle, "plain", "default", True, lv)
    assert not np.array_equal(exp["obs"], numpy_rows["obs"]), "the two streams draw different demands"
    env.reset(seed=SEED)
    twin.reset(seed=SEED)
    out = _run(env, invsim.NetLevelsAgent(lv), 30)
    _against(out, exp)
    _shares(out, exp["high"])
    _replay(twin, out)
    _same(env.get_state(), twin.get_state(), "state blob after the replay")


@pytest.mark.parametrize("path", list(PATHS))
def test_partial_wave_batch(gpu, oracle, monkeypatch, path):
    """N = 40: one workgroup whose only wave is partial"""
    import invsim
    n = 40
    (env,) = _envs(monkeypatch, gpu, "default", path, n=n, autoreset_mode="disabled")
    lv = _levels("default", n=n, seed=2)
    exp = _expected(oracle, "plain40", "default", True, lv, n=n)
    env.reset(seed=SEED)
    out = _run(env, invsim.NetLevelsAgent(lv), 30)
    _against(out, exp)
    _shares(out, exp["high"])


def test_device_residency(gpu, oracle, monkeypatch):
    """a device tensor is read in place: lv.copy_() between launches changes the next launch"""
    import invsim
    (env,) = _envs(monkeypatch, gpu, "default", "fused", autoreset_mode="disabled")
    lv1, lv2 = _levels("default", seed=8), _levels("default", seed=9) + 40.0
    loop = _loop(oracle, "default", True, lv1)
    a_exp = loop.run(15)                     # ("metrics": the sums after these 15 steps)
    loop.levels = lv2
    b_exp = loop.run(15)                     # (the sums after all 30)
    unchanged = _expected(oracle, "lv1", "default", True, lv1)
    assert np.array_equal(unchanged["actions"][:15], a_exp["actions"])
    assert not np.array_equal(unchanged["actions"][15], b_exp["actions"][0]), "the new levels must order differently"
    dev = torch.from_numpy(lv1).to(gpu)
    agent = invsim.NetLevelsAgent(dev)
    env.reset(seed=SEED)
    met = _metrics(env)
    a = _run(env, agent, 15, met)
    assert env._levels[0] is dev and agent.tensors(env)[0] is dev, "a device tensor is used in place"
    _against(dict(a, metrics=met.clone()), a_exp, "first launch: ")
    dev.copy_(torch.from_numpy(lv2))
    b = _run(env, agent, 15, met)
    _against(b, b_exp, "second launch: ")
    _shares(b, loop.high)
    for other in (dev.float(), dev[0], dev.cpu()):                         # dtype, shape [A], host: copied once
        t = invsim.NetLevelsAgent(other).tensors(env)[0]
        assert t.data_ptr() != other.data_ptr() and t.dtype == torch.float64 and tuple(t.shape) == (N, 11)
        assert t.device == env.device


def test_captured_graph_reads_current_levels(gpu):
    """in-place updates between replays of a captured graph are read by the next
    replay; the graph keeps the tensor it recorded alive"""
    import gc
    import weakref
    import invsim
    env = invsim.NetInvMgmtBacklogEnv(N, device=gpu)
    twin = invsim.NetInvMgmtBacklogEnv(N, device=gpu)
    lv1, lv2 = _levels("default", seed=10), _levels("default", seed=11)
    devs = [torch.from_numpy(lv1).to(gpu) for _ in range(2)]
    ag, ag_t = invsim.NetLevelsAgent(devs[0]), invsim.NetLevelsAgent(devs[1])
    env.reset(seed=2)
    twin.reset(seed=2)
    cyc = env._horizon() + 1
    g = env.capture(lambda: env.rollout_policy(ag, cyc, obs=True, actions=True))    # (warm-up: one eager cycle)
    twin.rollout_policy(ag_t, cyc, obs=True, actions=True)
    ref = weakref.ref(devs[0])
    for lv in (lv1, lv2, lv1):
        for d in devs:
            d.copy_(torch.from_numpy(lv))
        og = g.replay()
        oe = twin.rollout_policy(ag_t, cyc, obs=True, actions=True)
        torch.cuda.synchronize(gpu)
        for k in oe:
            _same(og[k], oe[k], f"{k}: replay against an eager run with the same values")
    assert bool(og["actions"].any())
    del ag, d
    devs.clear()
    gc.collect()
    assert ref() is not None, "the graph must keep the tensor it recorded"


def test_refusals(gpu):
    import invsim
    from invsim import _capi
    lib = _capi.lib()
    env = invsim.NetInvMgmtBacklogEnv(N, device=gpu, autoreset_mode="disabled")
    high = env._action_high()
    spec = _capi.PolicySpec(_capi.POLICY_KINDS["net_levels"], 0, 0.0, 0.0, high.ctypes.data)

    def launch(e, k=3):
        met = _metrics(e)
        return lib.invsim_rollout_policy(e._h, k, C.byref(spec), None, None, None, None, None, met.data_ptr(),
                                         e._stream())

    env.reset(seed=1)
    assert launch(env) == -22 and "no levels attached" in _capi.last_error(env._h)
    lv = torch.full((N, 11), 50.0, dtype=torch.float64, device=gpu)
    for other in (invsim.NewsvendorEnv(N, device=gpu), invsim.InvManagementBacklogEnv(N, device=gpu)):
        other.reset(seed=1)
        assert launch(other) == -22 and "NetInvMgmt" in _capi.last_error(other._h)
        assert lib.invsim_set_policy_net_levels(other._h, lv.data_ptr(), None) == -22
        assert "NetInvMgmt" in _capi.last_error(other._h)
        with pytest.raises(TypeError, match="NetInvMgmt"):
            other.rollout_policy(invsim.NetLevelsAgent([1.0]), 3)
        other.step(torch.zeros((N, other.action_dim), dtype=other.act_dtype, device=gpu))      # still usable
    # LEVELS stays InvMgmt's
    assert lib.invsim_set_policy_levels(env._h, lv.data_ptr(), None) == -22 and "InvMgmt" in _capi.last_error(env._h)
    same = invsim.NetInvMgmtBacklogEnv(N, device=gpu, autoreset_mode="same_step")
    same.reset(seed=1)
    with pytest.raises(_capi.InvsimError, match="SAME_STEP|final_obs"):
        same.rollout_policy(invsim.NetLevelsAgent(lv), 3)
    same.step(torch.zeros((N, 11), device=gpu))
    assert lib.invsim_capture_begin(env._h) == 0
    try:
        assert lib.invsim_set_policy_net_levels(env._h, lv.data_ptr(), None) == -22
        assert "cannot be captured" in _capi.last_error(env._h)
    finally:
        assert lib.invsim_capture_end(env._h, None) == 0
    assert launch(env) == -22, "the refused attach must not have attached"
    with pytest.raises(ValueError, match="shape"):
        env.rollout_policy(invsim.NetLevelsAgent(np.zeros((N, 10))), 3)
    nohigh = _capi.PolicySpec(_capi.POLICY_KINDS["net_levels"], 0, 0.0, 0.0, None)
    assert lib.invsim_set_policy_net_levels(env._h, lv.data_ptr(), None) == 0
    assert lib.invsim_rollout_policy(env._h, 3, C.byref(nohigh), None, None, None, None, None, None, env._stream()) == -22
    assert launch(env) == 0                                                # attached: the env was still at its reset
    assert lib.invsim_set_policy_net_levels(env._h, None, None) == 0      # detach
    assert launch(env) == -22
    # E = 44 > INVSIM_POLICY_MAX_ACTION
    wide = invsim.NetInvMgmtMasterEnv(N, device=gpu, graph=net_graphs.wide(), num_periods=8)
    assert wide.action_dim == 44
    wide.reset(seed=1)
    with pytest.raises(_capi.InvsimError, match=rf"\({_capi.INVSIM_ERANGE}\).*action_dim too large"):
        wide.rollout_policy(invsim.NetLevelsAgent(np.full(44, 50.0)), 3)
    o, r, te, tr, _ = wide.step(torch.zeros((N, 44), device=gpu))          # still usable
    assert tuple(o.shape) == (N, wide.obs_dim)


def test_evaluate_levels(gpu):
    import invsim
    from invsim.policies import evaluate_levels
    Cn, R, off = 3, 40, 1000
    base = np.asarray(invsim.NetLevelsAgent.from_mean_demand(invsim.NetInvMgmtBacklogEnv(1, device=gpu)).levels)
    lv = np.stack([base, 1.6 * base + 3.25, base])
    res = evaluate_levels(lv, invsim.NetInvMgmtBacklogEnv, n_episodes=R, seed_offset=off, device=gpu)
    for k in ("TotalReward", "Steps", "AvgServiceLevel", "TotalStockoutQty", "AvgEndingInv"):
        assert res[k].shape == (Cn, R), k
    tot = res["TotalReward"]
    assert np.array_equal(tot[0].view(np.uint64), tot[2].view(np.uint64)), "identical candidates, common seeds"
    assert not np.array_equal(tot[0], tot[1])
    assert (res["Steps"] == 30).all()
    for c in range(Cn):
        one = invsim.evaluate_agent(invsim.NetLevelsAgent(lv[c]), invsim.NetInvMgmtBacklogEnv, n_episodes=R,
                                    seed_offset=off, device=gpu)
        for k in ("TotalReward", "AvgServiceLevel", "TotalStockoutQty", "AvgEndingInv"):
            assert np.array_equal(one[k].view(np.uint64), res[k][c].view(np.uint64)), f"candidate {c} {k}"
        assert res["candidates"]["AvgReward"][c] == np.mean(one["TotalReward"])
    with pytest.raises(TypeError, match="level policies"):
        evaluate_levels(np.zeros((1, 1)), invsim.NewsvendorEnv, n_episodes=2, device=gpu)


def test_tune_levels(gpu):
    import invsim
    from invsim.policies import tune_levels
    kw = dict(n_episodes=8, population=16, iterations=3, seed=3, seed_offset=200, device=gpu)
    res = tune_levels(invsim.NetInvMgmtBacklogEnv, **kw)
    hist = res["history"]
    assert hist.shape == (3,) and res["levels"].shape == (11,) and res["TotalReward"].shape == (8,)
    assert (np.diff(hist) >= 0).all(), hist
    init = invsim.NetLevelsAgent.from_mean_demand(invsim.NetInvMgmtBacklogEnv(1, device=gpu))
    base = invsim.evaluate_agent(init, invsim.NetInvMgmtBacklogEnv, n_episodes=8, seed_offset=200, device=gpu)
    assert hist[0] >= np.mean(base["TotalReward"]), (hist, np.mean(base["TotalReward"]))
    assert hist[-1] == np.mean(res["TotalReward"])
    assert (res["levels"] >= 0).all() and (res["levels"] <= 1700.0).all()
    one = invsim.evaluate_agent(invsim.NetLevelsAgent(res["levels"]), invsim.NetInvMgmtBacklogEnv, n_episodes=8,
                                seed_offset=200, device=gpu)
    assert np.array_equal(one["TotalReward"].view(np.uint64), res["TotalReward"].view(np.uint64))
