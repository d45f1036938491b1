"""GPU: the generic NetInvMgmt kernel (net_run_kernel / net_step_lds, fed by
invsim.topology.compile_graph) on graphs outside the reference's two built-in
ones (tests/net_graphs.py): yields below 1, a factory feeding a factory,
scrambled node and edge order, an interior L = 0 link, a link with L > T, two
markets on one retailer, the user_D replay, and a launch that asks for more
than 64 KB of dynamic LDS.  test_net_graphs_model.py checks on the CPU that
the goldens reach those branches.

Everything is bit-exact: f32 obs bits, f64 reward and record bits, flags,
demands.  References: the goldens recorded from the reference env, the C
oracle at 197 envs (three full 64-env groups and a group of 5), the cohort
oracle for staggered periods, oracle/agents.py for the in-kernel policy.
"""
import numpy as np
import pytest
import torch

import agents
import net_graphs
import staggered
from conftest import load_golden
from net_graphs import GRAPHS, NET_GRAPH_GOLDENS, expected_user_demand
from test_gpu_staggered import SEED, _Dev, _drive, _net_make, _variant

pytestmark = pytest.mark.gpu

N = staggered.N
PERIODS = {"mixed": 12, "chain": 10, "wide": 8, "minimal": 8}
ALPHA = 0.93


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize]) if x.dtype.kind == "f" else x


def _eq(got, exp, what):
    """bit equality; a mismatch reports where and, for floats, max |diff|, and fails"""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, f"{what}: shape {got.shape} vs {exp.shape}"
    exp = exp.astype(got.dtype)
    if np.array_equal(_bits(got), _bits(exp)):
        return
    bad = np.argwhere(_bits(got) != _bits(exp))[:4].tolist()
    msg = f"{what}: first mismatches at {bad}: got {[got[tuple(b)] for b in bad]}, expected {[exp[tuple(b)] for b in bad]}"
    if got.dtype.kind == "f":
        msg += f", max|diff|={np.nanmax(np.abs(got.astype(np.float64) - exp.astype(np.float64)))}"
    pytest.fail(msg)


def _np(x):
    return x.cpu().numpy()


def _env(gpu, graph, n, backlog=True, T=None, alpha=ALPHA, **kw):
    import invsim
    T = PERIODS[graph] if T is None else T
    env = invsim.NetInvMgmtMasterEnv(n, device=gpu, graph=GRAPHS[graph](net_graphs.by_name, T), num_periods=T,
                                     backlog=backlog, alpha=alpha, **kw)
    assert env.kernel_variant == 0, "the generic table-walking kernel"
    return env


def _oracle(oracle, graph, n, seed, backlog=True, T=None, alpha=ALPHA):
    T = PERIODS[graph] if T is None else T
    orc = oracle.OracleNet(n, graph=GRAPHS[graph](net_graphs.by_name, T), num_periods=T, backlog=backlog,
                           alpha=alpha)
    orc.seed(range(seed, seed + n))
    return orc


def _actions(rng, shape):
    a = rng.uniform(-5.0, 60.0, size=shape)
    u = rng.random(shape)
    a[u < 0.2] = np.round(a[u < 0.2]) + 0.5            # exact .5 ties
    a[u > 0.99] = 1e30                                 # far past any inventory
    return a.astype(np.float32)


# ---------------------------------------------------------------- the reference's goldens
@pytest.mark.parametrize("name", NET_GRAPH_GOLDENS)
def test_net_graph_golden(gpu, name):
    fx, cfg = load_golden(name)
    n, T, topo = cfg["n_env"], cfg["ep_len"], cfg["topology"]
    env = _env(gpu, cfg["graph"], n, cfg["backlog"], cfg["num_periods"], cfg["alpha"], autoreset_mode="disabled",
               record_demand=True, record_info=True)
    assert env.obs_dim == topo["obs_dim"]
    assert [int(j) for j in env.main_nodes] == topo["main_nodes"]
    assert [list(e) for e in env.reorder_links] == topo["reorder_links"]
    assert [list(e) for e in env.retail_links] == topo["retail_links"]
    J, E, RL = len(env.main_nodes), len(env.reorder_links), len(env.retail_links)
    if cfg["graph"] == "wide":
        lds = net_graphs.lds_bytes(J, E, RL, sum(env.lead_times.values()))
        assert 64 * 1024 < lds <= 160 * 1024, "a launch with more than 64 KB of dynamic LDS"
    for ep in range(cfg["n_ep"]):
        obs, _ = env.reset(seed=cfg["base_seed"]) if ep == 0 else env.reset()
        _eq(_np(obs), fx["reset_obs"][:, ep], f"reset obs ep {ep}")
        for k in range(T):
            s = ep * T + k
            o, r, te, tr, info = env.step(torch.from_numpy(np.ascontiguousarray(fx["actions"][:, s])).to(gpu))
            _eq(_np(o), fx["obs"][:, s], f"obs step {s}")
            _eq(_np(r), fx["reward"][:, s], f"reward step {s}")
            assert not _np(te).any()
            _eq(_np(tr), fx["truncated"][:, s], f"truncated step {s}")
            _eq(_np(info["demand"]).reshape(n, RL), fx["D"][:, s].astype(np.int64), f"demand step {s}")
            for key, gk in (("sales", "S"), ("unfulfilled", "U"), ("inventory", "X"), ("replenishment", "R"),
                            ("pipeline", "Y"), ("profit", "P")):
                _eq(_np(info[key]), fx[gk][:, s], f"record {key} step {s}")


# ---------------------------------------------------------------- vs the C oracle at 197 envs
def _expected_rows(orc, mode, T, acts):
    """The oracle's answer to each call: (obs, reward, truncated, demand | None,
    final obs | None, info).  next_step: the call after a done step is the reset
    row; same_step: the done step returns the reset obs and the final obs apart."""
    t, rows = 0, []
    for a in acts:
        if mode == "next_step" and t >= T:
            rows.append((orc.reset(), np.zeros(orc.n), np.zeros(orc.n, bool), None, None, None))
            t = 0
            continue
        o, r, tr, info = orc.step(a, info=True)
        t += 1
        assert tr.all() == (t == T)
        fobs = None
        if mode == "same_step" and t == T:
            fobs, o, t = o, orc.reset(), 0
        rows.append((o, r, tr, info["D"].astype(np.int64), fobs, info))
    return rows


@pytest.mark.parametrize("drive,mode", [("steps", "next_step"), ("steps", "same_step"), ("rollout", "next_step")])
@pytest.mark.parametrize("backlog", [True, False])
@pytest.mark.parametrize("graph", ["mixed", "chain", "wide"])
def test_net_graph_vs_oracle_197(gpu, oracle, graph, backlog, drive, mode):
    """Two episodes and three periods of a third: by single steps (same_step
    with final_obs), and by rollouts whose chunks straddle the episode ends."""
    T = PERIODS[graph]
    env = _env(gpu, graph, N, backlog, autoreset_mode=mode, record_demand=True)
    orc = _oracle(oracle, graph, N, 610, backlog)
    RL = len(env.retail_links)
    obs, _ = env.reset(seed=610)
    _eq(_np(obs), orc.reset(), "reset obs")
    calls = 2 * T + 3 + (2 if mode == "next_step" else 0)
    acts = _actions(np.random.default_rng(21), (calls, N, env.action_dim))
    rows = _expected_rows(orc, mode, T, acts)
    assert sum(r[3] is None for r in rows) == (2 if mode == "next_step" else 0)
    assert sum(r[4] is not None for r in rows) == (2 if mode == "same_step" else 0)

    def check(k, o, r, te, tr, dem=None, fobs=None, fmask=None):
        e_obs, e_rew, e_tr, e_dem, e_fobs, _ = rows[k]
        _eq(o, e_obs, f"obs call {k}")
        _eq(r, e_rew, f"reward call {k}")
        assert not te.any(), k
        _eq(tr, e_tr, f"truncated call {k}")
        if dem is not None and e_dem is not None:
            _eq(dem.reshape(N, RL), e_dem, f"demand call {k}")
        if mode == "same_step":
            _eq(fmask, e_tr, f"_final_obs call {k}")
            if e_fobs is not None:
                _eq(fobs, e_fobs, f"final_obs call {k}")

    if drive == "steps":
        for k in range(calls):
            o, r, te, tr, info = env.step(torch.from_numpy(acts[k]).to(gpu))
            fin = (_np(info["final_obs"]), _np(info["_final_obs"])) if mode == "same_step" else (None, None)
            check(k, _np(o), _np(r), _np(te), _np(tr), _np(info["demand"]), *fin)
    else:
        K = 5 if T % 5 else 4
        assert any(c < T < c + K for c in range(0, calls, K)), "a chunk straddles the first episode end"
        for c in range(0, calls, K):
            out = [_np(x) for x in env.rollout(torch.from_numpy(acts[c:c + K]).to(gpu))]
            for q in range(out[0].shape[0]):
                check(c + q, *(x[q] for x in out))
            last = c + out[0].shape[0] - 1
            if rows[last][3] is not None:          # the demand record holds the launch's last period
                _eq(_np(env._demand).reshape(N, RL), rows[last][3], f"demand call {last}")
    info = rows[-1][5]
    st = env.state_fields()
    _eq(_np(st["X"].view(torch.float64)).T, info["X"], "final X")
    _eq(_np(st["U"].view(torch.float64)).T[:, :RL], info["U"], "final U")
    _eq(_np(st["Y"].view(torch.float64)).T, info["Y"], "final Y")
    assert (info["X"] != np.rint(info["X"])).any() or graph == "chain", "fractional inventory reached"


# ---------------------------------------------------------------- staggered periods
STAGGERED = [("mixed", True, "next_step"), ("mixed", False, "same_step"), ("mixed", True, "disabled"),
             ("wide", True, "next_step"), ("wide", False, "same_step")]


@pytest.mark.parametrize("graph,backlog,mode", STAGGERED)
def test_net_graph_staggered(gpu, oracle, graph, backlog, mode):
    """test_gpu_staggered.test_net's script (masked resets, per-env periods, the
    TU = false instantiation of net_run_kernel) on mixed and wide."""
    T = PERIODS[graph]
    g = GRAPHS[graph](net_graphs.by_name, T)
    h = staggered.make(oracle, "net", SEED, _variant(mode), mode, graph=g, num_periods=T, backlog=backlog)
    env = _net_make(gpu, mode, g, T, backlog)()
    assert env.kernel_variant == 0
    _drive([_Dev(env, graph)], h, staggered.script(h, np.random.default_rng(4)))


# ---------------------------------------------------------------- the in-kernel constant-order policy
def test_constant_order_on_mixed_vs_oracle(gpu, oracle):
    """rollout_policy and evaluate_agent on mixed (the POL instantiation): the
    agent's order is 52.5 on every link, a half-to-even tie; the 5 + J metrics
    columns sum fractional X and S."""
    import invsim
    T, n = PERIODS["mixed"], N
    env = _env(gpu, "mixed", n, True, autoreset_mode="next_step")
    agent = invsim.ConstantOrderAgent(0.07)
    a = agent.action(env)
    assert a.dtype == np.float32 and (a == 52.5).all()
    orc = _oracle(oracle, "mixed", n, 44)
    o0 = orc.reset()
    env.reset(seed=44)
    met = torch.zeros((n, invsim.policies.metrics_dim(env)), dtype=torch.float64, device=gpu)
    assert met.shape[1] == 5 + len(env.main_nodes)
    out = env.rollout_policy(agent, T, obs=True, actions=True, metrics=met)
    e_rew, e_obs, e_sum = agents.run_net(orc, o0, T, a)
    _eq(_np(out["actions"]), np.broadcast_to(a, (T, n, len(a))), "actions")
    _eq(_np(out["obs"]), e_obs, "obs")
    _eq(_np(out["reward"]), e_rew, "reward")
    _eq(_np(met), e_sum, "metrics")
    assert (e_sum[:, 5:] != np.rint(e_sum[:, 5:])).any(), "fractional X in the metrics"
    # metrics only, chained across the NEXT_STEP autoreset
    met2 = torch.zeros_like(met)
    env.reset(seed=44)
    env.rollout_policy(agent, 5, metrics=met2)
    env.rollout_policy(agent, T - 5, metrics=met2)
    assert torch.equal(met2, met)
    assert (env.rollout_policy(agent, 2, obs=True)["reward"][0] == 0).all()      # the reset row
    # evaluate_agent: one episode per env, the reference's summary columns
    res = invsim.evaluate_agent(agent, invsim.NetInvMgmtMasterEnv,
                                dict(graph=GRAPHS["mixed"](), num_periods=T, backlog=True, alpha=ALPHA),
                                n_episodes=n, seed_offset=44, device=gpu)
    _eq(res["TotalReward"], e_sum[:, 0], "TotalReward")
    assert res["Steps"].tolist() == [T] * n
    sl = [s / max(1e-6, d) if d > 1e-6 else 1.0 for s, d in zip(e_sum[:, 3], e_sum[:, 2])]
    _eq(res["AvgServiceLevel"], np.array(sl), "AvgServiceLevel")
    _eq(res["TotalStockoutQty"], e_sum[:, 4], "TotalStockoutQty")
    _eq(res["AvgEndingInv"], np.array([np.sum(x / T) / x.shape[0] for x in e_sum[:, 5:]]), "AvgEndingInv")


def test_constant_order_refused_past_32_links(gpu, oracle):
    """wide has 44 reorder links, more than the in-kernel constant policy holds:
    the call is refused before any launch and the env steps on, bit-exact."""
    import invsim
    from invsim._capi import InvsimError
    env = _env(gpu, "wide", 64, True)
    orc = _oracle(oracle, "wide", 64, 9)
    _eq(_np(env.reset(seed=9)[0]), orc.reset(), "reset obs")
    with pytest.raises(InvsimError, match="action_dim too large for a CONSTANT policy"):
        env.rollout_policy(invsim.ConstantOrderAgent(0.07), 2)
    a = _actions(np.random.default_rng(23), (64, env.action_dim))
    o, r, _, _, _ = env.step(torch.from_numpy(a).to(gpu))
    e_o, e_r, _ = orc.step(a)
    _eq(_np(o), e_o, "obs after the refused policy rollout")
    _eq(_np(r), e_r, "reward after the refused policy rollout")


# ---------------------------------------------------------------- the fast stream (no oracle for it)
def test_fast_stream_on_mixed(gpu):
    """demand_stream="philox": a rollout equals the same calls made one by one,
    and the user_D market replays its table under both streams."""
    T = PERIODS["mixed"]
    e1, e2 = (_env(gpu, "mixed", N, True, demand_stream="philox", record_demand=True) for _ in range(2))
    e3 = _env(gpu, "mixed", N, True, demand_stream="numpy", record_demand=True)
    for e in (e1, e2, e3):
        e.reset(seed=5)
    r_user = e1.retail_links.index((3, 8))
    table = expected_user_demand(T)
    K = 2 * T + 5
    acts = torch.from_numpy(_actions(np.random.default_rng(22), (K, N, e1.action_dim))).to(gpu)
    o1, r1, _, t1 = e1.rollout(acts)
    t, drawn = 0, []
    for k in range(K):
        o, r, _, tr, info = e2.step(acts[k])
        assert torch.equal(o, o1[k]) and torch.equal(r.view(torch.int64), r1[k].view(torch.int64)), k
        assert torch.equal(tr, t1[k]), k
        d3 = e3.step(acts[k])[4]["demand"]
        if t >= T:                                   # the NEXT_STEP reset row: no demand
            t = 0
            continue
        for d in (info["demand"], d3):
            assert (d[:, r_user] == table[t]).all(), (k, t)
        drawn.append(_np(info["demand"]))
        t += 1
    assert torch.equal(e1.get_state(), e2.get_state())
    drawn = np.stack(drawn)
    others = [r for r in range(drawn.shape[2]) if r != r_user]
    assert all(len(np.unique(drawn[:, :, r])) > 3 for r in others), "the sampled markets do draw"


# ---------------------------------------------------------------- create-time limits
def _still_works(gpu, oracle):
    env = _env(gpu, "minimal", 64, True, alpha=1.0)
    orc = _oracle(oracle, "minimal", 64, 3, alpha=1.0)
    _eq(_np(env.reset(seed=3)[0]), orc.reset(), "reset obs after a refused create")
    a = np.full((64, 1), 6.5, np.float32)
    o, r, _, _, _ = env.step(torch.from_numpy(a).to(gpu))
    e_o, e_r, _ = orc.step(a)
    _eq(_np(o), e_o, "obs after a refused create")
    _eq(_np(r), e_r, "reward after a refused create")


_series = net_graphs.series


def test_create_time_limits(gpu, oracle):
    import invsim
    from invsim._capi import INVSIM_ERANGE, InvsimError
    erange = rf"\({INVSIM_ERANGE}\)"
    with pytest.raises(InvsimError, match=erange + ".*topology too large for the LDS scratch"):
        invsim.NetInvMgmtMasterEnv(N, device=gpu, graph=net_graphs.too_large(), num_periods=8)
    _still_works(gpu, oracle)
    with pytest.raises(InvsimError, match=erange + ".*topology size out of supported range"):
        invsim.NetInvMgmtMasterEnv(N, device=gpu, graph=_series(65), num_periods=8)
    _still_works(gpu, oracle)
    assert invsim.NetInvMgmtMasterEnv(4, device=gpu, graph=_series(1, L=255), num_periods=8).obs_dim == 257
    with pytest.raises(InvsimError, match=erange + ".*max 255"):
        invsim.NetInvMgmtMasterEnv(N, device=gpu, graph=_series(1, L=256), num_periods=8)
    _still_works(gpu, oracle)
