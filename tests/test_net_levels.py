"""NetLevelsAgent without a GPU: from_mean_demand on the compiled topology, the
ABI pins, and self-checks of tests/net_levels_model.py: that the inputs the GPU
tests use exercise the rule (fractional positions, orders strictly inside the
bounds and orders of 0)."""
import os
import re

import numpy as np
import pytest

import net_graphs
import net_levels_model as model
from conftest import ROOT

DEFAULT_LEVELS = [60, 40, 30, 55, 100 / 3, 40, 65, 25 / 3, 10 / 3, 5, 25 / 3]
N, SEED = 200, 3


def _default_topology():
    from invsim.topology import compile_graph, default_graph
    g = default_graph()
    return compile_graph(g, 30, {(1, 0): np.zeros(30)}, {(1, 0): False})


def test_from_mean_demand_default_graph():
    from invsim.policies import NetLevelsAgent
    tp = _default_topology()
    agent = NetLevelsAgent.from_mean_demand(tp)
    np.testing.assert_allclose(np.asarray(agent.levels), DEFAULT_LEVELS, rtol=1e-12)
    assert agent.reorder is None and agent.name == "NetLevels"
    for sf in (0.5, 1.7):
        np.testing.assert_allclose(np.asarray(NetLevelsAgent.from_mean_demand(tp, sf).levels),
                                   sf * np.array(DEFAULT_LEVELS), rtol=1e-12)


def test_from_mean_demand_other_markets():
    """binomial n p, integers' half-open mean, geometric 1 / p, user_D's mean of
    max(0, round(x)), a market without a source; factory yields divide the flow"""
    from invsim.policies import NetLevelsAgent, _market_means
    from invsim.topology import compile_graph
    tp = compile_graph(net_graphs.mixed(T=12), 12)
    means = dict(zip(tp.retail_links, _market_means(tp)))
    assert means[(5, 0)] == 30 * 0.3 and means[(3, 0)] == 4.5
    assert means[(3, 8)] == np.mean(net_graphs.expected_user_demand(12))
    tc = compile_graph(net_graphs.chain(T=10), 10)
    mc = dict(zip(tc.retail_links, _market_means(tc)))
    assert mc[(2, 0)] == 1 / 0.2 and mc[(2, 7)] == 3.0 and mc[(3, 8)] == 0.0
    tm = compile_graph(net_graphs.minimal(T=8), 8)
    assert _market_means(tm)[0] == 4.0                      # integers [0, 9)
    # chain 10 -> 4 -> 1 -> 3 -> 2, one link into every node: every flow is the retailer's 8 per period
    lv = np.asarray(NetLevelsAgent.from_mean_demand(tc).levels)
    L = np.asarray(tc.tables["L"])[:len(tc.reorder_links)]
    np.testing.assert_allclose(lv, (L + 1) * 8.0, rtol=1e-12)
    # mixed: node 3 (index 0) buys over (5, 3) and (6, 3); its rate is 4.5 + the user_D mean
    lm = np.asarray(NetLevelsAgent.from_mean_demand(tp).levels)
    k = tp.reorder_links.index((5, 3))
    np.testing.assert_allclose(lm[k], (0 + 1) * (4.5 + means[(3, 8)]) / 2, rtol=1e-12)
    assert np.isfinite(lm).all() and (lm > 0).all()


def test_abi_names():
    from invsim import _capi
    src = open(os.path.join(ROOT, "include", "invsim.h")).read()
    assert re.search(r"#define\s+INVSIM_POLICY_NET_LEVELS\s+8\b", src)
    assert "int invsim_set_policy_net_levels(invsim_handle *h, const double *levels, const double *reorder);" in src
    assert _capi.POLICY_KINDS["net_levels"] == 8 and _capi.POLICY_KINDS["levels"] == 7
    assert "invsim_set_policy_net_levels" in _capi.EXPORTS
    assert re.search(r"#define\s+INVSIM_ABI_VERSION\s+4\b", src) and _capi.ABI_VERSION == 4


def test_levels_agent_unchanged_and_type_errors():
    import invsim
    from invsim import _capi

    class Fake:
        family = _capi.INVSIM_INVMGMT
    with pytest.raises(TypeError, match="NetInvMgmt"):
        invsim.NetLevelsAgent([1.0]).tensors(Fake())
    Fake.family = _capi.INVSIM_NETINVMGMT
    with pytest.raises(TypeError, match="InvManagement"):
        invsim.LevelsAgent([1.0]).tensors(Fake())
    assert issubclass(invsim.NetLevelsAgent, invsim.LevelsAgent)


def _run(oracle, graph, T, levels, reorder=None, backlog=True, alpha=1.0):
    g = None if graph is None else graph
    orc = oracle.OracleNet(N, graph=g, num_periods=T, backlog=backlog, alpha=alpha)
    orc.seed(range(SEED, SEED + N))
    high = model.action_high(oracle.default_graph() if g is None else g)
    loop = model.ClosedLoop(orc, levels, reorder, high)
    return loop, loop.run(T), high


def test_model_exercises_fractional_positions(oracle):
    """yields 0.8 and 0.55 make X fractional: the f64 summation order of the position shows"""
    lv = np.random.default_rng(0).uniform(0.0, 120.0, size=(N, 10))
    loop, out, high = _run(oracle, net_graphs.mixed(T=12), 12, lv, alpha=0.93)
    X = np.stack(loop.xs)
    assert (X != np.rint(X)).any(), "no fractional X entry: the mixed graph's yields are not exercised"
    inside, zero = model.shares(out["actions"], high)
    assert inside >= 0.10 and zero >= 0.10, (inside, zero)


@pytest.mark.parametrize("case", ["default", "default_reorder", "custom", "chain"])
def test_model_inputs_are_not_degenerate(oracle, case):
    """levels ~ U(0, 120) from default_rng(0), 200 envs seeded 3..202: at least
    10 % of the orders strictly inside (0, high) and at least 10 % equal to 0"""
    graph, T = {"default": (None, 30), "default_reorder": (None, 30), "custom": (oracle.custom_graph(), 30),
                "chain": (net_graphs.chain(T=10), 10)}[case]
    E = 11 if graph is None else sum(1 for e in graph.edges() if "L" in graph.edges[e])
    lv = np.random.default_rng(0).uniform(0.0, 120.0, size=(N, E))
    loop, out, high = _run(oracle, graph, T, lv, 0.8 * lv if case == "default_reorder" else None)
    if case.startswith("default"):
        assert high.tolist() == [1700.0] * 11
    inside, zero = model.shares(out["actions"], high)
    assert inside >= 0.10 and zero >= 0.10, (inside, zero)
    assert (out["metrics"][:, 1] == T).all() and out["truncated"][-1].all() and not out["truncated"][:-1].any()


def test_model_rule_edge_values():
    """the rule's corners on a hand-made state: NaN / inf levels and reorder points, the cap, the rounding"""
    pur, rl_node = np.array([0, 0, 1]), np.array([0])
    X = np.array([[10.25, 3.0]]); U = np.array([[1.5]]); Y = np.array([[2.0, 4.0, 0.125]])
    pos = model.positions(X, U, Y, pur, rl_node)
    assert pos.tolist() == [[((10.25 + 2.0) + 4.0) - 1.5, 3.0 + 0.125]]
    high = np.array([50.0, 50.0, 50.0], np.float32)
    lv = lambda *v: np.array([v], np.float64)  # noqa: E731
    act = lambda levels, ro=None: model.actions(X, U, Y, levels, ro, high, pur, rl_node)[0].tolist()  # noqa: E731
    assert act(lv(20.0, np.inf, np.nan)) == [5.25, 50.0, 0.0]
    assert act(lv(-np.inf, -3.0, 1e300)) == [0.0, 0.0, 50.0]
    assert act(lv(14.75 + 0.1, 14.75, 3.125 + 1e-9)) == [float(np.float32((14.75 + 0.1) - 14.75)), 0.0,
                                                          float(np.float32((3.125 + 1e-9) - 3.125))]
    assert act(lv(20.0, 20.0, 20.0), lv(14.75, np.nan, np.inf)) == [0.0, 0.0, 16.875]       # strict <, NaN, +inf
    assert act(lv(20.0, 20.0, 20.0), lv(14.75 + 1e-9, -np.inf, 3.2)) == [5.25, 0.0, 16.875]
