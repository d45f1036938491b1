"""CPU: NetInvMgmt on graphs outside the reference's two built-in ones
(tests/net_graphs.py) against goldens recorded from the reference
(tests/golden/gen_goldens.py graphs).  No GPU needed.

* the C oracle reproduces every golden bit for bit (obs, reward, X/U/D/R/Y/P
  and the market sales S);
* invsim.topology.compile_graph reproduces the golden's node and link lists and
  agrees with the oracle's own tables entry for entry;
* the goldens reach the branches the built-in graphs never reach (yield < 1,
  capacity and yield caps, shared suppliers, an interior L = 0 link, L > T,
  the user_D replay, adjacency-order sums), so that parity means something.
"""
import numpy as np
import pytest

import net_graphs
from conftest import load_golden
from net_graphs import GRAPHS, NET_GRAPH_GOLDENS, expected_user_demand

MIXED = [n for n in NET_GRAPH_GOLDENS if "mixed" in n]


def _bits_equal(a, b):
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b).astype(a.dtype)
    return np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _graph(cfg):
    return GRAPHS[cfg["graph"]](net_graphs.by_name, cfg["num_periods"])


def _topology(cfg):
    """The tables of the device env: it compiles its own copy of the graph
    (network_management.py:77)."""
    from invsim.topology import compile_graph
    return compile_graph(_graph(cfg).copy(), cfg["num_periods"])


def test_golden_names_match_cases():
    for name in NET_GRAPH_GOLDENS:
        fx, cfg = load_golden(name)
        builder, T, backlog, alpha = net_graphs.GOLDEN_CASES[name[len("net_graph_"):]]
        assert (cfg["graph"], cfg["num_periods"], cfg["backlog"], cfg["alpha"]) == (builder, T, backlog, alpha)
        assert cfg["n_env"] >= 4 and cfg["ep_len"] == T
    assert load_golden("net_graph_mixed_2ep")[1]["n_ep"] == 2


# ---------------------------------------------------------------- oracle vs golden
@pytest.mark.parametrize("name", NET_GRAPH_GOLDENS)
def test_oracle_net_graph_golden(oracle, name):
    fx, cfg = load_golden(name)
    env = oracle.OracleNet(cfg["n_env"], graph=_graph(cfg), num_periods=cfg["num_periods"],
                           backlog=cfg["backlog"], alpha=cfg["alpha"])
    assert env.obs_dim == cfg["topology"]["obs_dim"]
    n, L = cfg["n_env"], cfg["ep_len"]
    env.seed([cfg["base_seed"] + i for i in range(n)])
    for ep in range(cfg["n_ep"]):
        assert _bits_equal(env.reset(), fx["reset_obs"][:, ep])
        for k in range(L):
            s = ep * L + k
            o, r, tr, info = env.step(fx["actions"][:, s], info=True)
            assert _bits_equal(o, fx["obs"][:, s]), f"obs step {s}"
            assert _bits_equal(r, fx["reward"][:, s]), f"reward step {s}"
            assert np.array_equal(tr, fx["truncated"][:, s])
            for key in ("X", "U", "D", "R", "Y", "P", "S"):
                assert _bits_equal(info[key], fx[key][:, s]), (key, s)


# ---------------------------------------------------------------- topology vs golden
@pytest.mark.parametrize("name", NET_GRAPH_GOLDENS)
def test_compile_graph_vs_golden_and_oracle_tables(oracle, name):
    _, cfg = load_golden(name)
    tp, topo = _topology(cfg), cfg["topology"]
    assert [int(j) for j in tp.main_nodes] == topo["main_nodes"]
    assert [list(e) for e in tp.reorder_links] == topo["reorder_links"]
    assert [list(e) for e in tp.retail_links] == topo["retail_links"]
    assert tp.obs_dim == topo["obs_dim"]
    orc = oracle.OracleNet(1, graph=_graph(cfg), num_periods=cfg["num_periods"]).topo
    assert (orc["main"], orc["reorder"], orc["retail_links"]) == (tp.main_nodes, tp.reorder_links, tp.retail_links)
    t, ot = tp.tables, orc["tables"]
    for j in range(orc["J"]):
        s0, s1 = t["succ_ptr"][j], t["succ_ptr"][j + 1]
        assert s1 - s0 == ot["succ_n"][j]
        assert t["succ_kind"][s0:s1].tolist() == ot["succ_kind"][j, :s1 - s0].tolist(), j
        assert t["succ_idx"][s0:s1].tolist() == ot["succ_idx"][j, :s1 - s0].tolist(), j
        p0, p1 = t["pred_ptr"][j], t["pred_ptr"][j + 1]
        assert p1 - p0 == ot["pred_n"][j]
        assert t["pred_idx"][p0:p1].tolist() == ot["pred_idx"][j, :p1 - p0].tolist(), j
    for key in ("I0", "h", "C", "o", "v", "is_factory", "is_retail", "sup", "pur", "L", "sup_is_factory", "lp",
                "lg", "rl_node", "rl_p", "rl_b", "rl_user", "user_D"):
        assert t[key].dtype == ot[key].dtype and np.array_equal(t[key], ot[key]), key
    live = t["rl_user"] == 0                             # a replayed market's sampler is never read
    for key in ("rl_dist", "rl_lam", "rl_n", "rl_high", "rl_dp"):
        assert np.array_equal(t[key][live], ot[key][live]), key


def test_adjacency_order_is_not_sorted_order():
    """What the mutation "walk the successors sorted" would change: in mixed
    and wide some node's successor list and some node's predecessor list (of
    the env's copy of the graph) are out of sorted order."""
    for name in ("net_graph_mixed_backlog", "net_graph_wide"):
        _, cfg = load_golden(name)
        t = _topology(cfg).tables
        J = len(t["succ_ptr"]) - 1
        key = lambda k, x: 2 ** 20 * int(k) + int(x)     # noqa: E731  reorder links before market links
        succ = [[key(k, x) for k, x in zip(t["succ_kind"][a:b], t["succ_idx"][a:b])]
                for a, b in zip(t["succ_ptr"][:J], t["succ_ptr"][1:])]
        pred = [t["pred_idx"][a:b].tolist() for a, b in zip(t["pred_ptr"][:J], t["pred_ptr"][1:])]
        assert any(s != sorted(s) for s in succ) and any(p != sorted(p) for p in pred), name
        assert cfg["topology"]["retail_links"] != sorted(cfg["topology"]["retail_links"])


# ---------------------------------------------------------------- coverage conditions
def _start_X(fx, cfg, t):
    """X[t] before each recorded step: I0 at an episode's first step, else the previous X[t+1]."""
    Xs = np.empty_like(fx["X"])
    Xs[:, 1:] = fx["X"][:, :-1]
    Xs[:, ::cfg["ep_len"]] = t["I0"]
    return Xs


def _replay_orders(t, Xs, act, R):
    """The order loop of one env and period (network_management.py:448-490) over
    sorted links, checked against the recorded R.  Returns per link the set of
    caps that bound it: 'C' capacity, 'v' yield * available with v < 1, 'cut'
    what an earlier link of the same supplier consumed."""
    cons = np.zeros(len(t["I0"]))
    flags = []
    for k in range(len(t["sup"])):
        req = max(0.0, float(np.rint(np.float64(act[k]))))
        sp = int(t["sup"][k])
        fl = set()
        if sp >= 0:
            def avail(c):
                oav = max(0.0, Xs[sp] - c)
                return min(oav, t["C"][sp], t["v"][sp] * oav) if t["sup_is_factory"][k] else oav
            a, a0 = avail(cons[sp]), avail(0.0)
            f = min(req, a)
            if t["sup_is_factory"][k] and f > 0:
                oav = max(0.0, Xs[sp] - cons[sp])
                if f == t["C"][sp] and req > f and t["v"][sp] * oav > f:
                    fl.add("C")
                if t["v"][sp] < 1 and f == t["v"][sp] * oav and f < req and f < t["C"][sp]:
                    fl.add("v")
            if cons[sp] > 0 and f < min(req, a0):
                fl.add("cut")
            cons[sp] += f / t["v"][sp]
        else:
            f = req
        assert f == R[k], ("order replay", k, f, R[k])
        flags.append(fl)
    return flags, cons


@pytest.mark.parametrize("name", MIXED + ["net_graph_wide"])
def test_goldens_reach_yield_capacity_and_shared_supplier_caps(name):
    fx, cfg = load_golden(name)
    t = _topology(cfg).tables
    Xs = _start_X(fx, cfg, t)
    seen = set()
    for i in range(cfg["n_env"]):
        for s in range(fx["X"].shape[1]):
            flags, _ = _replay_orders(t, Xs[i, s], fx["actions"][i, s], fx["R"][i, s])
            seen |= set().union(*flags)
    assert seen == {"C", "v", "cut"}, seen
    X = fx["X"]
    assert (X != np.rint(X)).any(), "fractional on-hand inventory (cons += f / v with v < 1)"
    assert (fx["obs"] != np.rint(fx["obs"])).any(), "the f32 obs carries a fraction"
    assert (t["v"][t["is_factory"] == 1] < 1).any()
    fac = t["is_factory"] == 1
    assert (fac[t["sup"]] & fac[t["pur"]] & (t["sup"] >= 0)).any(), "a factory feeds a factory"


@pytest.mark.parametrize("name", MIXED)
def test_mixed_interior_l0_link_and_link_longer_than_the_episode(name):
    """Retailer 3 is reached by (5, 3) with L = 0 and (6, 3) with L = 20 > T = 12
    only.  Units bought over (5, 3) are sold to the markets in the same period;
    (6, 3) fills its pipeline and never delivers."""
    fx, cfg = load_golden(name)
    tp = _topology(cfg)
    t, T = tp.tables, cfg["ep_len"]
    j3 = tp.main_nodes.index(3)
    k53, k63 = tp.reorder_links.index((5, 3)), tp.reorder_links.index((6, 3))
    r38, r30 = tp.retail_links.index((3, 8)), tp.retail_links.index((3, 0))
    assert t["L"][k53] == 0 and t["L"][k63] > T and r38 < r30
    assert t["sup"][k53] >= 0 and t["is_retail"][t["sup"][k53]], "the L = 0 link's supplier is itself a retailer"
    assert sorted(tp.retail_links.index(e) for e in tp.retail_links if e[0] == 3) == [r38, r30], "two markets"
    Xs = _start_X(fx, cfg, t)[:, :, j3]
    R53, S38, S30 = fx["R"][:, :, k53], fx["S"][:, :, r38], fx["S"][:, :, r30]
    # X[t+1] = ((X[t] + R[t, (5, 3)]) - S[(3, 8)]) - S[(3, 0)]: nothing ever arrives over (6, 3)
    assert _bits_equal(((Xs + R53) - S38) - S30, fx["X"][:, :, j3])
    assert ((S38 + S30 > np.maximum(Xs, 0)) & (R53 > 0)).any(), "same-period sale of an L = 0 arrival"
    R63, Y63 = fx["R"][:, :, k63], fx["Y"][:, :, k63]
    assert (R63 > 0).any()
    for ep in range(cfg["n_ep"]):
        sl = slice(ep * T, (ep + 1) * T)
        assert _bits_equal(np.cumsum(R63[:, sl], axis=1), Y63[:, sl]), "Y only grows on the L > T link"


@pytest.mark.parametrize("name", MIXED + ["net_graph_wide"])
def test_user_d_market_replays_the_rounded_table(name):
    fx, cfg = load_golden(name)
    tp = _topology(cfg)
    (r,) = np.flatnonzero(tp.tables["rl_user"])
    exp = np.array(expected_user_demand(cfg["ep_len"]) * cfg["n_ep"], np.float64)
    tab = tp.tables["user_D"][r]
    assert 2.5 in tab and 3.5 in tab and (tab < 0).any(), "a tie each way and a negative entry"
    assert exp[list(tab).index(2.5)] == 2 and exp[list(tab).index(3.5)] == 4 and exp[int(np.argmin(tab))] == 0
    assert np.array_equal(fx["D"][:, :, r], np.broadcast_to(exp, fx["D"][:, :, r].shape))


def test_backlog_and_lost_sales_goldens():
    fx, cfg = load_golden("net_graph_mixed_backlog")
    assert cfg["backlog"] and (fx["U"] > 0).any() and cfg["alpha"] == 0.93
    fx, cfg = load_golden("net_graph_mixed_lost")
    assert not cfg["backlog"] and (fx["U"] == 0).all() and (fx["S"] < fx["D"]).any(), "sales are lost"
    a = load_golden("net_graph_mixed_2ep")[0]["actions"]
    tie = np.abs(a - np.floor(a)) == 0.5
    assert 0.15 < tie.mean() < 0.25 and a.min() < 0 and a.max() > 55


def test_mixed_revenue_sum_depends_on_adjacency_order():
    """Node 7 sells over three links, inserted (7, 6), (7, 4), (7, 5).  The
    reference sums p * S in that adjacency order (network_management.py:582);
    sorted link order gives other f64 bits in some (env, period)."""
    fx, cfg = load_golden("net_graph_mixed_backlog")
    tp = _topology(cfg)
    t = tp.tables
    j = tp.main_nodes.index(7)
    adj = t["succ_idx"][t["succ_ptr"][j]:t["succ_ptr"][j + 1]].tolist()
    assert [tp.reorder_links[k] for k in adj] == [(7, 6), (7, 4), (7, 5)]
    terms = t["lp"][None, None, :] * fx["R"]
    total = lambda order: ((0.0 + terms[:, :, order[0]]) + terms[:, :, order[1]]) + terms[:, :, order[2]]  # noqa: E731
    assert (total(adj) != total(sorted(adj))).any()


# ---------------------------------------------------------------- demand sources of chain and minimal
def _npg(seed):
    return np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed)))


def test_chain_sample_path_table_is_ignored_and_sourceless_market_draws_nothing():
    """Per period the env's generator is asked for one Poisson(3) draw (the
    (2, 7) market, whose user_D table is switched off by sample_path=True) and
    one geometric(0.2) draw, in that edge order; (3, 8) has no source."""
    fx, cfg = load_golden("net_graph_chain")
    links = [tuple(e) for e in cfg["topology"]["retail_links"]]
    assert links == [(3, 8), (2, 7), (2, 0)]
    assert (_topology(cfg).tables["rl_user"] == 0).all()
    for i in range(cfg["n_env"]):
        g = _npg(cfg["base_seed"] + i)
        exp = [[0, g.poisson(lam=3), g.geometric(p=0.2)] for _ in range(cfg["ep_len"])]
        assert np.array_equal(fx["D"][i], np.array(exp, np.float64)), i
    L = _topology(cfg).tables["L"]
    assert sorted(L.tolist()) == [0, 1, 2, 3] and not _topology(cfg).tables["is_factory"].any()


def test_minimal_shape_and_integers_market():
    fx, cfg = load_golden("net_graph_minimal")
    tp = _topology(cfg)
    assert (len(tp.main_nodes), len(tp.reorder_links), len(tp.retail_links), tp.obs_dim) == (1, 1, 1, 2)
    assert sum(tp.lead_times.values()) == 0 and tp.tables["rl_dist"][0] == 3
    for i in range(cfg["n_env"]):
        g = _npg(cfg["base_seed"] + i)
        exp = [g.integers(low=0, high=9) for _ in range(cfg["ep_len"])]
        assert np.array_equal(fx["D"][i, :, 0], np.array(exp, np.float64)), i


# ---------------------------------------------------------------- sizes against the kernel's limits
def _sizes(g, T):
    from invsim.topology import compile_graph
    tp = compile_graph(g, T)
    return len(tp.main_nodes), len(tp.reorder_links), len(tp.retail_links), sum(tp.lead_times.values())


def test_wide_and_too_large_straddle_the_lds_bound():
    J, E, RL, sumL = _sizes(net_graphs.wide(), 8)
    assert (J, E, RL) == (20, 44, 6) and 80 <= sumL <= 100
    assert 64 * 1024 < net_graphs.lds_bytes(J, E, RL, sumL) <= 160 * 1024
    J, E, RL, sumL = _sizes(net_graphs.too_large(), 8)
    assert (J, E, RL) == (24, 60, 6) and J <= 64 and E <= 256 and RL <= 64
    assert net_graphs.lds_bytes(J, E, RL, sumL) > 160 * 1024
    for name in ("mixed", "chain", "wide"):               # the oracle's padded adjacency (ORC_NET_MAXADJ)
        g = GRAPHS[name]()
        assert max(max(d for _, d in g.in_degree()), max(d for _, d in g.out_degree())) <= 16
