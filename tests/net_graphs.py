"""Supply networks outside the reference's two built-in graphs (test helper,
imported by tests/golden/gen_goldens.py, test_net_graphs_model.py and
test_gpu_net_graphs.py).  All of them run on the generic table-walking kernel.

Every builder returns a fresh ``networkx.DiGraph`` and takes ``sampler``: a
function from a numpy Generator method name to the edge's
``demand_dist_func``.  The golden generator passes a lambda over the reference
env's own ``np_random``; the oracle and the device take the method name
(``by_name``, the default).

Nodes and edges are inserted in deliberately non-sorted order.  The reference
keeps main nodes and reorder links sorted, but draws market demand in
``graph.edges()`` order (node insertion order, then each node's adjacency
order) and sums revenue, cost and arrivals in adjacency order
(network_management.py:158, :516-523, :582-609), so both orders are visible in
the RNG stream and in the f64 bits.  The reference, like the device env, works
on ``graph.copy()``: a copy keeps node and successor order and rebuilds every
predecessor list in ``graph.edges()`` order.

mixed      5 main nodes, 10 reorder links, 3 market links (GRAPHS["mixed"])
minimal    raw -> retailer -> market, L = 0: J = E = RL = 1, obs_dim = 2
chain      raw -> four distributors in series -> markets, no factory
wide       20 main nodes in layers, 44 reorder links, 6 market links: the
           kernel's dynamic LDS request is above 64 KB and below 160 KB
series     raw -> n distributors in series -> market, every link with lead
           time L (the create-time limits, tests/limit_cases.py)
too_large  24 main nodes, 60 reorder links: inside the J / E / RL limits, LDS
           need above 160 KB (creation must fail)
"""
import networkx as nx

USER_D = [2.5, 3.5, 0, -4, 7.49, 7.51, 1.5, 0.5, 6.5, 3, 4.499999, 9.5]


def by_name(name):
    return name


def user_d(T):
    """USER_D cycled to T periods: .5 ties both ways, a negative entry, a zero."""
    return [USER_D[t % len(USER_D)] for t in range(T)]


def expected_user_demand(T):
    """max(0, int(round(x))) of user_d(T), round half to even (network_management.py:540)."""
    return [max(0, int(round(x))) for x in user_d(T)]


def mixed(sampler=by_name, T=12):
    """Factory 7 (v = 0.8) feeds factory 4 (v = 0.55), distributor 6 and retailer
    5; retailer 5 supplies retailer 3 over an L = 0 link and sells to market 0;
    retailer 3 sells to markets 8 (user_D replay) and 0 and is otherwise only
    reached by a link with L = 20 > T.  Node 7 has three successors and node 5
    three predecessors, inserted out of sorted order."""
    g = nx.DiGraph()
    g.add_nodes_from([5], I0=35, h=0.033)
    g.add_nodes_from([0, 9])
    g.add_nodes_from([3], I0=3, h=0.041)
    g.add_nodes_from([7], I0=150, C=25, o=0.013, v=0.8, h=0.011)
    g.add_nodes_from([8])
    g.add_nodes_from([4], I0=40, C=45, o=0.021, v=0.55, h=0.009)
    g.add_nodes_from([2])
    g.add_nodes_from([6], I0=45, h=0.017)
    g.add_edges_from([
        (7, 6, {"L": 2, "p": 1.13, "g": 0.007}),
        (3, 8, {"p": 2.3, "b": 0.13, "user_D": user_d(T)}),
        (6, 5, {"L": 2, "p": 1.7, "g": 0.011}),
        (9, 7, {"L": 0, "p": 0.33, "g": 0.0}),
        (5, 3, {"L": 0, "p": 2.1, "g": 0.003}),
        (7, 4, {"L": 1, "p": 0.9, "g": 0.006}),
        (5, 0, {"p": 2.9, "b": 0.21, "demand_dist_func": sampler("binomial"), "dist_param": {"n": 30, "p": 0.3}}),
        (7, 5, {"L": 2, "p": 1.9, "g": 0.013}),
        (2, 4, {"L": 2, "p": 0.13, "g": 0.002}),
        (3, 0, {"p": 2.7, "b": 0.17, "demand_dist_func": sampler("poisson"), "dist_param": {"lam": 4.5}}),
        (6, 3, {"L": 20, "p": 1.6, "g": 0.004}),
        (4, 6, {"L": 3, "p": 1.3, "g": 0.005}),
        (4, 5, {"L": 1, "p": 1.45, "g": 0.012})])
    return g


def minimal(sampler=by_name, T=8):
    g = nx.DiGraph()
    g.add_nodes_from([2], I0=20, h=0.05)
    g.add_nodes_from([0, 1])
    g.add_edges_from([
        (2, 0, {"p": 3.1, "b": 0.4, "demand_dist_func": sampler("integers"), "dist_param": {"low": 0, "high": 9}}),
        (1, 2, {"L": 0, "p": 1.1, "g": 0.0})])
    return g


def chain(sampler=by_name, T=10):
    """10 -> 4 -> 1 -> 3 -> 2 with lead times 1, 0, 3, 2.  Market links: (2, 0)
    geometric; (2, 7) carries a user_D table with sample_path=True, which must
    be ignored in favour of its Poisson sampler; (3, 8) has no demand source:
    zero demand and no draw."""
    g = nx.DiGraph()
    g.add_nodes_from([3], I0=25, h=0.023)
    g.add_nodes_from([7, 10])
    g.add_nodes_from([1], I0=30, h=0.019)
    g.add_nodes_from([2], I0=12, h=0.037)
    g.add_nodes_from([0, 8])
    g.add_nodes_from([4], I0=60, h=0.007)
    g.add_edges_from([
        (2, 7, {"p": 2.6, "b": 0.23, "user_D": [5, 6, 7, 8, 9], "sample_path": True,
                "demand_dist_func": sampler("poisson"), "dist_param": {"lam": 3}}),
        (3, 2, {"L": 2, "p": 1.9, "g": 0.009}),
        (3, 8, {"p": 2.2, "b": 0.31}),
        (4, 1, {"L": 0, "p": 0.7, "g": 0.001}),
        (2, 0, {"p": 3.3, "b": 0.19, "demand_dist_func": sampler("geometric"), "dist_param": {"p": 0.2}}),
        (10, 4, {"L": 1, "p": 0.33, "g": 0.002}),
        (1, 3, {"L": 3, "p": 1.3, "g": 0.006})])
    return g


_YIELDS = (1.0, 0.8, 0.55, 0.9)
_CAPS = (30, 45, 25, 60)
_MARKETS = (("poisson", {"lam": 6.5}), ("binomial", {"n": 20, "p": 0.35}), ("integers", {"low": 1, "high": 12}),
            ("geometric", {"p": 0.25}), ("user_D", None), ("poisson", {"lam": 2.2}))


def _layered(sampler, T, widths, fanin, leads, n_lateral, n_feed, n_market_nodes=3):
    """raw materials -> widths[0] factories -> widths[1] ... -> widths[-1]
    retailers -> markets.  Node i of layer k + 1 buys from `fanin[k]` nodes of
    layer k (i, i + 1, ... modulo the layer's width); `n_lateral` retailers also
    supply their neighbour over an L = 0 link, `n_feed` factories feed the next
    factory.  Six market links over the retailers (two retailers serve two
    markets), one of them a user_D replay.  Node ids, node order and edge order
    are scrambled by fixed permutations."""
    n_main = sum(widths)
    n_nodes = n_market_nodes + 2 + n_main
    assert n_nodes <= 37
    nid = lambda i: (11 * i + 5) % 37                  # noqa: E731  (11 is a unit modulo 37)
    markets = [nid(i) for i in range(n_market_nodes)]
    raws = [nid(n_market_nodes), nid(n_market_nodes + 1)]
    layers, i = [], n_market_nodes + 2
    for w in widths:
        layers.append([nid(i + q) for q in range(w)])
        i += w
    attrs = {j: {} for j in markets + raws}
    for q, j in enumerate(layers[0]):
        attrs[j] = dict(I0=120 + 15 * q, C=_CAPS[q % 4], o=0.011 + 0.003 * q, v=_YIELDS[q % 4], h=0.007 + 0.001 * q)
    for k, layer in enumerate(layers[1:], 1):
        for q, j in enumerate(layer):
            attrs[j] = dict(I0=(45 if k < len(layers) - 1 else 14) + 4 * q, h=0.013 + 0.004 * k + 0.001 * q)
    edges = []

    def link(s, p, layer):
        q = len(edges)
        edges.append((s, p, {"L": leads[q % len(leads)], "p": round(0.37 + 0.41 * layer + 0.013 * (q % 7), 3),
                             "g": round(0.001 * (1 + q % 5), 3)}))

    for q, j in enumerate(layers[0]):
        link(raws[q % 2], j, 0)
    for q in range(n_feed):
        link(layers[0][q], layers[0][q + 1], 0)
    for k in range(len(layers) - 1):
        lo, hi = layers[k], layers[k + 1]
        for q, j in enumerate(hi):
            for f in range(fanin[k]):
                link(lo[(q + f) % len(lo)], j, k + 1)
    retailers = layers[-1]
    for q in range(n_lateral):
        s, p = retailers[q], retailers[q + 1]
        edges.append((s, p, {"L": 0, "p": round(2.05 + 0.07 * q, 3), "g": 0.002}))
    for q, (fn, dp) in enumerate(_MARKETS):
        e = {"p": round(2.9 + 0.23 * q, 3), "b": round(0.11 + 0.04 * q, 3)}
        if fn == "user_D":
            e["user_D"] = user_d(T)
        else:
            e["demand_dist_func"], e["dist_param"] = sampler(fn), dict(dp)
        edges.append((retailers[q % len(retailers)], markets[q % len(markets)], e))
    g = nx.DiGraph()
    for j in sorted(attrs, key=lambda j: (5 * j) % 37):
        g.add_nodes_from([j], **attrs[j])
    for q in sorted(range(len(edges)), key=lambda q: (7 * q) % 71):
        g.add_edges_from([edges[q]])
    return g


def wide(sampler=by_name, T=8):
    """J = 20, E = 44, RL = 6: 4 factories (yields 1.0, 0.8, 0.55, 0.9), two
    layers of 6 distributors, 4 retailers."""
    return _layered(sampler, T, widths=(4, 6, 6, 4), fanin=(2, 2, 3), leads=(2, 1, 3, 0, 4, 2, 1, 3, 2),
                    n_lateral=2, n_feed=2)


def too_large(sampler=by_name, T=8):
    """J = 24, E = 60, RL = 6 (every size inside the create-time limits 64 /
    256 / 64): the LDS scratch plus the obs tile need more than 160 KB."""
    return _layered(sampler, T, widths=(4, 8, 8, 4), fanin=(2, 2, 5), leads=(2, 1, 3, 2, 3, 2, 1, 3, 1),
                    n_lateral=2, n_feed=2)


def series(n_main, L=1):
    """raw -> n_main distributors in series -> market"""
    g = nx.DiGraph()
    g.add_nodes_from([0, 1])
    for j in range(2, 2 + n_main):
        g.add_nodes_from([j], I0=5, h=0.01)
        g.add_edge(j - 1, j, L=L, p=1.1, g=0.001)
    g.add_edge(1 + n_main, 0, p=2.3, b=0.1, demand_dist_func="poisson", dist_param={"lam": 2})
    return g


GRAPHS = {"mixed": mixed, "minimal": minimal, "chain": chain, "wide": wide, "too_large": too_large}

# name -> (builder, num_periods, backlog, alpha) of the committed tests/golden/net_graph_<name>.npz
GOLDEN_CASES = {
    "mixed_backlog": ("mixed", 12, True, 0.93),
    "mixed_lost": ("mixed", 12, False, 0.93),
    "mixed_2ep": ("mixed", 12, True, 0.93),
    "minimal": ("minimal", 8, True, 1.0),
    "chain": ("chain", 10, True, 0.97),
    "wide": ("wide", 8, True, 0.95),
}
NET_GRAPH_GOLDENS = ["net_graph_" + k for k in GOLDEN_CASES]


def lds_bytes(J, E, RL, sumL):
    """The generic kernel's dynamic LDS request (net_lds_bytes, netinvmgmt.hip):
    three f64 rows of 64 lanes per node, reorder link and market link, plus the
    f32 obs tile of 64 envs rounded up to 16 B."""
    tile = 64 * (RL + J + sumL) * 4
    return 3 * (J + E + RL) * 512 + (tile + 15) // 16 * 16
