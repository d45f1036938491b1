"""numpy restatement of the INVSIM_POLICY_NET_LEVELS rule (include/invsim.h,
"Per-env order-up-to levels on a supply network") and its closed loop on the C
oracle (TEST INFRASTRUCTURE, never shipped).

For env n and reorder link k with purchaser p = pur[k], from the f64 state at
the start of the period:

    pos = X[p]; pos = pos + Y[k'] for every link k' into p, ascending;
    pos = pos - U[r] for every market r of p, ascending
    x = levels[n][k] - pos;  with reorder: x = 0 unless pos < reorder[n][k]
    x = x > 0 ? x : 0;  x = x > high[k] ? high[k] : x;  action = float32(x)

`ClosedLoop` drives a pyoracle.OracleNet: the state is I0, 0, 0 after reset()
and the oracle's own X, U, Y (step(..., info=True)) afterwards; the metric sums
are kept in the kernels' order (oracle/agents.py run_net's).  The tables come
from oracle.topo["tables"].
"""
import numpy as np


def action_high(graph):
    """The env's action bound per reorder link (network_management.py:193-195,
    :270-275): 2 * (max I0 over the main nodes + 5 * max C over the factories),
    as float32; the maxima default to 100 where there is no such node."""
    nd = graph.nodes
    main = [j for j in nd if "C" in nd[j] or ("I0" in nd[j] and list(graph.predecessors(j)))]
    i0 = max((nd[j].get("I0", 0) for j in main), default=100)
    cap = max((graph.nodes[j]["C"] for j in graph.nodes() if "C" in graph.nodes[j]), default=100)
    n_reorder = sum(1 for e in graph.edges() if "L" in graph.edges[e])
    return (np.ones(n_reorder, np.float32) * (i0 + cap * 5) * 2).astype(np.float32)


def positions(X, U, Y, pur, rl_node):
    """[n, J]: every node's inventory position, summed in the contract's order"""
    pos = np.array(X, np.float64, copy=True)
    for j in range(pos.shape[1]):
        for k in range(len(pur)):
            if pur[k] == j:
                pos[:, j] = pos[:, j] + Y[:, k]
        for r in range(len(rl_node)):
            if rl_node[r] == j:
                pos[:, j] = pos[:, j] - U[:, r]
    return pos


def actions(X, U, Y, levels, reorder, high, pur, rl_node):
    """float32 [n, E]"""
    pos = positions(X, U, Y, pur, rl_node)
    E = len(pur)
    out = np.zeros((pos.shape[0], E), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(E):
            p = pos[:, pur[k]]
            x = levels[:, k] - p
            if reorder is not None:
                x = np.where(p < reorder[:, k], x, 0.0)
            x = np.where(x > 0, x, 0.0)
            hi = np.float64(high[k])
            x = np.where(x > hi, hi, x)
            out[:, k] = x.astype(np.float32)
    return out


class ClosedLoop:
    """The oracle's envs under the rule.  run(K, autoreset) returns the K launch
    rows the device writes: a NEXT_STEP reset row has the reset observation,
    reward 0, truncated False, an all-zero (unwritten) action row and adds
    nothing to `metrics`."""

    def __init__(self, orc, levels, reorder=None, high=None):
        t = orc.topo["tables"]
        self.orc = orc
        self.J, self.E, self.RL = orc.topo["J"], orc.topo["E"], orc.topo["RL"]
        self.pur = np.asarray(t["pur"])[:self.E]
        self.rl_node = np.asarray(t["rl_node"])[:self.RL]
        self.I0 = np.asarray(t["I0"], np.float64)[:self.J]
        self.T = int(orc.cfg.num_periods)
        n = orc.n
        self.levels = np.broadcast_to(np.asarray(levels, np.float64), (n, self.E))
        self.reorder = None if reorder is None else np.broadcast_to(np.asarray(reorder, np.float64), (n, self.E))
        self.high = np.asarray(high, np.float32)
        self.metrics = np.zeros((n, 5 + self.J))
        self.xs = []                 # X[t+1] of every applied step
        self.reset()

    def reset(self):
        n = self.orc.n
        self.obs0 = self.orc.reset()
        self.X = np.tile(self.I0, (n, 1))
        self.U = np.zeros((n, self.RL))
        self.Y = np.zeros((n, self.E))
        self.t = 0
        return self.obs0

    def run(self, K, autoreset=False):
        n = self.orc.n
        out = dict(actions=np.zeros((K, n, self.E), np.float32), obs=np.zeros((K, n, self.orc.obs_dim), np.float32),
                   reward=np.zeros((K, n)), truncated=np.zeros((K, n), bool), applied=np.zeros(K, bool))
        for k in range(K):
            if self.t >= self.T:
                assert autoreset, "stepping past the horizon"
                out["obs"][k] = self.reset()
                continue
            a = actions(self.X, self.U, self.Y, self.levels, self.reorder, self.high, self.pur, self.rl_node)
            obs, r, tr, info = self.orc.step(a, info=True)
            self.X, self.U, self.Y = info["X"], info["U"], info["Y"]
            m = self.metrics
            m[:, 0] += r
            m[:, 1] += 1
            for q in range(self.RL):
                m[:, 2] += info["D"][:, q]
                m[:, 3] += info["S"][:, q]
                m[:, 4] += info["U"][:, q]
            m[:, 5:] += info["X"]
            self.xs.append(info["X"].copy())
            out["actions"][k], out["obs"][k], out["reward"][k], out["truncated"][k] = a, obs, r, tr
            out["applied"][k] = True
            self.t += 1
        out["metrics"] = self.metrics.copy()
        return out


def shares(acts, high):
    """(share strictly inside (0, high), share equal to 0) of recorded actions [..., E]"""
    a = np.asarray(acts, np.float64)
    return float(((a > 0) & (a < np.asarray(high, np.float64))).mean()), float((a == 0).mean())
