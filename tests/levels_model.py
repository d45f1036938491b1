"""numpy restatement of the INVSIM_POLICY_LEVELS action rule (include/invsim.h,
"Per-env base-stock levels"), from an observation row and the env's period.

TEST INFRASTRUCTURE: the checker of the LEVELS kernels where oracle/agents.py
(BaseStockAgent with an array safety factor) cannot be: reorder points and
non-finite levels.  The observation holds I[t] and the last min(t, lt_max)
requested orders, oldest first, which is every order the rule needs because
L_i <= lt_max.
"""
import numpy as np


def position(obs, t, L):
    """Inventory position [N, M1]: I[t] + sum(action_log[max(0, t - L_i) : t, i]),
    int64 with wraparound.  obs [N, M1 * (lt_max + 1)] int64; t the period, a
    scalar or [N]; L [M1] lead times."""
    obs = np.asarray(obs, np.int64)
    L = np.asarray(L, np.int64)
    N, M1 = obs.shape[0], len(L)
    D = obs.shape[1] // M1 - 1
    t = np.broadcast_to(np.asarray(t, np.int64), (N,))
    pos = obs[:, :M1].copy()
    win = obs[:, M1:].reshape(N, D, M1)          # row r: period t - n + r, n = min(t, D) rows filled
    n = np.minimum(t, D)
    for i in range(M1):
        take = np.minimum(L[i], t)               # the last `take` of the n filled rows
        for a in range(1, int(L[i]) + 1):
            m = take >= a
            r = np.where(m, n - a, 0)
            with np.errstate(over="ignore"):
                pos[:, i] += np.where(m, win[np.arange(N), r, i], 0)
    return pos


def action(obs, t, L, c, levels, reorder=None):
    """The order of every env [N, M1] int64 at period t; levels / reorder f64
    [N, M1] (or broadcastable to it)."""
    pos = position(obs, t, L).astype(np.float64)
    lv = np.broadcast_to(np.asarray(levels, np.float64), pos.shape)
    cf = np.asarray(c, np.int64).astype(np.float64)
    with np.errstate(invalid="ignore"):
        x = lv - pos
        if reorder is not None:
            ro = np.broadcast_to(np.asarray(reorder, np.float64), pos.shape)
            x = np.where(pos < ro, x, 0.0)       # strict <; a NaN reorder point never orders
        x = np.where(x > 0, x, 0.0)              # a NaN level orders 0
        x = np.where(x > cf, cf, x)
    return x.astype(np.int64)
