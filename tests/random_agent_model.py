"""The numpy model of the in-kernel RandomAgent (include/invsim.h "RandomAgent")
and the evaluate_agent sums for a given per-step action array (TEST
INFRASTRUCTURE, never shipped).

The reference's RandomAgent is ``env.action_space.sample()`` on an unseeded
space, so there is no reference trajectory: the contract is numpy's own
``Generator``, called here directly.

* env with global index g draws from ``Generator(PCG64(SeedSequence(2**64 + seed + g)))``
* one launch step consumes ``action_dim`` doubles ``Generator.random()`` in action order
* float32 spaces:  ``(high.astype(f64) * u).astype(f32)``
  int64 spaces:    ``floor((high + 1).astype(f64) * u).astype(int64)``
  which is ``Generator.uniform(0, high)`` / ``uniform(0, high + 1)`` bit for bit
  (test_random_agent.py checks that).

The sums are written the way oracle/agents.py run_invmgmt / run_net /
run_newsvendor keep them for their agents, with the action of every step given.
"""
import numpy as np

ACTION_SEED_BASE = 2**64


def generator(seed, g):
    return np.random.Generator(np.random.PCG64(np.random.SeedSequence(ACTION_SEED_BASE + int(seed) + int(g))))


def scale(u, high, dtype):
    """Uniform doubles u [..., A] -> actions of an action space with bounds [0, high]."""
    high = np.asarray(high)
    if np.issubdtype(np.dtype(dtype), np.integer):
        return np.floor((high.astype(np.int64) + 1).astype(np.float64) * u).astype(np.int64)
    return (high.astype(np.float32).astype(np.float64) * u).astype(np.float32)


def _state_rows(gens):
    """[4, n] uint64: state hi / state lo / inc hi / inc lo of each generator."""
    out = np.zeros((4, len(gens)), np.uint64)
    m = (1 << 64) - 1
    for i, g in enumerate(gens):
        st = g.bit_generator.state["state"]
        out[:, i] = [st["state"] >> 64, st["state"] & m, st["inc"] >> 64, st["inc"] & m]
    return out


def expected_actions(seed, first, n, K, high, dtype, skip=0):
    """Actions [K, n, A] of envs with global indices first .. first + n - 1 over
    launch steps skip .. skip + K - 1 of their action streams, and the
    generators' [4, n] state rows after them."""
    A = len(high)
    gens = [generator(seed, first + i) for i in range(n)]
    u = np.empty((K, n, A), np.float64)
    for i, g in enumerate(gens):
        if skip:
            g.random(skip * A)
        u[:, i, :] = g.random(K * A).reshape(K, A)
    return scale(u, high, dtype), _state_rows(gens)


def sums_invmgmt(orc, acts):
    """evaluate_agent's sums [N, 6] of an OracleInvMgmt stepped with acts [K, N, M1]
    (agents.run_invmgmt's bookkeeping); also the rewards and observations."""
    N = acts.shape[1]
    sums = np.zeros((N, 6))
    rews, obss = [], []
    for a in acts:
        obs, r, tr, info = orc.step(a, info=True)
        sums[:, 0] += r
        sums[:, 1] += 1
        sums[:, 2] += info["demand"]
        sums[:, 3] += info["sales"][:, 0]
        sums[:, 4] += info["unfulfilled"][:, 0]
        sums[:, 5] += np.maximum(0, info["ending_inventory"]).sum(axis=1)
        rews.append(r), obss.append(obs)
    return sums, np.stack(rews), np.stack(obss)


def sums_newsvendor(orc, acts):
    """agents.run_newsvendor's sums [N, 2] for acts [K, N, 1]."""
    N = acts.shape[1]
    sums = np.zeros((N, 2))
    rews, obss = [], []
    for a in acts:
        obs, r, tr, _ = orc.step(a)
        sums[:, 0] += r
        sums[:, 1] += 1
        rews.append(r), obss.append(obs)
    return sums, np.stack(rews), np.stack(obss)


def sums_net(orc, acts):
    """agents.run_net's sums [N, 5 + J] for acts [K, N, E]."""
    N = acts.shape[1]
    J = orc.topo["J"]
    sums = np.zeros((N, 5 + J))
    rews, obss = [], []
    for a in acts:
        obs, r, tr, info = orc.step(np.ascontiguousarray(a, np.float32), info=True)
        sums[:, 0] += r
        sums[:, 1] += 1
        for q in range(info["D"].shape[1]):
            sums[:, 2] += info["D"][:, q]
            sums[:, 3] += info["S"][:, q]
            sums[:, 4] += info["U"][:, q]
        sums[:, 5:] += info["X"]
        rews.append(r), obss.append(obs)
    return sums, np.stack(rews), np.stack(obss)
