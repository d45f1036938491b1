"""The 2-role InvMgmt rollout (im_roll3_kernel) as back-to-back launches over
sub-ranges of the env groups (INVSIM_IM_ROLL_SUB), against the C oracle stepping
the same seeds (inventory_management.py:224-352 per env).

test_gpu_roll_sub.py compares the sub-launches with one launch of the same
kernel, so a fault both launch shapes share (the partial last group's e0 / el,
the k * N + e output index, the action prefetch at (k + 1) * N + el) passes
there.  Here every output row, the final state, every env's PCG64 state and the
episode sink's running returns and per-group partials are the oracle's.

Knob combinations pinned (libinvsim reads the knobs when a handle is made):

  class      n       ROLL3O_MAX_N  ROLL_SUB  launches (64-env groups)
  Backlog    3141    0             1024      16, 16, 16, 2 (one full + the group of 5)
  LostSales  3141    0             100       50 of one group (100 rounds down to 64)
  LostSales  3141    0             1024      16, 16, 16, 2
  Backlog    65605   unset         unset     1024, 2: the shipped default past 65 536 envs
  BaseStock policy (POL = true), Backlog sf 1.37 and LostSales sf 1.0:
             3141    0             1024      16, 16, 16, 2
"""
import math

import numpy as np
import pytest
import torch

import agents
from test_gpu_parity import _assert_reward, _eq_bits, _im_random_actions

pytestmark = pytest.mark.gpu

T = 30                       # periods of the default config
KS = (33, 28, 1, 1, 1, 5)    # rollouts (K > 1) and single steps, in call order:
#   K = 33: periods 0..29, the NEXT_STEP reset row at row 30 inside the launch, periods 0, 1
#           (33 is no multiple of the demand chunk of 4)
#   K = 28: periods 2..29, ends on the truncation
#   three steps: the lock-step reset step, periods 0 and 1
#   K = 5:  periods 2..6


def _make(monkeypatch, cls_name, n, gpu, max_n, sub, **kw):
    import invsim
    for var, v in (("INVSIM_IM_ROLL3O_MAX_N", max_n), ("INVSIM_IM_ROLL_SUB", sub)):
        if v is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, str(v))
    env = getattr(invsim, cls_name)(n, device=gpu, **kw)
    monkeypatch.delenv("INVSIM_IM_ROLL3O_MAX_N", raising=False)
    monkeypatch.delenv("INVSIM_IM_ROLL_SUB", raising=False)
    return env


def _near(got, terms, where):
    """got, an f64 sum of `terms` in the kernel's order, against their exact sum
    (math.fsum): any order of m terms errs by at most (m - 1) 2**-53 sum|x|.
    The largest m here is a group's reward sum, 64 envs x 67 rewards = 4288
    terms: under 4.8e-13 sum|x|, so 1e-12 sum|x| holds for every order."""
    terms = np.asarray(terms, np.float64).ravel()
    exp, tol = math.fsum(terms), 1e-12 * math.fsum(np.abs(terms))
    assert abs(float(got) - exp) <= tol, f"{where}: {float(got)!r} != {exp!r} (tol {tol:.3g})"


@pytest.mark.parametrize("cls_name,n,max_n,sub", [
    ("InvManagementBacklogEnv", 3141, 0, 1024),
    ("InvManagementLostSalesEnv", 3141, 0, 100),
    ("InvManagementLostSalesEnv", 3141, 0, 1024),
    ("InvManagementBacklogEnv", 65536 + 64 + 5, None, None),
])
def test_roll_sub_open_loop_vs_oracle(gpu, oracle, monkeypatch, cls_name, n, max_n, sub):
    from invsim.distributed import EpisodeStats
    backlog = cls_name.endswith("BacklogEnv")
    seed = 300
    oracle.set_threads(8)
    try:
        env = _make(monkeypatch, cls_name, n, gpu, max_n, sub)
        orc = oracle.OracleInvMgmt(n, backlog=backlog)
        orc.seed(range(seed, seed + n))
        e_obs = orc.reset()
        obs, _ = env.reset(seed=seed)
        assert _eq_bits(obs.cpu().numpy(), e_obs)
        st = None
        if backlog:
            st = EpisodeStats(n, gpu)
            st.attach(env)
        rng = np.random.default_rng(11)
        calls = sum(KS)
        acts = np.stack([_im_random_actions(rng, n, 3, [100, 200, 230]) for _ in range(calls)])
        dev_acts = torch.from_numpy(acts).to(gpu)
        ret = np.zeros(n)                 # the sink's arithmetic on the oracle's rewards
        fin, rews = [], []
        t, k, info = 0, 0, None
        for K in KS:
            if K > 1:
                o, r, te, tr = env.rollout(dev_acts[k:k + K])
            else:
                o, r, te, tr, _ = env.step(dev_acts[k])
                o, r, te, tr = o[None], r[None], te[None], tr[None]
            o, r, te, tr = o.cpu().numpy(), r.cpu().numpy(), te.cpu().numpy(), tr.cpu().numpy()
            assert not te.any(), f"terminated, call at row {k}"
            for j in range(K):
                where = f"row {k} (row {j} of K={K})"
                if t >= T:                                   # NEXT_STEP autoreset step
                    assert _eq_bits(o[j], orc.reset()), where
                    assert (r[j] == 0).all() and not tr[j].any(), where
                    ret = ret + 0.0
                    t = 0
                else:
                    res = orc.step(acts[k], info=(k == calls - 1))
                    assert _eq_bits(o[j], res[0]), f"obs {where}"
                    _assert_reward(r[j], res[1], where)
                    assert np.array_equal(tr[j], res[2]), f"truncated {where}"
                    ret = ret + res[1]
                    rews.append(res[1])
                    t += 1
                    if res[2].all():
                        fin.append(ret)
                        ret = np.zeros(n)
                    if len(res) > 3:
                        info = res[3]
                k += 1
        fields = env.state_fields()
        assert np.array_equal(fields["I"].cpu().numpy().T, info["ending_inventory"])
        # every env's PCG64 (state hi, state lo, inc hi, inc lo): the demand wave's
        # state store of each sub-launch
        got_rng = fields["rng"].cpu().numpy().view(np.uint64).T
        exp_rng = orc.rng_state()
        bad = np.flatnonzero((got_rng != exp_rng).any(axis=1))
        assert bad.size == 0, f"PCG64 state of {bad.size} envs, first {bad[:4].tolist()}"
        if st is None:
            return
        torch.cuda.synchronize()
        got = st.ret.cpu().numpy()
        assert np.array_equal(got.view(np.int64), ret.view(np.int64)), \
            f"running returns: {np.flatnonzero(got != ret)[:4].tolist()}"
        part = st.part.cpu().numpy()
        fin, rews = np.stack(fin), np.stack(rews)            # [2, n] episode returns, [67, n] rewards
        assert fin.shape == (2, n) and rews.shape == (calls - 2, n)
        groups = (n + 63) // 64
        assert part.shape == (groups, 4)
        size = np.minimum(64, n - 64 * np.arange(groups))
        assert np.array_equal(part[:, 2], 2.0 * size), "finished episodes per group"
        for g in range(groups):
            e = slice(64 * g, min(64 * g + 64, n))
            _near(part[g, 0], fin[:, e], f"group {g} sum of episode returns")
            _near(part[g, 1], fin[:, e] * fin[:, e], f"group {g} sum of squared episode returns")
            _near(part[g, 3], rews[:, e], f"group {g} sum of rewards")
    finally:
        oracle.set_threads(1)


@pytest.mark.parametrize("cls_name,sf", [("InvManagementBacklogEnv", 1.37), ("InvManagementLostSalesEnv", 1.0)])
def test_roll_sub_policy_vs_oracle(gpu, oracle, monkeypatch, cls_name, sf):
    """the in-kernel BaseStock agent (POL = true) on the sub-launched 2-role
    kernel, as test_policies.test_base_stock_vs_oracle does for the 3-role one;
    then K = 13 + 17 into one metrics tensor: its read-modify-write across
    sub-launches and calls"""
    import invsim
    n, mu = 3141, 20
    oracle.set_threads(8)
    try:
        env = _make(monkeypatch, cls_name, n, gpu, 0, 1024, autoreset_mode="disabled")
        orc = oracle.OracleInvMgmt(n, backlog=cls_name.endswith("BacklogEnv"))
        orc.seed(range(500, 500 + n))
        o0 = orc.reset()
        env.reset(seed=500)
        M = invsim.policies.metrics_dim(env)
        met = torch.zeros((n, M), dtype=torch.float64, device=gpu)
        out = env.rollout_policy(invsim.BaseStockAgent(sf), 30, obs=True, actions=True, metrics=met)
        e_act, e_rew, e_obs, e_sum = agents.run_invmgmt(orc, o0, 30, env.lead_time, mu, sf, env.supply_capacity)
        assert np.array_equal(out["actions"].cpu().numpy(), e_act)
        assert np.array_equal(out["obs"].cpu().numpy(), e_obs)
        assert np.array_equal(out["reward"].cpu().numpy().view(np.uint64), e_rew.view(np.uint64))
        assert np.array_equal(met.cpu().numpy().view(np.uint64), e_sum.view(np.uint64))
        assert bool(out["truncated"][-1].all()) and not bool(out["truncated"][:-1].any())
        assert not bool(out["terminated"].any())
        env2 = _make(monkeypatch, cls_name, n, gpu, 0, 1024, autoreset_mode="disabled")
        env2.reset(seed=500)
        met2 = torch.zeros((n, M), dtype=torch.float64, device=gpu)
        a = env2.rollout_policy(invsim.BaseStockAgent(sf), 13, metrics=met2)
        b = env2.rollout_policy(invsim.BaseStockAgent(sf), 17, metrics=met2)
        assert torch.equal(met2.view(torch.int64), met.view(torch.int64)), "metrics of K = 13 + 17 against K = 30"
        rew2 = torch.cat([a["reward"], b["reward"]]).cpu().numpy()
        assert np.array_equal(rew2.view(np.uint64), e_rew.view(np.uint64))
    finally:
        oracle.set_threads(1)
