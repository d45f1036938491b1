"""The cohort oracle of tests/staggered.py against N single-env oracles (no
GPU): every env is an oracle instance of its own (n = 1) that tracks its own
period and applies the autoreset rule itself, driven through the same masks
and actions.  Rows, generator states, periods and params must be identical.

The second half asserts, from the period table alone, the coverage conditions
the GPU cases of test_gpu_staggered.py rely on (they run these same scripts):

 (a) some row has a 64-env group with both resetting and stepping envs;
 (b) some row has a group that resets as a whole while another group has
     stepping envs;
 (c) every cohort crosses its horizon at least once, one of them twice;
 (d) env N - 1 is under a mask in schedule 'a' and under none in 'b';
 (e) no cohort is empty.

"Resets" is what staggered.coverage defines per autoreset mode.  DISABLED
InvMgmt / Net scripts reset by mask before a cohort overruns, so there (a) and
(b) are asked of the horizon-fault schedule (staggered.fault_script), where the refused
lanes sit next to stepping ones, and of the main script only that some group
holds envs at different periods.
"""
import numpy as np
import pytest

import agents
import staggered
from staggered import N

IM7 = dict(periods=7)
IM12 = dict(periods=12, I0=(30, 40, 50, 60, 70, 80, 90, 100), r=(9, 8, 7, 6, 5, 4, 3, 2, 1),
            k=(0.3, 0.2, 0.1, 0.1, 0.05, 0.05, 0.05, 0.02, 0.01), h=(0.2, 0.15, 0.12, 0.1, 0.08, 0.06, 0.04, 0.02),
            c=(60, 70, 80, 90, 100, 110, 120, 130), L=(0, 1, 2, 3, 0, 4, 2, 6), p=11, alpha=0.9,
            dist_param={"mu": 35})
MODES = ("next_step", "same_step", "disabled")


class Singles:
    """N oracles of one env each; the autoreset rules restated per env"""

    def __init__(self, pyoracle, family, n, seed, mode, **kw):
        cls = {"im": pyoracle.OracleInvMgmt, "nv": pyoracle.OracleNewsvendor, "net": pyoracle.OracleNet}[family]
        self.orcs = [cls(1, **kw) for _ in range(n)]
        for e, o in enumerate(self.orcs):
            o.seed([seed + e])
        self.family, self.n, self.mode = family, n, mode
        self.t = np.zeros(n, np.int32)
        self.obs = [None] * n
        self.log = [[] for _ in range(n)]

    def _reset(self, e):
        self.obs[e] = self.orcs[e].reset()
        self.t[e], self.log[e] = 0, []
        return self.obs[e][0]

    def reset(self, mask):
        return {e: self._reset(e) for e in range(self.n) if mask is None or mask[e]}

    def _action(self, e, agent):
        if agent[0] == "base_stock":
            _, sf, mu, L, cap = agent
            log = np.stack(self.log[e]) if self.log[e] else np.zeros((0, 1, len(L)), np.int64)
            return agents.base_stock(self.obs[e], int(self.t[e]), log, L, mu, sf, cap)
        if agent[0] == "order_up_to":
            return agents.order_up_to(self.obs[e], agent[2], agent[1], agent[3])
        if agent[0] == "classic_nv":
            return agents.classic_nv(self.obs[e], agent[3], agent[2], agent[4], agent[1])
        return np.asarray(agent[1])[None]

    def check_row(self, row, T, actions=None, agent=None, where=""):
        fam, mode = self.family, self.mode
        raises = False
        for e, o in enumerate(self.orcs):
            w = f"{where} env {e}"
            if mode == "next_step" and self.t[e] >= T:
                assert np.array_equal(row.obs[e], self._reset(e)), w
                assert row.reward[e] == 0 and not row.truncated[e] and not row.stepped[e], w
                assert not row.actions[e].any(), w
                continue
            if mode == "disabled" and fam != "nv" and self.t[e] >= T:
                raises = True
                assert not row.stepped[e] and not row.defined[e], w
                continue
            a = self._action(e, agent) if agent is not None else actions[e:e + 1]
            assert np.array_equal(row.actions[e], np.asarray(a).reshape(-1)), w
            if fam == "im":
                obs, r, tr, info = o.step(a, info=True)
                dem = info["demand"]
                self.log[e].append(np.maximum(np.asarray(a, np.int64).reshape(1, -1), 0))
            elif fam == "nv":
                obs, r, tr, dem = o.step(a)
            else:
                obs, r, tr, info = o.step(a, info=True)
                dem = info["D"][0].astype(np.int64)
            self.t[e] += 1
            self.obs[e] = obs
            assert row.stepped[e] and row.defined[e], w
            assert np.array_equal(r.view(np.int64), row.reward[e:e + 1].view(np.int64)), w
            assert bool(tr[0]) == bool(row.truncated[e]) == bool(self.t[e] >= T), w
            assert np.array_equal(np.asarray(dem).reshape(-1), row.demand[e]), w
            if mode == "same_step" and tr[0]:
                assert row.final_mask[e] and np.array_equal(row.final_obs[e], obs[0]), w
                assert np.array_equal(row.obs[e], self._reset(e)), w
            else:
                assert not row.final_mask[e], w
                assert np.array_equal(row.obs[e].view(np.uint8), obs[0].view(np.uint8)), w
        assert raises == row.raises, where

    def rng_state(self):
        return np.concatenate([o.rng_state() for o in self.orcs])


def _agent(family, h, kw):
    if family == "im":
        o = h.cohorts[0].orc
        return ("base_stock", 1.1, kw.get("dist_param", {"mu": 20}).get("mu", 10), o._keep["L"], o._keep["c"])
    if family == "nv":
        if kw.get("classic"):
            return ("classic_nv", "k_vs_h", 1.1, h.cohorts[0].orc.L, 2000)
        return ("order_up_to", 1.2, h.cohorts[0].orc.L, 2000)
    return ("constant", np.full(h.act_dim, 23.0, np.float32))


def _run(oracle, family, mode, variant, kw, calls):
    """Drive the script through the cohort harness and the singles; returns
    (harness, pre-row period table)."""
    okw = {k: v for k, v in kw.items() if k != "classic"}
    h = staggered.make(oracle, family, 400, variant, mode, **okw)
    ref = Singles(oracle, family, N, 400, mode, **okw)
    rng = np.random.default_rng(11)
    pre, i = [], 0
    shadow = np.zeros(N, np.int32)                 # the period table kept from the rows alone

    def one(row, a, agent, where):
        nonlocal shadow
        pre.append(shadow.copy())
        ref.check_row(row, h.T, a, agent, where)
        shadow = ref.t.copy()

    for op, arg, exp in staggered.script(h, rng, calls=_agent(family, h, kw) if calls else None):
        i += 1
        if op == "reset":
            obs, mask = exp
            got = ref.reset(arg)
            assert sorted(got) == list(np.flatnonzero(mask))
            for e, o in got.items():
                assert np.array_equal(obs[e], o), f"reset {i} env {e}"
            shadow = ref.t.copy()
        elif op in ("state", "checkpoint"):
            assert np.array_equal(h.periods(), ref.t) and np.array_equal(h.rng_state(), ref.rng_state())
        elif op == "step":
            one(exp, arg, None, f"op {i}")
        elif op == "rollout":
            for k, row in enumerate(exp):
                one(row, arg[k], None, f"op {i} row {k}")
        else:
            rows, met = exp
            want = np.zeros_like(met)
            for k, row in enumerate(rows):
                one(row, None, arg[0], f"op {i} policy row {k}")
                want[:, 0] += np.where(row.stepped, row.reward, 0.0)
                want[:, 1] += row.stepped
            assert np.array_equal(met[:, :2].view(np.int64), want[:, :2].view(np.int64)), "metrics: reward, steps"
            assert (met[:, 1] <= len(rows)).all()
    assert np.array_equal(h.periods(), ref.t)
    assert np.array_equal(h.rng_state(), ref.rng_state())
    if family == "nv":
        assert np.array_equal(h.params(), np.concatenate([o.params() for o in ref.orcs]))
    return h, np.stack(pre)


CASES = [("im", IM7), ("im", dict(IM7, backlog=False, dist=3, dist_param={"low": 0, "high": 40})), ("im", IM12),
         ("nv", dict(step_limit=7)), ("nv", dict(step_limit=7, lead_time=0, mu_max=8.0)),
         ("net", dict(num_periods=4)), ("net", dict(num_periods=30, backlog=False))]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("family,kw", CASES, ids=[f"{f}{i}" for i, (f, _) in enumerate(CASES)])
def test_cohorts_equal_single_envs(oracle, family, kw, mode):
    variant = "a" if mode != "same_step" else "b"
    h, pre = _run(oracle, family, mode, variant, kw, calls=False)
    T = h.T
    assert all(len(c.idx) > 0 for c in h.cohorts) and len(h.cohorts) == 4                     # (e)
    assert sum(len(c.idx) for c in h.cohorts) == N
    assert min(h.crossings) >= 1 and max(h.crossings) >= 2, h.crossings                       # (c)
    a, b = staggered.coverage(pre, T, mode)
    if mode == "disabled" and family != "nv":
        mixed = any(len(set(row[s:s + 64])) > 1 for row in pre for s in range(0, N, 64))
        assert mixed
    else:
        assert a, "(a) a group with resetting and stepping envs"
        assert b, "(b) a group resetting as a whole next to a stepping one"


@pytest.mark.parametrize("mode", ["next_step", "disabled"])
@pytest.mark.parametrize("family,kw", [CASES[0], CASES[3], CASES[5], ("nv", dict(step_limit=7, classic=True))],
                         ids=["im", "nv", "net", "nv_classic"])
def test_cohorts_equal_single_envs_calls(oracle, family, kw, mode):
    """the same with a rollout and a policy rollout in place of steps"""
    h, pre = _run(oracle, family, mode, "b", kw, calls=True)
    assert min(h.crossings) >= 1 and max(h.crossings) >= 2, h.crossings
    if mode == "next_step":
        a, b = staggered.coverage(pre, h.T, mode)
        assert a and b


def test_last_env_under_a_mask_in_one_schedule_only():                                        # (d)
    a, b = staggered.schedule_masks(N, "a"), staggered.schedule_masks(N, "b")
    assert a[:, N - 1].any() and not b[:, N - 1].any()
    for m in (a, b):
        assert m[1, 64:128].all() and not m[0, 64:128].all()       # group 1 whole under mask 2 only
        assert len(set(staggered.cohort_keys(m, N))) == 4


@pytest.mark.parametrize("family,kw", [("im", IM7), ("net", dict(num_periods=4))], ids=["im", "net"])
def test_fault_schedule_coverage(oracle, family, kw):
    """the DISABLED horizon-fault run: its raising row has refused and stepping
    lanes in one group (staggered.fault_script)"""
    h = staggered.make(oracle, family, 400, "a", "disabled", **kw)
    ref = Singles(oracle, family, N, 400, "disabled", **kw)
    rng = np.random.default_rng(3)
    pre, raised = [], 0
    for op, arg, exp in staggered.fault_script(h, rng):
        if op == "reset":
            ref.reset(arg)
        elif op == "step":
            pre.append(ref.t.copy())
            ref.check_row(exp, h.T, arg, None, op)
            raised += exp.raises
    assert raised == 1
    a, b = staggered.coverage(np.stack(pre), h.T, "disabled")
    assert a, "(a) refused and stepping lanes in one group"
    assert np.array_equal(h.periods(), ref.t) and np.array_equal(h.rng_state(), ref.rng_state())
