"""The case table of the parameter-limit tests: every env family at the ends
of the range its create call accepts, shared by

* tests/test_limit_cases.py (CPU): the C oracle against tests/invmgmt_model.py
  on every InvMgmt case over its whole call plan, and for Newsvendor and
  NetInvMgmt (no second restatement exists) the REACH of each case over the
  GPU test's own seeds: the order ring is walked round at least twice, every
  link delivers orders placed L periods earlier.  The counts are in the table.
* tests/test_gpu_limits.py: the kernels against the oracle, bit for bit.
* tests/test_abi.py: the create-time twins (accepted / refused), no GPU.

An InvMgmt launch asks 512 B of LDS per observation entry of a wave's window
tile, 4 KiB for the PTRS table and 512 B more on the split step
(kernels.hpp im_split_lds_bytes); a workgroup can have 160 KiB, so the largest
observation length (m-1) * (max L + 1) create accepts is 311.

A call plan is a tuple of ("step", n) and ("rollout", K): n single step()
calls, one rollout of K rows.  The InvMgmt plans keep single steps over the
first periods, the window's wrap and the first horizon (the reset step), cover
the rest with rollouts, and cross a horizon inside a rollout too (the second;
L255, of 300 periods, its only one: the step-call reset of that window depth
is L255_short's); every
plan ends on a step, so the final state is the oracle's last record.  Call c
of a plan takes actions(case)[c]; under NEXT_STEP autoreset the call after a
truncation is the reset call.
"""
import numpy as np

N_ENV = 130            # two full waves and a partial one; a partial second lookahead workgroup
LDS_LIMIT = 160 * 1024
OBS_DIM_MAX = 311      # (LDS_LIMIT - 4096 - 512) // 512


def im_lds_bytes(m1, D, split=True):
    """kernels.hpp im_run_lds_bytes / im_split_lds_bytes"""
    return 64 * m1 * (D + 1) * 8 + 512 * 8 + (64 * 8 if split else 0)


def stage_kwargs(m1):
    """Costs and capacities for m1 + 1 stages (the defaults are the reference's own, 4 stages)."""
    if m1 == 3:
        return {}
    m = m1 + 1
    return dict(I0=tuple(100 + 25 * i for i in range(m1)), p=20,
                r=tuple(15 - 1.25 * i for i in range(m)), k=tuple(0.10 - 0.01 * i for i in range(m)),
                h=tuple(0.15 - 0.015 * i for i in range(m1)), c=tuple(100 + 30 * i for i in range(m1)))


def _im(id, L, periods, plan, seed, backlog=True, autoreset="next_step", fused=False):
    m1 = len(L)
    kw = dict(stage_kwargs(m1), L=tuple(L), periods=periods)
    D = max(L)
    return dict(id=id, family="im", kwargs=kw, backlog=backlog, autoreset=autoreset, n_envs=N_ENV, seed=seed,
                plan=tuple(plan), m1=m1, D=D, obs_dim=m1 * (D + 1), lds=im_lds_bytes(m1, D), fused=fused)


# the largest accepted observation length of 4, 6 and 9 stages (309, 310, 304)
# and the smallest refused one (312, 315, 312).  Spread: a stage with L = 0, one
# with L = max, sum L > 63
OD_MAX = {4: ((17, 102, 0), 120), 6: ((61, 0, 1, 60, 5), 70), 9: ((37, 0, 1, 36, 5, 37, 2, 9), 45)}
OD_REFUSED = {4: (17, 103, 0), 6: (62, 0, 1, 60, 5), 9: (38, 0, 1, 36, 5, 37, 2, 9)}
L_DEFAULT = (1, 5, 10)

IM_CASES = [
    # two stages, max L: the ring wraps at t = 255; 128 KiB + 4.5 KiB of LDS.  Single steps over the first periods
    # and the wrap, rollouts between; the last rollout (calls 298..311) holds the truncation (299) and the reset row
    # (300) with the full, wrapped window
    _im("L255", (255,), 300, [("step", 6), ("rollout", 240), ("step", 20), ("rollout", 30), ("step", 2), ("rollout", 14), ("step", 4)], 7100),
    # periods < max L: the window never fills; three episodes begun, the second unseeded
    _im("L255_short", (255,), 40, [("step", 45), ("rollout", 50), ("step", 5)], 7200),
    _im("all_zero_backlog", (0,) * 8, 9, [("step", 12), ("rollout", 15), ("step", 5)], 7300),
    _im("all_zero_lost", (0,) * 8, 9, [("step", 12), ("rollout", 15), ("step", 5)], 7400, backlog=False),
    _im("od_max_4", OD_MAX[4][0], 120, [("step", 5), ("rollout", 95), ("step", 25), ("rollout", 120)], 7500),
    _im("od_max_6", OD_MAX[6][0], 70, [("step", 5), ("rollout", 50), ("step", 22), ("rollout", 70)], 7600, backlog=False),
    _im("od_max_9", OD_MAX[9][0], 45, [("step", 5), ("rollout", 28), ("step", 18), ("rollout", 45)], 7700, backlog=False),
    # obs_dim 123: the first size past 64 KB of dynamic LDS
    _im("above_64k", (17, 40, 3), 50, [("step", 5), ("rollout", 30), ("step", 22), ("rollout", 50)], 7800),
    # every step a truncation
    _im("T1_next", L_DEFAULT, 1, [("step", 7), ("rollout", 6), ("step", 4)], 7900),
    _im("T1_same", L_DEFAULT, 1, [("step", 8)], 7900, autoreset="same_step"),
    _im("T1_off", L_DEFAULT, 1, [("step", 8)], 7900, autoreset="disabled", backlog=False),
    # either side of IM_AP_LDS (the 3-role rollout's alpha**t table): rollouts of 30 up to period 240, then across the horizon
    _im("T256", L_DEFAULT, 256, [("rollout", 30)] * 8 + [("rollout", 30), ("step", 6)], 8000, fused=True),
    _im("T257", L_DEFAULT, 257, [("rollout", 30)] * 8 + [("rollout", 30), ("step", 6)], 8100, fused=True, backlog=False),
]
IM_IDS = [c["id"] for c in IM_CASES]
IM_BY_ID = {c["id"]: c for c in IM_CASES}
MODEL_ENVS = (0, 64, N_ENV - 1)      # the envs test_limit_cases.py restates with the numpy model


def n_calls(case):
    return sum(n for _, n in case["plan"])


def im_capacity(case):
    return np.array(case["kwargs"].get("c", (100, 200, 230)), np.int64)


def im_actions(case):
    """[calls, n_envs, m1] int64 requested orders: some negative, some above capacity"""
    rng = np.random.default_rng(case["seed"] + 1)
    c = im_capacity(case)
    return rng.integers(-5, int(c.max()) + 30, size=(n_calls(case), case["n_envs"], case["m1"])).astype(np.int64)


def reference_rows(ref, actions, autoreset="next_step"):
    """The rows the calls of a plan must return, from a freshly reset reference
    `ref`: .reset() -> obs [n, O]; .step(a) -> (obs, reward, truncated, demand).
    One dict per call: obs, reward, truncated, demand (None on a NEXT_STEP
    reset call, which steps nothing), and under same_step `final_obs` (the
    step's own observation; obs is then the reset's), under disabled
    `reset_obs` (of the reset() the caller makes after a truncation); `info` is
    the reference's own record of the step, where it keeps one (ref.info)."""
    rows, pending = [], False
    for a in actions:
        if pending:
            o = getattr(ref, "reset_call", ref.reset)()
            rows.append(dict(obs=o, reward=np.zeros(len(o)), truncated=np.zeros(len(o), bool), demand=None, reset=True))
            pending = False
            continue
        o, r, tr, d = ref.step(a)
        row = dict(obs=o, reward=r, truncated=np.asarray(tr, bool), demand=d, reset=False, info=getattr(ref, "info", None))
        if row["truncated"].any():
            assert row["truncated"].all(), "lock-step episodes"
            if autoreset == "next_step":
                pending = True
            elif autoreset == "same_step":
                row["final_obs"], row["obs"] = o, ref.reset()
            else:
                row["reset_obs"] = ref.reset()
        rows.append(row)
    return rows


class OracleIm:
    """pyoracle.OracleInvMgmt as reference_rows takes it; keeps the last step's info"""

    def __init__(self, oracle, case, envs=None, demand_stream="numpy", n=None):
        n = case["n_envs"] if n is None else n
        envs = range(n) if envs is None else envs
        self.orc = oracle.OracleInvMgmt(len(envs), backlog=case["backlog"], demand_stream=demand_stream, **case["kwargs"])
        self.orc.seed([case["seed"] + i for i in envs])
        self.info = None

    def reset(self):
        return self.orc.reset()

    def reset_call(self):
        """a NEXT_STEP reset call: on the fast stream it owns a counter value and draws nothing"""
        if self.orc.demand_stream == "philox":
            self.orc.philox_step += 1
        return self.orc.reset()

    def step(self, a):
        o, r, tr, self.info = self.orc.step(a, info=True)
        return o, r, tr, self.info["demand"]


class ModelIm:
    """tests/invmgmt_model.py, one model per env, as reference_rows takes it"""

    def __init__(self, case, envs):
        from invmgmt_model import InvMgmtModel
        self.models = [InvMgmtModel(case["seed"] + i, backlog=case["backlog"], **case["kwargs"]) for i in envs]

    def reset(self):
        return np.stack([m.reset() for m in self.models])

    def step(self, a):
        out = [m.step(a[i]) for i, m in enumerate(self.models)]
        return (np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.float64),
                np.array([o[2] for o in out], bool), np.array([o[3] for o in out], np.int64))


# ------------------------------------------------------------------ Newsvendor
# `wraps`: how often the order ring's slot index passes L within an episode of
# the plan ((step_limit - 1) // L); `late_arrivals`: over the GPU test's seeds,
# orders > 0 that arrive at a step >= 2 L (placed after the first lap), counted
# by test_limit_cases.py, which asserts at least these
def _nv(id, lead_time, step_limit, plan, seed, wraps=0, late_arrivals=0):
    return dict(id=id, family="nv", kwargs=dict(lead_time=lead_time, step_limit=step_limit), n_envs=N_ENV, seed=seed,
                plan=tuple(plan), wraps=wraps, late_arrivals=late_arrivals)


NV_CASES = [
    _nv("nv_L128", 128, 300, [("step", 5), ("rollout", 120), ("step", 10), ("rollout", 120), ("step", 10), ("rollout", 30),
                              ("step", 8), ("rollout", 10)], 9100, wraps=2, late_arrivals=5345),
    _nv("nv_L127", 127, 300, [("step", 5), ("rollout", 120), ("step", 10), ("rollout", 120), ("step", 10), ("rollout", 30),
                              ("step", 8), ("rollout", 10)], 9200, wraps=2, late_arrivals=5605),
    _nv("nv_L128_T1", 128, 1, [("step", 7), ("rollout", 6), ("step", 3)], 9300),
    _nv("nv_L0_T1", 0, 1, [("step", 7), ("rollout", 6), ("step", 3)], 9400),
]
NV_IDS = [c["id"] for c in NV_CASES]


def nv_actions(case):
    """[calls, n_envs, 1] float32 orders, small enough that max_inventory
    (4000 over up to 128 ring slots) seldom caps them: most slots hold an order"""
    rng = np.random.default_rng(case["seed"] + 1)
    return rng.uniform(-3.0, 45.0, size=(n_calls(case), case["n_envs"], 1)).astype(np.float32)


class OracleNv:
    def __init__(self, oracle, case, demand_stream="numpy"):
        self.orc = oracle.OracleNewsvendor(case["n_envs"], demand_stream=demand_stream, **case["kwargs"])
        self.orc.seed([case["seed"] + i for i in range(case["n_envs"])])

    def reset(self):
        return self.orc.reset()

    def step(self, a):
        return self.orc.step(a)


# ------------------------------------------------------------------ NetInvMgmt
# net_graphs.lds_bytes: series(1, 255) 70 400 B, series(3, 85) 77 056 B: both
# far inside the limit, so neither needs a refusal twin.  `deliveries`: the
# least number, over links, of (env, period) pairs where an order > 0 placed L
# periods earlier leaves the pipeline (counted and asserted on the CPU)
def _net(id, graph, num_periods, plan, seed, deliveries=0):
    return dict(id=id, family="net", graph=graph, num_periods=num_periods, n_envs=N_ENV, seed=seed, plan=tuple(plan),
                deliveries=deliveries)


NET_CASES = [
    _net("series1_L255", ("series", 1, 255), 300, [("step", 5), ("rollout", 245), ("step", 12), ("rollout", 33), ("step", 8),
                                                    ("rollout", 10)], 9500, deliveries=4968),
    _net("series3_L85", ("series", 3, 85), 300, [("step", 5), ("rollout", 75), ("step", 12), ("rollout", 200), ("step", 12),
                                                  ("rollout", 10)], 9600, deliveries=4937),
    _net("default_T257", ("default",), 257, [("rollout", 30)] * 8 + [("rollout", 30), ("step", 6)], 9700, deliveries=19747),
]
NET_IDS = [c["id"] for c in NET_CASES]


def net_graph(case):
    import net_graphs
    g = case["graph"]
    return net_graphs.series(g[1], L=g[2]) if g[0] == "series" else None     # None: the reference's default graph


def net_actions(case, act_dim):
    rng = np.random.default_rng(case["seed"] + 1)
    return rng.uniform(-1.0, 9.0, size=(n_calls(case), case["n_envs"], act_dim)).astype(np.float32)


class OracleNetRef:
    def __init__(self, oracle, case, demand_stream="numpy"):
        self.orc = oracle.OracleNet(case["n_envs"], graph=net_graph(case), num_periods=case["num_periods"],
                                    demand_stream=demand_stream)
        self.orc.seed([case["seed"] + i for i in range(case["n_envs"])])
        self.info = None

    def reset(self):
        return self.orc.reset()

    def step(self, a):
        o, r, tr, self.info = self.orc.step(a, info=True)
        return o, r, tr, self.info["D"].astype(np.int64)
