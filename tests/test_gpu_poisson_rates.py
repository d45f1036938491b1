"""Poisson demand at rates whose draws leave the PTRS right-hand-side table
(csrc/ptrs_table.hpp: the window [k0, k0 + nk) of at most 512 entries per rate,
none above 1e8; Newsvendor's loggam table of k < 512), on every kernel path,
bit for bit against the CPU oracle: the demand record, obs, reward bits and
flags of every call, the final "rng" rows of the state blob, on the fast
stream its "philox_step", and Newsvendor's params after every reset.  Nothing
here has a tolerance.

The rates, seeds and call plans are tests/poisson_rate_cases.py.
tests/test_ptrs_table.py pins, without a GPU and over exactly these seeds and
calls: the windows themselves (against the host's own rhs_table), that log
tests fall inside, below and above each window and that accepted draws lie
outside it (the FLOORS), and that no log test of the reference is closer to a
tie than the device's own log could move it (the MARGINS).  So a mismatch
here is a wrong k - k0, bound, table offset, staging load or off-table
formula, not a near-tie.

Launch paths are picked with the INVSIM_* switches of
tests/test_gpu_philox_oracle.py (PATHS, _make), at 1 000 envs.
"""
import numpy as np
import pytest
import torch

import poisson_rate_cases as prc
import test_gpu_numpy_samplers as tns
import test_gpu_philox_oracle as tpo

pytestmark = pytest.mark.gpu

N = prc.N_ENV
_same, _make = tpo._same, tpo._make


class _Ref(tpo._Ref):
    """tpo._Ref on either stream: on numpy's, a reset step owns no counter
    value and the PCG64 rows advance with the draws"""

    def __init__(self, orc, fam, horizon, seeds):
        self.orc, self.fam, self.T, self.t = orc, fam, horizon, 0
        self.ph = orc.demand_stream == "philox"
        orc.seed(seeds)
        self.rng0 = orc.rng_state().copy()
        self.obs0 = self.last_obs = orc.reset()
        self.log = []

    def call(self, a):
        n = self.orc.n
        if self.t == self.T:
            self.t, self.log = 0, []
            if self.ph and self.fam != "nv":
                self.orc.philox_step += 1
            self.last_obs = self.orc.reset()
            return self.last_obs, np.zeros(n), np.zeros(n, bool), None, None
        self.t += 1
        if self.fam == "im":
            self.log.append(np.maximum(np.asarray(a, np.int64), 0))
        out = self.step(a)
        self.last_obs = out[0]
        return out


def _final(env, ref, what="final state"):
    """the blob's generator rows are the oracle's (numpy stream: advanced by
    exactly the committed draws; fast stream: untouched, and the counter is the oracle's)"""
    if ref.ph:
        return tpo._final(env, ref, what)
    _same(env.state_fields()["rng"].cpu().numpy().view(np.uint64).T, ref.orc.rng_state(), f"{what}: rng rows")


def _stream_kw(c):
    return {"demand_stream": "philox"} if c["stream"] == "philox" else {}


# ================================================================ InvMgmt
def _im_pair(gpu, oracle, monkeypatch, cid, path, **kw):
    import invsim
    c = prc.CASES[cid]
    dp = {"mu": c["rates"][0]}
    cls = kw.pop("cls", c["cls"])
    env = _make(monkeypatch, "im", path,
                lambda: getattr(invsim, cls)(N, device=gpu, periods=prc.IM_T, dist=1, dist_param=dict(dp),
                                             record_demand=True, **_stream_kw(c), **kw))
    okw = {k: v for k, v in kw.items() if k != "record_info"}
    orc = oracle.OracleInvMgmt(N, periods=prc.IM_T, backlog=cls.endswith("BacklogEnv"), dist=1, dist_param=dict(dp),
                               demand_stream=c["stream"], **okw)
    ref = _Ref(orc, "im", prc.IM_T, range(c["seed"], c["seed"] + N))
    obs, _ = env.reset(seed=c["seed"])
    _same(obs, ref.obs0, "reset obs")
    return env, ref


def _drive_recording(env, ref, phases, acts, what, cid, rec=None):
    """tpo._drive, with the oracle's demands of every drawing call kept and compared with the reference's"""
    dem, step = [], ref.step

    def keep(a):
        out = step(a)
        dem.append(np.asarray(out[3]).reshape(ref.orc.n, -1))
        return out
    ref.step = keep
    tpo._drive(env, ref, phases, acts, what, rec=rec)
    ref.step = step
    live = [q for q, lam in enumerate(prc.CASES[cid]["rates"]) if lam is not None]
    want = prc.reference(cid)["demand"]
    assert len(dem) == want.shape[0] and np.array_equal(np.stack(dem)[:, :, live], want[:, :, live]), \
        "the oracle env left the CPU-checked reference"


@pytest.mark.parametrize("path", ["run", "fused", "roll2"])
@pytest.mark.parametrize("cid", ["im_200", "im_371", "im_1e4", "im_1e8", "im_1.5e8", "im_3e9", "im_371_ph", "im_1e6_ph"])
def test_invmgmt_rates(gpu, oracle, monkeypatch, cid, path):
    """12 steps (the split step draws inline, then from the lookahead slot; call
    9 is the NEXT_STEP reset step), a 23-row rollout with two reset rows (the
    3-role kernel, the 2-role one under "roll2", im_run_kernel under "run"), 8
    more steps.  200 and 371: a window that starts at k0 = 20 / 135; 1e4, 1e6,
    1e8: log tests on both sides of the window; 1.5e8, 3e9: no table.  At 3e9
    every demand is past int32 and the backlog past 2^32 from the second period."""
    env, ref = _im_pair(gpu, oracle, monkeypatch, cid, path)
    _drive_recording(env, ref, prc.PHASES, tpo._int_actions(N, 3), f"{cid}/{path}", cid)
    _final(env, ref)


def test_invmgmt_step_record(gpu, oracle, monkeypatch):
    """record_info at lam = 1e4: sales and unfulfilled of every step (it keeps rollouts on im_run_kernel)"""
    env, ref = _im_pair(gpu, oracle, monkeypatch, "im_1e4", "fused", cls="InvManagementLostSalesEnv", record_info=True)
    _drive_recording(env, ref, prc.PHASES, tpo._int_actions(N, 3), "record", "im_1e4",
                     rec={"sales": "sales", "unfulfilled": "unfulfilled"})
    _final(env, ref)


def test_invmgmt_five_stage(gpu, oracle, monkeypatch):
    """M1 = 4 with one lead time of 0 at lam = 1e4: im_run_kernel under rollouts"""
    env, ref = _im_pair(gpu, oracle, monkeypatch, "im_1e4", "fused", **tns._FIVE_STAGE)
    _drive_recording(env, ref, prc.PHASES, tpo._int_actions(N, 4), "five-stage", "im_1e4")
    _final(env, ref)


def test_invmgmt_base_stock_rollout(gpu, oracle, monkeypatch):
    """BaseStockAgent at lam = 1e4 on the fused policy kernel (its demand wave is
    another instantiation): the plan's 12 steps, its 23 rows as a policy rollout
    with actions, obs, rewards, flags and evaluate_agent's sums, its last 8 steps."""
    import agents
    import invsim
    cid, mu, z = "im_1e4", 1e4, 1.1
    env, ref = _im_pair(gpu, oracle, monkeypatch, cid, "fused")
    (_, k0), (_, K), (_, k2) = prc.PHASES
    acts = tpo._int_actions(N, 3)
    tpo._drive(env, ref, (("steps", k0),), acts, "lead-in")
    L, c = np.asarray(env.lead_time), np.asarray(env.supply_capacity)
    met = torch.zeros((N, invsim.policies.metrics_dim(env)), dtype=torch.float64, device=gpu)
    out = env.rollout_policy(invsim.BaseStockAgent(z), K, obs=True, actions=True, metrics=met)

    def act(obs, t, k):
        hist = np.stack(ref.log) if ref.log else np.zeros((0, N, 3), np.int64)
        return agents.base_stock(obs, min(t, ref.T), hist, L, mu, z, c)
    tpo._policy(env, ref, out, met, K, act, "base_stock")
    tpo._drive(env, ref, (("steps", k2),), acts, "after the policy rollout")
    _final(env, ref)


# ================================================================ NetInvMgmt
def _net_pair(gpu, oracle, monkeypatch, cid, path):
    import invsim
    c = prc.CASES[cid]
    g = prc.apply_rates(prc.net_graph(c["graph"]), c["rates"])
    env = _make(monkeypatch, "net", path,
                lambda: invsim.NetInvMgmtMasterEnv(N, device=gpu, graph=g, num_periods=prc.NET_T, backlog=True,
                                                   record_demand=True, **_stream_kw(c)))
    want = {"default": 1, "custom": 2}.get(c["graph"], 0) if path != "generic" else 0
    assert env.kernel_variant == want, (cid, path, env.kernel_variant)
    orc = oracle.OracleNet(N, graph=g, num_periods=prc.NET_T, backlog=True, demand_stream=c["stream"])
    ref = _Ref(orc, "net", prc.NET_T, range(c["seed"], c["seed"] + N))
    obs, _ = env.reset(seed=c["seed"])
    _same(obs, ref.obs0, "reset obs")
    return env, ref


_NET = [("net_custom", p) for p in ("spec", "fused", "roll2", "generic")] + \
       [(cid, p) for cid in ("net_default_1e4", "net_default_1.5e8") for p in ("spec", "fused", "roll2")] + \
       [("net_mixed", "fused")] + [("net_custom_ph", p) for p in ("spec", "fused")]


@pytest.mark.parametrize("cid,path", _NET, ids=[f"{c}-{p}" for c, p in _NET])
def test_net_rates(gpu, oracle, monkeypatch, cid, path):
    """The custom graph with rates (20, 250, 1e4) on its three markets: three
    windows (0, 114), (50, 430), (9764, 512) at table offsets 0, 114, 544, each
    staged into its own 512-entry LDS slice; the default graph at 1e4 and with
    no table at 1.5e8; a two-retailer graph of the generic kernel with rates
    371 and 1e6 around a user_D link (an empty window between theirs).  The
    plan of test_invmgmt_rates with a 10-period horizon."""
    env, ref = _net_pair(gpu, oracle, monkeypatch, cid, path)
    _drive_recording(env, ref, prc.PHASES, tpo._f32_actions(N, env.action_dim), f"{cid}/{path}", cid)
    _final(env, ref)


# ================================================================ Newsvendor
@pytest.mark.parametrize("path", ["run", "fused"])
@pytest.mark.parametrize("cid", ["nv_600", "nv_3000", "nv_1e6", "nv_3000_ph"])
def test_newsvendor_rates(gpu, oracle, monkeypatch, cid, path):
    """The episode's rate is uniform on [0, mu_max): at 600 an env's candidates
    fall on both sides of the loggam table's end (k = 512), at 3000 and 1e6
    nearly all lie past it.  Steps across two reset steps (the lookahead
    kernel), an explicit reset(), steps, the 3-wave rollout with resets inside
    (nv_roll_kernel's two stream waves), steps; params after every reset."""
    import invsim
    c = prc.CASES[cid]
    kw = dict(lead_time=prc.NV_L, step_limit=prc.NV_T, mu_max=c["rates"][0])
    env = _make(monkeypatch, "nv", path,
                lambda: invsim.NewsvendorEnv(N, device=gpu, record_demand=True, **kw, **_stream_kw(c)))
    orc = oracle.OracleNewsvendor(N, demand_stream=c["stream"], **kw)
    ref = _Ref(orc, "nv", prc.NV_T, range(c["seed"], c["seed"] + N))
    obs, _ = env.reset(seed=c["seed"])
    _same(obs, ref.obs0, "reset obs")
    _same(env.params(), orc.params(), "params after reset(seed)")
    g = np.random.default_rng(8)
    acts = lambda: g.uniform(0, 150, size=(N, 1)).astype(np.float32)   # noqa: E731
    dem, step = [], ref.step

    def keep(a):
        out = step(a)
        dem.append(np.asarray(out[3]).reshape(N, 1))
        return out
    ref.step = keep
    tpo._nv_drive(env, ref, prc.NV_PHASES, acts, f"{cid}/{path}")
    assert np.array_equal(np.stack(dem), prc.reference(cid)["demand"]), "the oracle env left the CPU-checked reference"
    _final(env, ref)
