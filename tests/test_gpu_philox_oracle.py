"""The fast demand stream (demand_stream="philox", include/invsim.h
INVSIM_DEMAND_PHILOX) on every kernel path, bit for bit against the CPU
oracle's restatement of the stream's written contract (oracle/oracle.c:
Philox4x32-10, key = the env's PCG64 increment high word, counter = (block,
draw stream, launch step), the samplers numpy's).  tests/test_oracle.py pins
that restatement without a GPU: against a pure-Python model
(tests/philox_model.py), against rocRAND's own block function run on the host,
and, over exactly the seeds and launch steps used here, the FLOORS
(tests/philox_cases.py): PTRS rejections that reach blocks j >= 1,
multiplication draws that leave a held half behind, the 32-bit integers path.

Nothing here has a tolerance: demands, obs, reward bits, flags, actions,
metrics, step records, Newsvendor params, the final "philox_step" of the state
blob and the untouched "rng" rows are compared for equality.

Launch paths are picked by the INVSIM_* switches (read when a handle is
made), at 1 000 envs (a multiple of neither 64 nor 256):

  InvMgmt   "run"    SPLIT/ROLL/POL_ROLL = 0: im_run_kernel for everything
            "fused"  the split step with its demand lookahead, the 3-role
                     rollout (one group per workgroup open loop, two under a
                     policy: 1 000 envs are 16 groups; 950 envs are 15, which
                     takes the one-group policy kernel)
            "roll2"  INVSIM_IM_ROLL3O_MAX_N = 0: the 2-role rollout, which the
                     launcher otherwise picks above 32 768 envs only
            32 897 envs: the split step's early-stores instantiation (N >
            32 768 is the code's threshold; no switch lowers it)
  Net       "spec" (AHEAD/ROLL/POL_ROLL = 0: net_spec_kernel), "fused"
            (net_step2_kernel's lookahead, the 4-role rollout without a demand
            record, the 3-role one with), "roll2" (INVSIM_NET_ROLL3 = 0,
            ROLL4_MAX_N = 0: net_roll_kernel), "generic" (INVSIM_NET_GENERIC = 1)
  Newsvendor "run" (AHEAD/ROLL/POL_ROLL = 0) and "fused"
"""
import numpy as np
import pytest
import torch

import levels_model
import philox_cases as pc
import random_agent_model as model

pytestmark = pytest.mark.gpu

N = pc.N_ENV
ASEED = 91

PATHS = {
    "im": {"run": {"INVSIM_IM_SPLIT": "0", "INVSIM_IM_ROLL": "0", "INVSIM_IM_POL_ROLL": "0"},
           "fused": {},
           "roll2": {"INVSIM_IM_ROLL3O_MAX_N": "0"},
           "g2": {"INVSIM_IM_ROLL3O_G2": "1"}},
    "net": {"spec": {"INVSIM_NET_AHEAD": "0", "INVSIM_NET_ROLL": "0", "INVSIM_NET_POL_ROLL": "0"},
            "fused": {},
            "roll2": {"INVSIM_NET_ROLL3": "0", "INVSIM_NET_ROLL4_MAX_N": "0"},
            "generic": {"INVSIM_NET_GENERIC": "1"}},
    "nv": {"run": {"INVSIM_NV_AHEAD": "0", "INVSIM_NV_ROLL": "0", "INVSIM_NV_POL_ROLL": "0"},
           "fused": {}},
}
_ALL_SWITCHES = sorted({k for fam in PATHS.values() for sw in fam.values() for k in sw})


def _make(monkeypatch, fam, path, ctor):
    """ctor() with the path's switches set (a handle reads them once, when it is made)"""
    for k in _ALL_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in PATHS[fam][path].items():
        monkeypatch.setenv(k, v)
    env = ctor()
    for k in PATHS[fam][path]:
        monkeypatch.delenv(k, raising=False)
    return env


# ---------------------------------------------------------------- comparison
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32, 1: np.uint8}[a.dtype.itemsize])


def _same(t, exp, what):
    got = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    exp = np.asarray(exp)
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, got.dtype, exp.shape, exp.dtype)
    eq = _bits(got) == _bits(exp)
    if not eq.all():
        bad = np.argwhere(~eq)
        pytest.fail(f"{what}: {len(bad)} of {eq.size} differ, first at {bad[0].tolist()}: "
                    f"got {got[tuple(bad[0])]!r}, expected {exp[tuple(bad[0])]!r}")


def _final(env, ref, what="final state"):
    """the blob's launch-step counter is the oracle's, and the PCG64 rows are the seeded ones"""
    f = env.state_fields()
    assert int(f["philox_step"].cpu().numpy().view(np.uint64).reshape(-1)[0]) == ref.orc.philox_step, what
    _same(f["rng"].cpu().numpy().view(np.uint64).T, ref.rng0, f"{what}: rng rows")
    assert np.array_equal(ref.orc.rng_state(), ref.rng0), "the oracle's PCG64 states moved"


class _Ref:
    """An oracle env on the fast stream under NEXT_STEP autoreset, with the
    counter rules of include/invsim.h: the call after the horizon is the reset
    step, which consumes a counter value (InvMgmt / Net: no draw; Newsvendor:
    the five uniforms of draw stream RESET at that value)."""

    def __init__(self, orc, fam, horizon, seeds):
        self.orc, self.fam, self.T, self.t = orc, fam, horizon, 0
        assert orc.demand_stream == "philox"
        orc.seed(seeds)
        assert orc.philox_step == 0
        self.rng0 = orc.rng_state().copy()
        self.obs0 = self.last_obs = orc.reset()
        self.log = []                              # the episode's requested orders (InvMgmt's action_log rows)

    def step(self, a):
        """(obs, reward, truncated, demand [n, D] int64, info)"""
        if self.fam == "nv":
            o, r, tr, d = self.orc.step(a)
            return o, r, tr, d.reshape(-1, 1), {}
        o, r, tr, info = self.orc.step(a, info=True)
        d = info["demand"].reshape(-1, 1) if self.fam == "im" else info["D"].astype(np.int64)
        return o, r, tr, d, info

    def call(self, a):
        n = self.orc.n
        if self.t == self.T:
            self.t, self.log = 0, []
            if self.fam != "nv":
                self.orc.philox_step += 1          # the reset step's own counter value; nothing drawn
            self.last_obs = self.orc.reset()
            return self.last_obs, np.zeros(n), np.zeros(n, bool), None, None
        self.t += 1
        if self.fam == "im":
            self.log.append(np.maximum(np.asarray(a, np.int64), 0))
        out = self.step(a)
        self.last_obs = out[0]
        return out

    def check(self, o, r, te, tr, a, what, demand=None, rec=None):
        e_obs, e_rew, e_tr, e_dem, e_info = self.call(a)
        _same(o, e_obs, f"{what}: obs")
        _same(r, e_rew, f"{what}: reward")
        _same(tr, e_tr, f"{what}: truncated")
        assert not bool(torch.as_tensor(te).any()), f"{what}: terminated"
        if demand is not None and e_dem is not None:
            _same(demand.reshape(e_dem.shape), e_dem, f"{what}: demand")
        if rec is not None and e_info:
            for k, v in rec.items():
                _same(v, e_info[k], f"{what}: record {k}")
        return e_info


def _drive(env, ref, phases, gen_actions, what, rec=None):
    """phases of ("steps", k) / ("rollout", K) on the device env against ref, every call checked"""
    call = 0
    for kind, k in phases:
        if kind == "steps":
            for _ in range(k):
                a = gen_actions()
                o, r, te, tr, info = env.step(torch.from_numpy(a).to(env.device))
                ref.check(o, r, te, tr, a, f"{what} call {call} (step)", info.get("demand"),
                          {dst: info[src] for src, dst in rec.items()} if rec else None)
                call += 1
        else:
            A = np.stack([gen_actions() for _ in range(k)])
            o, r, te, tr = env.rollout(torch.from_numpy(A).to(env.device))
            for j in range(k):
                last = j == k - 1 and env._demand is not None
                ref.check(o[j], r[j], te[j], tr[j], A[j], f"{what} call {call} (rollout row {j})",
                          env._demand if last else None)     # the demand record is the launch's last row's
                call += 1


class _Sums:
    """evaluate_agent's per-env sums as oracle/agents.py keeps them"""

    def __init__(self, fam, n, J=0):
        self.fam, self.m = fam, np.zeros((n, {"im": 6, "nv": 2}.get(fam, 5 + J)))

    def add(self, r, info):
        m = self.m
        m[:, 0] += r
        m[:, 1] += 1
        if self.fam == "im":
            m[:, 2] += info["demand"]
            m[:, 3] += info["sales"][:, 0]
            m[:, 4] += info["unfulfilled"][:, 0]
            m[:, 5] += np.maximum(0, info["ending_inventory"]).sum(axis=1)
        elif self.fam == "net":
            for q in range(info["D"].shape[1]):
                m[:, 2] += info["D"][:, q]
                m[:, 3] += info["S"][:, q]
                m[:, 4] += info["U"][:, q]
            m[:, 5:] += info["X"]


def _policy(env, ref, out, met, K, act, what, every_row_acts=False):
    """A policy rollout's rows against the oracle driven in closed loop:
    act(obs, t, k) is the model's action of row k from the oracle's own obs."""
    sums = _Sums(ref.fam, ref.orc.n, ref.orc.topo["J"] if ref.fam == "net" else 0)
    for k in range(K):
        reset_row = ref.t == ref.T
        a = act(ref.last_obs, ref.t, k)
        e_obs, e_rew, e_tr, _, e_info = ref.call(a)
        _same(out["obs"][k], e_obs, f"{what} row {k}: obs")
        _same(out["reward"][k], e_rew, f"{what} row {k}: reward")
        _same(out["truncated"][k], e_tr, f"{what} row {k}: truncated")
        if "actions" in out and (every_row_acts or not reset_row):
            _same(out["actions"][k], a, f"{what} row {k}: action")
        if not reset_row:
            sums.add(e_rew, e_info)
    assert not bool(out["terminated"].any())
    if met is not None:
        _same(met, sums.m, f"{what}: metrics")


def _int_actions(n, a_dim, seed=2, hi=120):
    g = np.random.default_rng(seed)
    return lambda: g.integers(0, hi, size=(n, a_dim))


def _f32_actions(n, a_dim, seed=4, hi=60.0):
    g = np.random.default_rng(seed)
    return lambda: g.uniform(0, hi, size=(n, a_dim)).astype(np.float32)


# ================================================================ InvMgmt
_IM_PHASES = (("steps", 33), ("rollout", 45))        # pc.IM_STEPS launch steps; calls 30 and 61 are reset steps


def _im_pair(gpu, oracle, monkeypatch, path, cls, n, dist, dp, seed, **kw):
    import invsim
    env = _make(monkeypatch, "im", path,
                lambda: getattr(invsim, cls)(n, device=gpu, dist=dist, dist_param=dict(dp), record_demand=True,
                                             demand_stream="philox", **kw))
    okw = {k: v for k, v in kw.items() if k not in ("autoreset_mode", "record_info")}
    orc = oracle.OracleInvMgmt(n, backlog=cls.endswith("BacklogEnv"), dist=dist, dist_param=dict(dp),
                               demand_stream="philox", **okw)
    ref = _Ref(orc, "im", env.num_periods, range(seed, seed + n))
    obs, _ = env.reset(seed=seed)
    _same(obs, ref.obs0, "reset obs")
    return env, ref


@pytest.mark.parametrize("path", ["run", "fused"])
@pytest.mark.parametrize("case", list(pc.IM_CASES))
def test_invmgmt_steps_and_rollout(gpu, oracle, monkeypatch, case, path):
    """33 steps across the NEXT_STEP reset step (the split kernel draws launch
    step s + 1 ahead; the reset step consumes a counter value and draws
    nothing), then a 45-row rollout with its own reset row: every demand, obs,
    reward and flag, for Poisson rates on both sampler branches and at their
    boundary, and for the binomial / integers / geometric samplers (which carry
    no 32-bit half from one step to the next on this stream)."""
    dist, dp, seed = pc.IM_CASES[case]
    env, ref = _im_pair(gpu, oracle, monkeypatch, path, "InvManagementBacklogEnv", N, dist, dp, seed)
    _drive(env, ref, _IM_PHASES, _int_actions(N, 3), f"{case}/{path}")
    assert ref.orc.philox_step == pc.IM_STEPS
    _final(env, ref)


@pytest.mark.parametrize("path", ["run", "fused", "roll2", "g2"])
@pytest.mark.parametrize("cls", ["InvManagementBacklogEnv", "InvManagementLostSalesEnv"])
def test_invmgmt_rollout_kernels(gpu, oracle, monkeypatch, cls, path):
    """K = 45 rollouts first thing after the reset and again mid-episode, on
    im_run_kernel, the 3-role kernel with one and with two groups per workgroup,
    and the 2-role kernel; Backlog and LostSales."""
    dist, dp, seed = pc.IM_CASES["mu20"]
    env, ref = _im_pair(gpu, oracle, monkeypatch, path, cls, N, dist, dp, seed + 7)
    _drive(env, ref, (("rollout", 45), ("steps", 3), ("rollout", 45)), _int_actions(N, 3, seed=3), f"{cls}/{path}")
    _final(env, ref)


def test_invmgmt_early_stores_instantiation(gpu, oracle, monkeypatch):
    """N > 32 768 (the code's threshold, IM_EARLY_STORES_MIN_N): the lookahead
    steps run the split kernel's EARLY instantiation; 32 897 envs leave partial
    last workgroups.  8 steps and a 3-row rollout."""
    n = 32768 + 129
    env, ref = _im_pair(gpu, oracle, monkeypatch, "fused", "InvManagementBacklogEnv", n, 1, {"mu": 20}, 5000)
    _drive(env, ref, (("steps", 8), ("rollout", 3)), _int_actions(n, 3), "early")
    _final(env, ref)


def test_invmgmt_user_demand_draws_nothing(gpu, oracle, monkeypatch):
    """dist 5 replays user_D on either stream; the counter still advances."""
    uD = [int(x) for x in np.random.default_rng(1).integers(0, 60, 30)]
    for path in ("run", "fused"):
        env, ref = _im_pair(gpu, oracle, monkeypatch, path, "InvManagementBacklogEnv", 300, 5, {}, 5100, user_D=uD)
        _drive(env, ref, (("steps", 33), ("rollout", 10)), _int_actions(300, 3), f"user_D/{path}")
        assert ref.orc.philox_step == 43
        _final(env, ref)


@pytest.mark.parametrize("path", ["run", "fused"])
def test_invmgmt_same_step_autoreset(gpu, oracle, monkeypatch, path):
    """SAME_STEP: the done step resets in place (no counter value of its own),
    two episode ends in 65 steps; the last step of an episode leaves the split path."""
    n, seed = 300, 5200
    env, ref = _im_pair(gpu, oracle, monkeypatch, path, "InvManagementBacklogEnv", n, 1, {"mu": 20}, seed,
                        autoreset_mode="same_step")
    orc, acts = ref.orc, _int_actions(n, 3)
    for s in range(65):
        a = acts()
        o, r, te, tr, info = env.step(torch.from_numpy(a).to(gpu))
        e_obs, e_rew, e_tr, e_info = orc.step(a, info=True)
        _same(r, e_rew, f"step {s}: reward")
        _same(tr, e_tr, f"step {s}: truncated")
        _same(info["demand"], e_info["demand"], f"step {s}: demand")
        if e_tr.all():
            _same(info["final_obs"], e_obs, f"step {s}: final obs")
            e_obs = orc.reset()
        _same(o, e_obs, f"step {s}: obs")
    assert orc.philox_step == 65
    _final(env, ref)


def test_invmgmt_step_record(gpu, oracle, monkeypatch):
    """record_info on the fast stream (steps; it keeps rollouts on im_run_kernel):
    sales and unfulfilled of every step."""
    for path in ("run", "fused"):
        env, ref = _im_pair(gpu, oracle, monkeypatch, path, "InvManagementLostSalesEnv", 300, 1, {"mu": 9.99}, 5300,
                            record_info=True)
        _drive(env, ref, (("steps", 33), ("rollout", 5), ("steps", 2)), _int_actions(300, 3), f"record/{path}",
               rec={"sales": "sales", "unfulfilled": "unfulfilled"})
        _final(env, ref)


@pytest.mark.parametrize("n", [N, 950])
@pytest.mark.parametrize("path", ["run", "fused"])
@pytest.mark.parametrize("agent", ["base_stock", "levels", "random", "external"])
def test_invmgmt_policy_rollouts(gpu, oracle, monkeypatch, agent, path, n):
    """BaseStock, Levels (per-env levels with reorder points), Random and
    caller-supplied actions (rollout_metrics), K = 45 after 4 steps: the reset
    row falls inside the launch.  1 000 envs are 16 groups (two per workgroup
    on the fused policy kernel), 950 are 15 (one per workgroup).  Actions, obs,
    reward bits, flags and evaluate_agent's sums, with the oracle driven in
    closed loop by oracle/agents.py, tests/levels_model.py and
    tests/random_agent_model.py."""
    import agents
    import invsim
    K, mu = 45, 20
    env, ref = _im_pair(gpu, oracle, monkeypatch, path, "InvManagementBacklogEnv", n, 1, {"mu": mu}, 5400)
    _drive(env, ref, (("steps", 4),), _int_actions(n, 3), "lead-in")
    L, c = np.asarray(env.lead_time), np.asarray(env.supply_capacity)
    met = torch.zeros((n, invsim.policies.metrics_dim(env)), dtype=torch.float64, device=gpu)
    every = False
    if agent == "external":
        A = np.random.default_rng(3).integers(0, 120, size=(K, n, 3))
        out = env.rollout_metrics(torch.from_numpy(A).to(gpu), metrics=met)
        act = lambda obs, t, k: A[k]                                           # noqa: E731
    elif agent == "random":
        out = env.rollout_policy(invsim.RandomAgent(seed=ASEED), K, obs=True, actions=True, metrics=met)
        A, _ = model.expected_actions(ASEED, 0, n, K, env._action_high(), np.int64)
        act, every = (lambda obs, t, k: A[k]), True                            # noqa: E731
    elif agent == "levels":
        g = np.random.default_rng(5)
        lv, ro = g.uniform(0, 400, size=(n, 3)), g.uniform(50, 500, size=(n, 3))
        out = env.rollout_policy(invsim.LevelsAgent(lv, ro), K, obs=True, actions=True, metrics=met)
        act = lambda obs, t, k: levels_model.action(obs, t, L, c, lv, ro)      # noqa: E731
    else:
        out = env.rollout_policy(invsim.BaseStockAgent(1.1), K, obs=True, actions=True, metrics=met)

        def act(obs, t, k):
            hist = np.stack(ref.log) if ref.log else np.zeros((0, n, 3), np.int64)
            return agents.base_stock(obs, min(t, ref.T), hist, L, mu, 1.1, c)
    _policy(env, ref, out, met, K, act, f"{agent}/{path}/{n}", every_row_acts=every)
    _final(env, ref)


# ================================================================ NetInvMgmt
def _net_graph(name):
    import net_graphs
    from invsim.topology import custom_graph, default_graph
    if name == "default":
        return default_graph(), 30
    if name == "custom":
        return custom_graph(), 30
    if name == "user_d_between":
        # markets in draw order: binomial, a user_D replay (draws nothing, still owns stream 1), poisson
        return net_graphs.mixed(net_graphs.by_name, 12), 12
    if name == "no_source_first":
        # markets in draw order: no demand source (nothing drawn), poisson, geometric
        return net_graphs.chain(net_graphs.by_name, 10), 10
    if name == "samplers":
        # integers [0, 2^31] (rejects every other draw: the 32-bit half it leaves buffered, or not, is the
        # next integers market's first 32 bits, within the step only), geometric, integers [2, 41]
        g = custom_graph()
        markets = [e for e in g.edges() if "L" not in g.edges[e]]
        for e, (fn, dp) in zip(markets, [("integers", {"low": 0, "high": 2**31 + 1}), ("geometric", {"p": 0.07}),
                                         ("integers", {"low": 2, "high": 42})]):     # numpy's exclusive high
            g.edges[e]["demand_dist_func"] = fn
            g.edges[e]["dist_param"] = dp
        return g, 30
    raise KeyError(name)


def _net_pair(gpu, oracle, monkeypatch, path, graph, n, seed, record_demand=True, **kw):
    import invsim
    g, T = _net_graph(graph)
    env = _make(monkeypatch, "net", path,
                lambda: invsim.NetInvMgmtMasterEnv(n, device=gpu, graph=g, num_periods=T, backlog=True,
                                                   record_demand=record_demand, demand_stream="philox", **kw))
    want = {"default": 1, "custom": 2}.get(graph, 0) if path != "generic" else 0
    assert env.kernel_variant == want, (graph, path, env.kernel_variant)
    orc = oracle.OracleNet(n, graph=g, num_periods=T, backlog=True, demand_stream="philox")
    ref = _Ref(orc, "net", T, range(seed, seed + n))
    obs, _ = env.reset(seed=seed)
    _same(obs, ref.obs0, "reset obs")
    return env, ref


@pytest.mark.parametrize("path", ["spec", "fused", "roll2", "generic"])
@pytest.mark.parametrize("graph", ["default", "custom"])
def test_net_builtin_graphs(gpu, oracle, monkeypatch, graph, path):
    """33 steps across the reset step (net_step2_kernel draws launch step s + 1
    ahead) and a 45-row rollout, on the compiled kernels (net_spec_kernel; the
    3-role and, with INVSIM_NET_ROLL3 = 0, the 2-role rollout) and forced onto
    the generic kernel.  The custom graph's three Poisson(20) markets must come
    from draw streams 0, 1, 2."""
    env, ref = _net_pair(gpu, oracle, monkeypatch, path, graph, N, pc.NET_SEED[graph])
    _drive(env, ref, (("steps", 33), ("rollout", 45)), _f32_actions(N, env.action_dim), f"{graph}/{path}")
    _final(env, ref)


@pytest.mark.parametrize("graph", ["default", "custom"])
def test_net_four_role_rollout(gpu, oracle, monkeypatch, graph):
    """Without a demand record, open-loop rollouts of small batches run
    net_roll4_kernel: K = 45 first thing and again after three steps."""
    env, ref = _net_pair(gpu, oracle, monkeypatch, "fused", graph, N, pc.NET_SEED[graph] + 50, record_demand=False)
    _drive(env, ref, (("rollout", 45), ("steps", 3), ("rollout", 45)), _f32_actions(N, env.action_dim), f"{graph}/roll4")
    _final(env, ref)


@pytest.mark.parametrize("graph", ["user_d_between", "no_source_first", "samplers"])
def test_net_other_graphs(gpu, oracle, monkeypatch, graph):
    """The generic kernel on graphs whose markets do not all draw: a user_D
    replay between a binomial and a Poisson market, and a market without a
    demand source in front of a Poisson and a geometric one.  A market keeps
    its draw stream (its index in retail-link order) whether or not it draws.
    "samplers": two integers markets around a geometric one; the 32-bit half
    starts every launch step empty and passes from one integers market to the
    next within it."""
    env, ref = _net_pair(gpu, oracle, monkeypatch, "fused", graph, N, pc.NET_SEED.get(graph, 3300))
    T = ref.T
    _drive(env, ref, (("steps", T + 3), ("rollout", 2 * T + 3)), _f32_actions(N, env.action_dim, hi=40.0), graph)
    _final(env, ref)


def test_net_step_record(gpu, oracle, monkeypatch):
    """record_info on the custom graph's compiled kernel: the step record's
    sales, backlog, inventory, replenishment, pipeline and profit columns."""
    env, ref = _net_pair(gpu, oracle, monkeypatch, "fused", "custom", 300, 3500, record_info=True)
    _drive(env, ref, (("steps", 33),), _f32_actions(300, env.action_dim), "net record",
           rec={"sales": "S", "unfulfilled": "U", "inventory": "X", "replenishment": "R", "pipeline": "Y",
                "profit": "P"})
    _final(env, ref)


@pytest.mark.parametrize("path", ["spec", "fused", "generic"])
@pytest.mark.parametrize("agent", ["constant", "random"])
@pytest.mark.parametrize("graph", ["default", "custom"])
def test_net_policy_rollouts(gpu, oracle, monkeypatch, graph, agent, path):
    """ConstantOrder and Random policy rollouts, K = 45 after 4 steps (the
    reset row inside the launch), with evaluate_agent's sums."""
    import invsim
    K = 45
    env, ref = _net_pair(gpu, oracle, monkeypatch, path, graph, N, pc.NET_SEED[graph] + 100)
    _drive(env, ref, (("steps", 4),), _f32_actions(N, env.action_dim), "lead-in")
    met = torch.zeros((N, invsim.policies.metrics_dim(env)), dtype=torch.float64, device=gpu)
    if agent == "constant":
        ag = invsim.ConstantOrderAgent(0.1)
        out = env.rollout_policy(ag, K, obs=True, actions=True, metrics=met)
        a0 = np.broadcast_to(ag.action(env), (N, env.action_dim)).astype(np.float32)
        _policy(env, ref, out, met, K, lambda obs, t, k: a0, f"{graph}/{agent}/{path}")
    else:
        out = env.rollout_policy(invsim.RandomAgent(seed=ASEED), K, obs=True, actions=True, metrics=met)
        A, _ = model.expected_actions(ASEED, 0, N, K, env._action_high(), np.float32)
        _policy(env, ref, out, met, K, lambda obs, t, k: A[k], f"{graph}/{agent}/{path}", every_row_acts=True)
    _final(env, ref)


# ================================================================ Newsvendor
def _nv_pair(gpu, oracle, monkeypatch, path, case, n=N, **kw):
    import invsim
    (L, limit, mu_max), seed = pc.NV_CASES[case]
    env = _make(monkeypatch, "nv", path,
                lambda: invsim.NewsvendorEnv(n, device=gpu, lead_time=L, step_limit=limit, mu_max=mu_max,
                                             record_demand=True, demand_stream="philox", **kw))
    orc = oracle.OracleNewsvendor(n, lead_time=L, step_limit=limit, mu_max=mu_max, demand_stream="philox")
    ref = _Ref(orc, "nv", limit, range(seed, seed + n))
    obs, _ = env.reset(seed=seed)
    _same(obs, ref.obs0, "reset obs")
    _same(env.params(), orc.params(), "params after reset(seed)")
    assert orc.philox_step == 1, "invsim_reset on Newsvendor owns one counter value"
    return env, ref, (L, limit)


def _nv_drive(env, ref, phases, acts, what):
    """_drive that also compares params() after every call that reset"""
    call = 0
    for kind, k in phases:
        if kind == "steps":
            for _ in range(k):
                a = acts()
                was_reset = ref.t == ref.T
                o, r, te, tr, info = env.step(torch.from_numpy(a).to(env.device))
                ref.check(o, r, te, tr, a, f"{what} call {call} (step)", info.get("demand"))
                if was_reset:
                    _same(env.params(), ref.orc.params(), f"{what} call {call}: params after the reset step")
                call += 1
        elif kind == "rollout":
            A = np.stack([acts() for _ in range(k)])
            o, r, te, tr = env.rollout(torch.from_numpy(A).to(env.device))
            for j in range(k):
                ref.check(o[j], r[j], te[j], tr[j], A[j], f"{what} call {call} (rollout row {j})",
                          env._demand if j == k - 1 else None)
                call += 1
            _same(env.params(), ref.orc.params(), f"{what}: params after the rollout")
        elif kind == "reset":
            obs, _ = env.reset()
            ref.t = 0
            e = ref.last_obs = ref.orc.reset()
            _same(obs, e, f"{what}: explicit reset obs")
            _same(env.params(), ref.orc.params(), f"{what}: params after reset()")
        else:
            raise KeyError(kind)


@pytest.mark.parametrize("path", ["run", "fused"])
@pytest.mark.parametrize("case", list(pc.NV_CASES))
def test_newsvendor_steps_resets_rollout(gpu, oracle, monkeypatch, case, path):
    """Steps across two NEXT_STEP reset steps (the lookahead kernel; the reset's
    five uniforms come from draw stream RESET at the step's counter value), an
    explicit reset() between steps (it owns a counter value), then the 3-wave
    rollout of 2 * limit + 7 rows with resets mid-launch, and steps again;
    params() after every reset.  mu_max = 14 puts episodes on both Poisson
    branches (tests/test_oracle.py counts them)."""
    env, ref, (L, limit) = _nv_pair(gpu, oracle, monkeypatch, path, case)
    g = np.random.default_rng(8)
    acts = lambda: g.uniform(0, 150, size=(N, 1)).astype(np.float32)   # noqa: E731
    _nv_drive(env, ref, (("steps", limit + 6), ("reset", 0), ("steps", 5), ("rollout", 2 * limit + 7), ("steps", 3)),
              acts, f"{case}/{path}")
    _final(env, ref)


@pytest.mark.parametrize("path", ["run", "fused"])
def test_newsvendor_masked_reset_between_steps(gpu, oracle, monkeypatch, path):
    """A masked reset() mid-episode advances the handle's counter by one for
    every env (the masked envs draw their parameters at its old value); the
    periods then differ per env, so the per-env-period kernels run, with reset
    lanes (stream RESET) beside stepping lanes (stream 0) in one wave."""
    import staggered
    case = "L2_mu14"
    (L, limit, mu_max), seed = pc.NV_CASES[case]
    n = staggered.N
    h = staggered.make(oracle, "nv", seed, "a", "next_step", n=n, lead_time=L, step_limit=limit, mu_max=mu_max,
                       demand_stream="philox")
    _count_launch_steps(h)
    _staggered_run(gpu, monkeypatch, h, "nv", path, seed,
                   lambda inv: inv.NewsvendorEnv(n, device=gpu, lead_time=L, step_limit=limit, mu_max=mu_max,
                                                 record_demand=True, demand_stream="philox"))


@pytest.mark.parametrize("path", ["run", "fused"])
@pytest.mark.parametrize("agent", ["order_up_to", "classic", "random"])
@pytest.mark.parametrize("case", list(pc.NV_CASES))
def test_newsvendor_policy_rollouts(gpu, oracle, monkeypatch, case, agent, path):
    """OrderUpTo, ClassicNewsvendor and Random policy rollouts of limit + 9 rows
    after 3 steps (a reset row inside the launch).  The classic agent's model
    calls scipy's ppf per env and row, so it runs on 300 envs, the others on
    1 000."""
    import agents
    import invsim
    n = 300 if agent == "classic" else N
    env, ref, (L, limit) = _nv_pair(gpu, oracle, monkeypatch, path, case, n=n)
    g = np.random.default_rng(9)
    _nv_drive(env, ref, (("steps", 3),), lambda: g.uniform(0, 150, size=(n, 1)).astype(np.float32), "lead-in")
    K = limit + 9
    met = torch.zeros((n, 2), dtype=torch.float64, device=gpu)
    mo = env.max_order_quantity
    every = False
    if agent == "order_up_to":
        out = env.rollout_policy(invsim.OrderUpToHeuristicAgent(1.2), K, obs=True, actions=True, metrics=met)
        act = lambda obs, t, k: agents.order_up_to(obs, L, 1.2, mo)                          # noqa: E731
    elif agent == "classic":
        out = env.rollout_policy(invsim.ClassicNewsvendorAgent("profit_margin", 0.9), K, obs=True, actions=True,
                                 metrics=met)
        act = lambda obs, t, k: agents.classic_nv(obs, L, 0.9, mo, "profit_margin")          # noqa: E731
    else:
        out = env.rollout_policy(invsim.RandomAgent(seed=ASEED), K, obs=True, actions=True, metrics=met)
        A, _ = model.expected_actions(ASEED, 0, n, K, env._action_high(), np.float32)
        act, every = (lambda obs, t, k: A[k]), True                                          # noqa: E731
    _policy(env, ref, out, met, K, act, f"{case}/{agent}/{path}", every_row_acts=every)
    _same(env.params(), ref.orc.params(), "params after the policy rollout")
    _final(env, ref)


# ================================================================ staggered periods
def _count_launch_steps(h):
    """Give a staggered.CohortOracle the handle's one launch-step counter: every
    cohort oracle is put at the counter's value before a call, a row adds one,
    and so does a reset() of Newsvendor envs (masked or not); a reset inside a
    row (the NEXT_STEP reset row, SAME_STEP's reset in the done step) draws at
    the row's own value."""
    h.ph = 0
    row, reset, reset_cohort = h.row, h.reset, h._reset_cohort

    def sync():
        for c in h.cohorts:
            c.orc.philox_step = h.ph

    def reset_cohort_at(c):
        c.orc.philox_step = h.ph
        return reset_cohort(c)

    def row_counted(*a, **kw):
        sync()
        out = row(*a, **kw)
        h.ph += 1
        return out

    def reset_counted(mask=None):
        sync()
        out = reset(mask)
        if h.family == "nv":
            h.ph += 1
        return out
    h.row, h.reset, h._reset_cohort = row_counted, reset_counted, reset_cohort_at


def _staggered_run(gpu, monkeypatch, h, fam, path, seed, ctor, agent=None, calls=None):
    import invsim
    import staggered
    import test_gpu_staggered as tgs
    assert h.n == tgs.N
    monkeypatch.setattr(tgs, "SEED", seed)                # the seed its driver gives the first reset
    env = _make(monkeypatch, fam, path, lambda: ctor(invsim))
    rng0 = h.rng_state().copy()
    tgs._drive([tgs._Dev(env, f"{fam}/{path}")], h, staggered.script(h, np.random.default_rng(1), calls=calls),
               agent=agent)
    f = env.state_fields()
    assert int(f["philox_step"].cpu().numpy().view(np.uint64).reshape(-1)[0]) == h.ph
    _same(f["rng"].cpu().numpy().view(np.uint64).T, rng0, "rng rows")


@pytest.mark.parametrize("path", ["run", "fused"])
def test_invmgmt_staggered_periods(gpu, oracle, monkeypatch, path):
    """tests/staggered.py's run (masked resets, then per-env periods: every env
    steps or resets at a row of its own) with a rollout of 2 * horizon + 5 rows
    and a BaseStock policy rollout, on the fast stream: the counter is the
    handle's, whatever an env's period."""
    import invsim
    import staggered
    n, seed, kw = staggered.N, 5600, dict(periods=7, backlog=True)
    h = staggered.make(oracle, "im", seed, "b", "next_step", n=n, demand_stream="philox", **kw)
    _count_launch_steps(h)
    _staggered_run(gpu, monkeypatch, h, "im", path, seed,
                   lambda inv: inv.InvManagementBacklogEnv(n, device=gpu, periods=7, record_demand=True,
                                                           demand_stream="philox"),
                   agent=invsim.BaseStockAgent(1.1),
                   calls=("base_stock", 1.1, 20, np.array([1, 5, 10]), np.array([100, 200, 230])))


# ================================================================ the launch-step counter
def _set_counter(env, value):
    """write the state blob's philox_step through its state_fields view, then set_state"""
    blob = env.get_state().clone()
    f = env.state_fields(blob)["philox_step"]
    f.view(torch.int64).fill_(int(np.array(value, np.uint64).view(np.int64)))
    env.set_state(blob)
    got = env.state_fields()["philox_step"].cpu().numpy().view(np.uint64).reshape(-1)[0]
    assert int(got) == value


@pytest.mark.parametrize("path", ["per_env", "run", "fused"])
@pytest.mark.parametrize("fam", ["im", "net", "nv"])
def test_counter_carry_past_2_to_32(gpu, oracle, monkeypatch, fam, path):
    """philox_step = 2^32 - 3 through the state blob, then 6 steps and a K = 5
    rollout across the carry into the counter's high word (counter word 3),
    against the oracle put at the same value.  After set_state the host knows
    no common period, so the per-env-period kernels run ("per_env"); an
    unmasked reset() after it (which keeps the counter; Newsvendor's takes one
    value) brings back the lock-step kernels of "run" and "fused"."""
    start = 2**32 - 3
    relock, path = path != "per_env", "fused" if path == "per_env" else path
    if fam == "im":
        env, ref = _im_pair(gpu, oracle, monkeypatch, path, "InvManagementBacklogEnv", N, 1, {"mu": 20}, 5700)
        acts = _int_actions(N, 3)
    elif fam == "net":
        env, ref = _net_pair(gpu, oracle, monkeypatch, path if path == "fused" else "spec", "custom", N, 5800)
        acts = _f32_actions(N, env.action_dim)
    else:
        env, ref, _ = _nv_pair(gpu, oracle, monkeypatch, path, "L5")
        acts = _f32_actions(N, 1, hi=150.0)
    _drive(env, ref, (("steps", 2),), acts, "lead-in")          # a live lookahead cache for set_state to drop
    _set_counter(env, start)
    ref.orc.philox_step = start
    if relock:
        obs, _ = env.reset()
        ref.t, ref.log = 0, []
        ref.last_obs = ref.orc.reset()
        _same(obs, ref.last_obs, "reset obs")
        if fam == "nv":
            _same(env.params(), ref.orc.params(), "params drawn at counter 2^32 - 3")
    _drive(env, ref, (("steps", 6), ("rollout", 5)), acts, f"{fam}/{path} across 2^32")
    assert ref.orc.philox_step == start + 11 + (relock and fam == "nv") and ref.orc.philox_step >> 32 == 1
    _final(env, ref)


@pytest.mark.parametrize("fam", ["im", "net", "nv"])
def test_masked_reseed_keeps_counter_unmasked_restarts(gpu, oracle, monkeypatch, fam):
    """invsim_seed_range with a mask re-keys the masked envs and keeps the
    counter; an unmasked seed restarts it at 0."""
    if fam == "im":
        env, ref = _im_pair(gpu, oracle, monkeypatch, "fused", "InvManagementBacklogEnv", N, 1, {"mu": 20}, 5900)
        acts = _int_actions(N, 3)
    elif fam == "net":
        env, ref = _net_pair(gpu, oracle, monkeypatch, "fused", "custom", N, 6000)
        acts = _f32_actions(N, env.action_dim)
    else:
        env, ref, _ = _nv_pair(gpu, oracle, monkeypatch, "fused", "L5")
        acts = _f32_actions(N, 1, hi=150.0)
    _drive(env, ref, (("steps", 5),), acts, "before")
    before = ref.orc.philox_step
    mask = np.arange(N) % 4 == 1
    m = torch.from_numpy(mask.astype(np.uint8)).to(gpu)
    new = 777_000
    from invsim import _capi
    _capi.check(env._lib.invsim_seed_range(env._h, new, 0, 0, m.data_ptr(), env._stream()), env._h, "seed_range")
    ref.orc.seed(range(new, new + N), mask=mask)
    ref.rng0 = ref.orc.rng_state().copy()
    assert ref.orc.philox_step == before
    _drive(env, ref, (("steps", 4), ("rollout", 6)), acts, "after the masked seed")
    _final(env, ref)
    obs, _ = env.reset(seed=new + 5)
    ref.orc.seed(range(new + 5, new + 5 + N))
    assert ref.orc.philox_step == 0
    ref.rng0 = ref.orc.rng_state().copy()
    ref.t, ref.log = 0, []
    ref.last_obs = ref.orc.reset()
    _same(obs, ref.last_obs, "reset obs after the unmasked seed")
    _drive(env, ref, (("steps", 3),), acts, "after the unmasked seed")
    assert ref.orc.philox_step == (4 if fam == "nv" else 3)
    _final(env, ref)


@pytest.mark.parametrize("path", ["run", "fused"])
def test_stream_switches_continue_both_streams(gpu, oracle, monkeypatch, path):
    """numpy -> philox -> numpy on an integers demand that buffers a 32-bit
    half: the fast stream starts at counter 0 whatever the numpy stream drew,
    leaves the PCG64 states and the buffered half alone, and the numpy stream
    continues where it stood, half included."""
    import invsim
    n, seed, dp = N, 6100, {"low": 0, "high": 3 * 2**30}
    env = _make(monkeypatch, "im", path,
                lambda: invsim.InvManagementBacklogEnv(n, device=gpu, dist=3, dist_param=dp, record_demand=True))
    orc = oracle.OracleInvMgmt(n, dist=3, dist_param=dp)
    orc.seed(range(seed, seed + n))
    _same(env.reset(seed=seed)[0], orc.reset(), "reset obs")
    acts = _int_actions(n, 3)

    def steps(k, what):
        for j in range(k):
            a = acts()
            o, r, te, tr, info = env.step(torch.from_numpy(a).to(gpu))
            e_obs, e_rew, e_tr, e_info = orc.step(a, info=True)
            _same(info["demand"], e_info["demand"], f"{what} step {j}: demand")
            _same(o, e_obs, f"{what} step {j}: obs")
            _same(r, e_rew, f"{what} step {j}: reward")
    steps(3, "numpy")
    env.set_demand_stream("philox")
    orc.set_demand_stream("philox")
    steps(4, "philox")
    assert orc.philox_step == 4
    f = env.state_fields()
    _same(f["rng"].cpu().numpy().view(np.uint64).T, orc.rng_state(), "PCG64 rows after the fast-stream steps")
    assert int(f["philox_step"].cpu().numpy().view(np.uint64).reshape(-1)[0]) == 4
    env.set_demand_stream("numpy")
    orc.set_demand_stream("numpy")
    steps(5, "numpy again")
    env.set_demand_stream("philox")
    orc.set_demand_stream("philox")
    steps(3, "philox again")
    assert orc.philox_step == 7
    _same(env.state_fields()["rng"].cpu().numpy().view(np.uint64).T, orc.rng_state(), "PCG64 rows at the end")


@pytest.mark.parametrize("fam", ["im", "net", "nv"])
def test_graph_capture_is_refused_and_moves_nothing(gpu, oracle, monkeypatch, fam):
    """include/invsim.h: the counter is a launch parameter, so a captured
    launch would replay the same counter value; capture on the fast stream is
    refused (INVSIM_EINVAL) instead.  The refused capture of one episode cycle
    consumes no counter value: the steps after it draw what the oracle draws."""
    import invsim
    if fam == "im":
        env, ref = _im_pair(gpu, oracle, monkeypatch, "fused", "InvManagementBacklogEnv", 300, 1, {"mu": 20}, 6200)
        acts = _int_actions(300, 3)
    elif fam == "net":
        env, ref = _net_pair(gpu, oracle, monkeypatch, "fused", "default", 300, 6300)
        acts = _f32_actions(300, env.action_dim)
    else:
        env, ref, _ = _nv_pair(gpu, oracle, monkeypatch, "fused", "L5", n=300)
        acts = _f32_actions(300, 1, hi=150.0)
    _drive(env, ref, (("steps", 2),), acts, "before")
    a = torch.from_numpy(acts()).to(gpu)

    def cycle():
        for _ in range(ref.T + 1):
            env.step(a)
    with pytest.raises(invsim._capi.InvsimError, match="numpy demand stream"):
        env.capture(cycle, warmup=0)
    _drive(env, ref, (("steps", 4), ("rollout", 3)), acts, "after the refused capture")
    _final(env, ref)


# ================================================================ SAME_STEP autoreset, Newsvendor and Net
@pytest.mark.parametrize("path", ["run", "fused"])
@pytest.mark.parametrize("fam", ["nv", "net"])
def test_same_step_autoreset(gpu, oracle, monkeypatch, fam, path):
    """SAME_STEP: the done step resets in place and has one counter value.
    Newsvendor draws the new episode's five uniforms from draw stream RESET at
    the done step's own value (its demand came from stream 0 of that value), so
    the oracle is put back by one before its reset; Net draws nothing."""
    import invsim
    n = 300
    if fam == "nv":
        (L, limit, mu_max), seed = pc.NV_CASES["L2_mu14"]
        env = _make(monkeypatch, "nv", path,
                    lambda: invsim.NewsvendorEnv(n, device=gpu, lead_time=L, step_limit=limit, mu_max=mu_max,
                                                 record_demand=True, demand_stream="philox",
                                                 autoreset_mode="same_step"))
        orc = oracle.OracleNewsvendor(n, lead_time=L, step_limit=limit, mu_max=mu_max, demand_stream="philox")
        acts = _f32_actions(n, 1, hi=30.0)
    else:
        g, T = _net_graph("custom")
        limit, seed = T, 6400
        env = _make(monkeypatch, "net", path if path == "fused" else "spec",
                    lambda: invsim.NetInvMgmtMasterEnv(n, device=gpu, graph=g, num_periods=T, backlog=True,
                                                       record_demand=True, demand_stream="philox",
                                                       autoreset_mode="same_step"))
        orc = oracle.OracleNet(n, graph=g, num_periods=T, backlog=True, demand_stream="philox")
        acts = _f32_actions(n, env.action_dim)
    ref = _Ref(orc, fam, limit, range(seed, seed + n))
    _same(env.reset(seed=seed)[0], ref.obs0, "reset obs")
    steps = 2 * limit + 5
    for s in range(steps):
        a = acts()
        o, r, te, tr, info = env.step(torch.from_numpy(a).to(gpu))
        e_obs, e_rew, e_tr, e_dem, _ = ref.step(a)
        _same(r, e_rew, f"step {s}: reward")
        _same(tr, e_tr, f"step {s}: truncated")
        _same(info["demand"].reshape(e_dem.shape), e_dem, f"step {s}: demand")
        if e_tr.all():
            _same(info["final_obs"], e_obs, f"step {s}: final obs")
            if fam == "nv":
                orc.philox_step -= 1               # the reset draws at the done step's counter value
            e_obs = orc.reset()
            if fam == "nv":
                _same(env.params(), orc.params(), f"step {s}: params of the new episode")
        _same(o, e_obs, f"step {s}: obs")
    assert orc.philox_step == steps + (fam == "nv")
    _final(env, ref)
