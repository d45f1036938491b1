"""The numpy demand samplers (dist 2-4: binomial, integers, geometric;
csrc/numpy_dists.hpp) on every sampler branch and every kernel path that runs
them, against the CPU oracle, whose samplers are pinned draw for draw against
numpy itself (tests/test_oracle.py).

1. Sampler-branch parity (test_sampler_branches_*): the checker is the sampler
   alone, pyoracle.dist_stream on the env's seeds.  The cases and what each one
   targets are tests/numpy_sampler_cases.py; tests/test_oracle.py asserts, with
   the oracle's branch counters over exactly these seeds and draw counts, that
   every targeted branch is taken (both Lemire rejection loops, every BTPE
   region, the F product and Step 52 with its four-log test, the flipped and the
   degenerate binomials, the ziggurat's slow path, tail and wedge, the
   geometric search and the INT64_MAX clamp).  Demands after every step, and
   the generator state AND the buffered 32-bit half (state_fields "rng" /
   "u32buf") after every phase, with and without the demand lookahead.
2. Kernel-path parity (test_*_vs_oracle): the env oracles (OracleInvMgmt /
   OracleNet) on obs, reward bits and flags at every step, for the
   instantiations of NPD = true no other test compares with an oracle:
   LostSales, M1 != 3, same-step autoreset, the EARLY stores instantiation
   (N > 32 768), im_run_kernel under rollouts and under the in-kernel and
   caller-supplied policies, and the generic Net kernel with a rejecting
   integers market in front of another market.
3. The buffered half across a checkpoint taken while the lookahead cache is live.
4. The fast stream (demand_stream="philox"): a chi-square of 2e6 draws
   against the exact pmf; tests/test_oracle.py passes numpy's own samplers
   through the same function.  (Its draws are compared bit for bit with the
   oracle's restatement of the stream in tests/test_gpu_philox_oracle.py.)
"""
import numpy as np
import pytest
import torch

import numpy_sampler_cases as cases
import random_agent_model as model
from conftest import knob_envs

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- helpers
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32, 1: np.uint8}[a.dtype.itemsize])


def _same_np(t, exp, what):
    got = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    exp = np.asarray(exp)
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, got.dtype, exp.shape, exp.dtype)
    eq = _bits(got) == _bits(exp)
    if not eq.all():
        bad = np.argwhere(~eq)
        pytest.fail(f"{what}: {len(bad)} of {eq.size} differ, first at {bad[0].tolist()}: "
                    f"got {got[tuple(bad[0])]!r}, expected {exp[tuple(bad[0])]!r}")


def _generator_state(env, blob=None):
    """(PCG64 rows uint64 [N, 4] as the oracle keeps them, buffered halves int64 [N])"""
    f = env.state_fields(blob)
    return f["rng"].cpu().numpy().view(np.uint64).T, f["u32buf"].cpu().numpy()[0]


def _compare_state(env, states, bufs, what):
    """every env's generator state and buffered half, as test_gpu_long_draws._compare reports them"""
    rng_gpu, u32_gpu = _generator_state(env)
    bad = np.nonzero((rng_gpu != states).any(axis=1))[0]
    assert bad.size == 0, f"{what}: {bad.size} streams in a different PCG64 state (first env {bad[:5]})"
    bad = np.nonzero(u32_gpu != bufs)[0]
    assert bad.size == 0, (f"{what}: {bad.size} envs hold a different buffered half (first env {bad[:5]}: "
                           f"{[hex(int(x)) for x in u32_gpu[bad[:5]]]}, expected "
                           f"{[hex(int(x)) for x in bufs[bad[:5]]]})")


# ================================================================ 1. sampler branches
@pytest.mark.parametrize("ahead", [None, "0"], ids=["lookahead", "ahead0"])
@pytest.mark.parametrize("case", cases.CASES, ids=cases.CASE_IDS)
def test_sampler_branches_vs_oracle_streams(gpu, oracle, monkeypatch, case, ahead):
    """Env i's demands are max(draw, 0) of numpy's stream of seed BASE_SEED + i,
    through split steps (the first draws inline, the rest read the lookahead
    slot), one im_run_kernel rollout with the NEXT_STEP reset call inside it,
    and more split steps; after every phase the committed generator state and
    the buffered 32-bit half are the oracle's at that draw count."""
    from invsim import InvManagementBacklogEnv
    n, ref = cases.N_ENV, cases.streams(case["id"])
    env, = knob_envs(monkeypatch, "INVSIM_IM_AHEAD", [ahead],
                     lambda: InvManagementBacklogEnv(n, device=gpu, dist=case["dist"], dist_param=case["dist_param"],
                                                     record_demand=True))
    env.reset(seed=cases.BASE_SEED)
    g = np.random.default_rng(7)
    acts = lambda *lead: torch.from_numpy(g.integers(0, 120, size=lead + (n, 3))).to(gpu)  # noqa: E731
    draws = np.maximum(ref["draws"], 0)
    for k, ((kind, _), calls) in enumerate(zip(case["phases"], cases.call_plan(case["phases"]))):
        if kind == "steps":
            for idx in calls:
                d = env.step(acts())[4]["demand"]
                if idx is not None:                       # (the NEXT_STEP reset call draws nothing)
                    _same_np(d, draws[:, idx], f"{case['id']}: demand of draw {idx} (phase {k})")
        else:
            env.rollout(acts(len(calls)))
        _compare_state(env, ref["states"][k], ref["bufs"][k], f"{case['id']} after phase {k} ({ref['marks'][k]} draws)")


# ================================================================ 2. kernel paths
PARAMS = {"binomial": (2, {"n": 1000, "p": 0.3}),
          "integers": (3, {"low": 0, "high": 3 * 2**30}),          # the 32-bit rejection loop runs
          "geometric": (4, {"p": 0.05})}
PARAM_IDS = list(PARAMS)
# the mean demand, for BaseStockAgent (which reads dist_param["mu"] as the reference's agent does)
MEAN = {"binomial": 300, "integers": 3 * 2**29, "geometric": 20}

_TWO_STAGE = dict(I0=(60,), p=14, r=(10, 6), k=(0.2, 0.1), h=(0.1,), c=(90,), L=(4,))
_FIVE_STAGE = dict(I0=(10, 20, 30, 40), r=(15, 10, 7, 5, 3), k=(0.1, 0.08, 0.06, 0.04, 0.02),
                   h=(0.15, 0.1, 0.05, 0.03), c=(100, 200, 230, 250), L=(2, 0, 4, 1))    # one stage with L = 0


class _NextStep:
    """An oracle env under NEXT_STEP autoreset: the call after the horizon is
    the reset (reset obs, reward 0, no flag, the action ignored, no draw)."""

    def __init__(self, orc, periods, seed):
        self.orc, self.periods, self.t = orc, periods, 0
        orc.seed(range(seed, seed + orc.n))
        self.obs0 = orc.reset()

    def call(self, a):
        """(obs, reward, truncated, info or None)"""
        if self.t == self.periods:
            self.t = 0
            return self.orc.reset(), np.zeros(self.orc.n), np.zeros(self.orc.n, bool), None
        self.t += 1
        return self.orc.step(a, info=True)

    def check(self, o, r, te, tr, a, what, demand=None):
        e_obs, e_rew, e_tr, e_info = self.call(a)
        _same_np(o, e_obs, f"{what}: obs")
        _same_np(r, e_rew, f"{what}: reward")
        _same_np(tr, e_tr, f"{what}: truncated")
        assert not bool(torch.as_tensor(te).any()), f"{what}: terminated"
        if demand is not None and e_info is not None:
            key = "demand" if "demand" in e_info else "D"
            _same_np(demand.reshape(e_info[key].shape), e_info[key].astype(np.int64), f"{what}: demand")


def _drive(env, ref, phases, gen_actions, what):
    """phases of ("steps", k) / ("rollout", K) on the device env against ref, every call checked"""
    call = 0
    for kind, k in phases:
        if kind == "steps":
            for _ in range(k):
                a = gen_actions()
                o, r, te, tr, info = env.step(torch.from_numpy(a).to(env.device))
                ref.check(o, r, te, tr, a, f"{what} call {call} (step)", info.get("demand"))
                call += 1
        else:
            A = np.stack([gen_actions() for _ in range(k)])
            o, r, te, tr = env.rollout(torch.from_numpy(A).to(env.device))
            for j in range(k):
                ref.check(o[j], r[j], te[j], tr[j], A[j], f"{what} call {call} (rollout row {j})")
                call += 1


def _im_pair(gpu, oracle, cls, n, param, seed, **kw):
    import invsim
    dist, dp = PARAMS[param]
    env = getattr(invsim, cls)(n, device=gpu, dist=dist, dist_param=dict(dp), record_demand=True, **kw)
    okw = {k: v for k, v in kw.items() if k != "autoreset_mode"}
    orc = oracle.OracleInvMgmt(n, backlog=cls.endswith("BacklogEnv"), dist=dist, dist_param=dict(dp), **okw)
    ref = _NextStep(orc, env.num_periods, seed)
    obs, _ = env.reset(seed=seed)
    _same_np(obs, ref.obs0, "reset obs")
    return env, ref


def _int_actions(n, a_dim, seed=2):
    g = np.random.default_rng(seed)
    return lambda: g.integers(0, 120, size=(n, a_dim))


@pytest.mark.parametrize("param", PARAM_IDS)
def test_lostsales_steps_rollout_steps_vs_oracle(gpu, oracle, param):
    """LostSales, M1 = 3: a whole episode of split steps and the reset call, a
    31-row rollout (im_run_kernel: it commits the lookahead cache itself, no
    state read in between) and split steps again."""
    n = 1000
    env, ref = _im_pair(gpu, oracle, "InvManagementLostSalesEnv", n, param, 140)
    _drive(env, ref, (("steps", 31), ("rollout", 31), ("steps", 10)), _int_actions(n, 3), param)
    rng_gpu, _ = _generator_state(env)
    assert np.array_equal(rng_gpu, ref.orc.rng_state())


@pytest.mark.parametrize("chain", ["two_stage", "five_stage"])
@pytest.mark.parametrize("param", PARAM_IDS)
def test_backlog_other_stage_counts_vs_oracle(gpu, oracle, param, chain):
    """M1 = 1 and M1 = 4 (one stage with lead time 0): im_split_kernel's and
    im_run_kernel's instantiations for other stage counts than 3."""
    n = 300
    kw = _TWO_STAGE if chain == "two_stage" else _FIVE_STAGE
    env, ref = _im_pair(gpu, oracle, "InvManagementBacklogEnv", n, param, 150, **kw)
    _drive(env, ref, (("steps", 35), ("rollout", 10)), _int_actions(n, len(kw["L"])), f"{param}/{chain}")
    rng_gpu, _ = _generator_state(env)
    assert np.array_equal(rng_gpu, ref.orc.rng_state())


@pytest.mark.parametrize("param", PARAM_IDS)
def test_same_step_autoreset_vs_oracle(gpu, oracle, param):
    """SAME_STEP autoreset: the done step leaves the split path; two episode
    ends in 65 steps.  The terminal obs is info["final_obs"], the returned obs
    the reset one."""
    n = 300
    env, ref = _im_pair(gpu, oracle, "InvManagementBacklogEnv", n, param, 160, autoreset_mode="same_step")
    orc, acts = ref.orc, _int_actions(n, 3)
    for s in range(65):
        a = acts()
        o, r, te, tr, info = env.step(torch.from_numpy(a).to(gpu))
        e_obs, e_rew, e_tr, e_info = orc.step(a, info=True)
        _same_np(r, e_rew, f"{param} step {s}: reward")
        _same_np(tr, e_tr, f"{param} step {s}: truncated")
        _same_np(info["demand"], e_info["demand"], f"{param} step {s}: demand")
        assert not bool(te.any())
        if e_tr.all():
            _same_np(info["final_obs"], e_obs, f"{param} step {s}: final obs")
            e_obs = orc.reset()
        else:
            assert not e_tr.any()
        _same_np(o, e_obs, f"{param} step {s}: obs")
    rng_gpu, _ = _generator_state(env)
    assert np.array_equal(rng_gpu, orc.rng_state())


@pytest.mark.parametrize("param", PARAM_IDS)
def test_early_stores_instantiation_vs_oracle(gpu, oracle, param):
    """N > IM_EARLY_STORES_MIN_N (32 768): after the inline first step the
    lookahead steps run im_split_kernel<.., NPD = true, .., EARLY = true>; a
    3-row rollout then commits the cache.  32 897 envs: a partial last
    lookahead workgroup (128 envs each) and a partial last step workgroup."""
    n = 32768 + 129
    env, ref = _im_pair(gpu, oracle, "InvManagementBacklogEnv", n, param, 170)
    _drive(env, ref, (("steps", 8), ("rollout", 3)), _int_actions(n, 3), param)
    rng_gpu, u32 = _generator_state(env)
    assert np.array_equal(rng_gpu, ref.orc.rng_state())
    if param == "integers":
        assert 0 < (u32 != 0).sum() < n          # rejections shifted the half's parity env by env


ASEED = 77


@pytest.mark.parametrize("agent", ["constant", "random", "external", "base_stock"])
@pytest.mark.parametrize("param", PARAM_IDS)
def test_policies_on_run_kernel_vs_oracle(gpu, oracle, param, agent):
    """im_run_kernel<NPD = true> under the policies: ConstantOrderAgent and
    BaseStockAgent (the policy form), RandomAgent (the RANDOM translation
    unit) and caller-supplied actions through rollout_metrics (the EXTERNAL
    one), K = 31: a whole episode and its NEXT_STEP reset row.  Actions, obs,
    reward bits, flags and the evaluate_agent sums against oracle/agents.py and
    tests/random_agent_model.py over the env oracle.

    BaseStockAgent takes the mean demand from dist_param["mu"], as the
    reference's agent does (env.dist_param.get('mu', 10)); the non-Poisson
    samplers ignore that key, so the mean is handed over there, explicitly."""
    import agents
    import invsim
    n, K, T = 1000, 31, 30
    dist, dp = PARAMS[param]
    dp = dict(dp, mu=MEAN[param]) if agent == "base_stock" else dict(dp)
    env = invsim.InvManagementBacklogEnv(n, device=gpu, dist=dist, dist_param=dp)
    orc = oracle.OracleInvMgmt(n, dist=dist, dist_param=dp)
    orc.seed(range(180, 180 + n))
    o0 = orc.reset()
    obs, _ = env.reset(seed=180)
    _same_np(obs, o0, "reset obs")
    met = torch.zeros((n, invsim.policies.metrics_dim(env)), dtype=torch.float64, device=gpu)
    if agent == "external":
        exp = np.random.default_rng(3).integers(0, 120, size=(K, n, 3))
        out = env.rollout_metrics(torch.from_numpy(exp).to(gpu), metrics=met)
    else:
        ag = {"constant": invsim.ConstantOrderAgent(0.1), "random": invsim.RandomAgent(seed=ASEED),
              "base_stock": invsim.BaseStockAgent(1.1)}[agent]
        out = env.rollout_policy(ag, K, obs=True, actions=True, metrics=met)
        if agent == "constant":
            exp = np.broadcast_to(ag.action(env), (K, n, 3)).copy()
        elif agent == "random":
            exp, _ = model.expected_actions(ASEED, 0, n, K, env._action_high(), np.int64)
    if agent == "base_stock":
        exp, e_rew, e_obs, sums = agents.run_invmgmt(orc, o0, T, env.lead_time, MEAN[param], 1.1, env.supply_capacity)
    else:
        sums, e_rew, e_obs = model.sums_invmgmt(orc, exp[:T])
    if "actions" in out:       # (the env ignores the reset row's action; only RandomAgent's model defines it)
        rows = K if agent == "random" else T
        _same_np(out["actions"][:rows], exp[:rows], "actions")
    _same_np(out["obs"][:T], e_obs, "obs")
    _same_np(out["reward"][:T], e_rew, "reward")
    _same_np(out["obs"][T], orc.reset(), "the reset row's obs")
    assert bool((out["reward"][T] == 0).all()), "the reset row's reward"
    tr = out["truncated"].cpu().numpy()
    assert tr[T - 1].all() and not tr[:T - 1].any() and not tr[T].any() and not bool(out["terminated"].any())
    _same_np(met, sums, "metrics (the reset row adds nothing)")
    assert np.array_equal(_generator_state(env)[0], orc.rng_state())


def _sampler_graph():
    """The custom graph with market samplers integers [0, 2^31] (rejects every
    other draw, so the half it leaves buffered, or not, is the next market's
    first 32 bits), geometric and integers [2, 41]."""
    from invsim.topology import custom_graph
    g = custom_graph()
    markets = [e for e in g.edges() if "L" not in g.edges[e]]
    assert len(markets) == 3
    for e, (fn, dp) in zip(markets, [("integers", {"low": 0, "high": 2**31 + 1}), ("geometric", {"p": 0.07}),
                                     ("integers", {"low": 2, "high": 42})]):     # numpy's exclusive high
        g.edges[e]["demand_dist_func"] = fn
        g.edges[e]["dist_param"] = dp
    return g


def test_net_lostsales_generic_kernel_vs_oracle(gpu, oracle):
    """NetInvMgmtLostSalesEnv on the generic kernel (netinvmgmt.hip): steps
    across the reset call, a 20-row rollout and a RandomAgent policy rollout of
    31 (its own reset row inside)."""
    import invsim
    n, seed = 1000, 190
    g = _sampler_graph()
    env = invsim.NetInvMgmtLostSalesEnv(n, device=gpu, graph=g, record_demand=True)
    assert env.kernel_variant == 0
    ref = _NextStep(oracle.OracleNet(n, graph=g, backlog=env.backlog), env.num_periods, seed)
    obs, _ = env.reset(seed=seed)
    _same_np(obs, ref.obs0, "reset obs")
    rg = np.random.default_rng(4)
    acts = lambda: rg.uniform(0, 60, size=(n, env.action_dim)).astype(np.float32)  # noqa: E731
    _drive(env, ref, (("steps", 31), ("rollout", 20)), acts, "net")
    K = 31
    out = env.rollout_policy(invsim.RandomAgent(seed=ASEED), K, obs=True, actions=True)
    exp, _ = model.expected_actions(ASEED, 0, n, K, env._action_high(), np.float32)
    _same_np(out["actions"], exp, "RandomAgent actions")
    for k in range(K):
        ref.check(out["obs"][k], out["reward"][k], out["terminated"][k], out["truncated"][k], exp[k],
                  f"net policy row {k}")
    rng_gpu, u32 = _generator_state(env)
    assert np.array_equal(rng_gpu, ref.orc.rng_state())
    assert 0 < (u32 != 0).sum() < n


# ================================================================ 3. checkpoint carry
def test_rejecting_integers_buffer_survives_checkpoint(gpu, oracle):
    """test_invmgmt_integers_buffer_is_state on a range that rejects
    (integers(0, 2^31 + 1)), the checkpoint taken after an odd number of steps
    while the lookahead cache is live: get_state commits the cache (the blob
    holds the oracle's state and half after 7 draws, not after 8), and a fresh
    env loaded from it continues bit-identically, steps and a rollout; a
    re-seed clears the half."""
    from invsim import InvManagementBacklogEnv
    n, seed, lo, hi = 300, 5, 0, 2**31
    mk = lambda: InvManagementBacklogEnv(n, device=gpu, dist=3, dist_param={"low": lo, "high": hi},  # noqa: E731
                                         record_demand=True)
    e1, e2 = mk(), mk()
    e1.reset(seed=seed)
    g = torch.Generator(device=gpu).manual_seed(1)
    A = torch.randint(0, 120, (40, n, 3), device=gpu, dtype=torch.int64, generator=g)
    for k in range(7):
        e1.step(A[k])
    ck = e1.get_state().clone()
    streams = [oracle.dist_stream(seed + i, 3, 7, lo, hi + 1) for i in range(n)]
    rng_ck, u32_ck = _generator_state(e1, ck)
    assert np.array_equal(rng_ck, np.stack([s[1] for s in streams])), "the blob's generators: 7 draws, cache committed"
    assert np.array_equal(u32_ck, np.array([cases.u32_word(s[2]) for s in streams])), "the blob's buffered halves"
    assert 0 < (u32_ck != 0).sum() < n
    e2.set_state(ck)
    full = np.stack([oracle.dist_stream(seed + i, 3, 17, lo, hi + 1)[0] for i in range(n)])
    for k in range(7, 17):
        r1, r2 = e1.step(A[k]), e2.step(A[k])
        for x, y in zip(r1[:4], r2[:4]):
            assert torch.equal(x, y), k
        assert torch.equal(r1[4]["demand"], r2[4]["demand"]), k
        _same_np(r1[4]["demand"], full[:, k], f"demand of draw {k}")
    o1, o2 = e1.rollout(A[17:33]), e2.rollout(A[17:33])      # crosses the horizon and its reset call
    assert all(torch.equal(x, y) for x, y in zip(o1, o2))
    assert torch.equal(e1.get_state(), e2.get_state())
    e1.reset(seed=seed)
    e3 = mk()
    e3.reset(seed=seed)
    assert torch.equal(e1.step(A[0])[4]["demand"], e3.step(A[0])[4]["demand"])
    _same_np(e1._demand[:, 0], full[:, 0], "a re-seed restarts the stream with no half buffered")


# ================================================================ 4. the fast stream
@pytest.mark.parametrize("mode", ["steps", "rollout"])
@pytest.mark.parametrize("id,dist,dp", cases.FAST_CASES, ids=[c[0] for c in cases.FAST_CASES])
def test_fast_stream_distribution(gpu, id, dist, dp, mode):
    """demand_stream="philox" with the numpy samplers: 20 000 envs x 100 draws
    against the exact pmf (chi-square, bins pooled to an expected count >= 5,
    p > 1e-4), through split steps and through one im_run_kernel rollout.

    A two-stage chain with 10^6 units on hand, no orders and a 100-period
    horizon: the retailer never runs out, so a rollout's demands are its
    on-hand differences, row by row (checked against the recorded demand where
    there is one: every step, and the rollout's last row)."""
    import invsim
    n, K = cases.FAST_ENVS, cases.FAST_DRAWS
    env = invsim.InvManagementBacklogEnv(n, device=gpu, dist=dist, dist_param=dict(dp), demand_stream="philox",
                                         record_demand=True, periods=K, I0=(10**6,), p=14, r=(10, 6), k=(0.2, 0.1),
                                         h=(0.1,), c=(90,), L=(1,))
    obs0, _ = env.reset(seed=11 if mode == "steps" else 11 + 10**6)     # (env i draws under seed + i: disjoint samples)
    kmax = cases.fast_kmax(dist, dp)
    if mode == "steps":
        a = torch.zeros((n, 1), dtype=torch.int64, device=gpu)
        prev, ds = obs0[:, 0].clone(), []
        for _ in range(K):
            o, _, _, _, info = env.step(a)
            assert torch.equal(prev - o[:, 0], info["demand"])
            prev = o[:, 0].clone()
            ds.append(info["demand"].clone())
        d = torch.stack(ds)
    else:
        o, _, _, tr = env.rollout(torch.zeros((K, n, 1), dtype=torch.int64, device=gpu))
        on_hand = torch.cat([obs0[None, :, 0], o[:, :, 0]])
        d = on_hand[:-1] - on_hand[1:]
        assert torch.equal(d[-1], env._demand[:, 0]) and bool(tr[-1].all()) and not bool(tr[:-1].any())
    assert d.shape == (K, n) and bool((d >= 0).all()) and bool((o[..., 0] > 0).all())
    counts = torch.bincount(d.flatten().clamp(max=kmax), minlength=kmax + 1).cpu().numpy()
    stat, dof, p = cases.chi2_pmf(counts, cases.exact_pmf(dist, dp, kmax))
    print(f"{id}/{mode}: chi-square {stat:.1f} on {dof} dof, p = {p:.3g}")
    assert p > cases.P_MIN, f"chi-square {stat:.1f} on {dof} dof, p = {p:.2e}"
