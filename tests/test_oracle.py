"""CPU: the oracle against the reference's golden vectors and against numpy
(the third-party RNG the reference calls).  No GPU needed."""
import os

import numpy as np
import pytest

import numpy_sampler_cases as cases
from conftest import IM_GOLDENS, NET_GOLDENS, NV_GOLDENS, im_kwargs, load_golden, nv_kwargs


def _bits_equal(a, b):
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b).astype(a.dtype)
    return np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---------------------------------------------------------------- RNG
def test_rng_kat_fixture(oracle):
    fx, cfg = load_golden("rng_kat")
    for i, s in enumerate(int(x) for x in cfg["seeds"]):
        st = oracle.pcg64_init(s)
        assert (st == fx["init_state"][i]).all(), s
        raw = [oracle.lib().orc_next64(oracle._p(st)) for _ in range(16)]
        assert (np.array(raw, np.uint64) == fx["random_raw"][i]).all()
        st = oracle.pcg64_init(s)
        dbl = [oracle.lib().orc_next_double(oracle._p(st)) for _ in range(16)]
        assert _bits_equal(np.array(dbl), fx["random_double"][i])
        for j, lam in enumerate(cfg["lams"]):
            out, st = oracle.poisson_stream(s, lam, 1000)
            assert (out == fx["poisson"][i, j]).all(), (s, lam)
            assert (st[:2] == fx["poisson_end_state"][i, j]).all()
    out, _ = oracle.poisson_stream(42, 20, 100)      # reference test.py:1-11
    assert (out == fx["testpy_poisson20"]).all()


@pytest.mark.parametrize("lam", [1e-3, 0.5, 3.3, 9.999999, 10.0, 10.5, 20, 47.25, 200.0, 1234.5, 1e6])
def test_poisson_vs_numpy(oracle, lam):
    for seed in (7, 99991, 2**33 + 1):
        g = np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed)))
        exp = np.array([g.poisson(lam) for _ in range(3000)])
        out, st = oracle.poisson_stream(seed, lam, 3000)
        assert np.array_equal(out, exp)
        s = g.bit_generator.state["state"]["state"]
        assert int(st[0]) == s >> 64 and int(st[1]) == s & (2**64 - 1)


def test_seedsequence_vs_numpy(oracle):
    rng = np.random.default_rng(0)
    seeds = [0, 1, 2**32 - 1, 2**32, 2**64 - 1, 2**64, 2**96 + 5, 2**128 - 1]
    seeds += [int(x) for x in rng.integers(0, 2**63, 40)]
    for s in seeds:
        d = np.random.PCG64(np.random.SeedSequence(s)).state["state"]
        st = oracle.pcg64_init(s)
        assert int(st[0]) == d["state"] >> 64 and int(st[1]) == d["state"] & (2**64 - 1)
        assert int(st[2]) == d["inc"] >> 64 and int(st[3]) == d["inc"] & (2**64 - 1)


def test_loggam_known_values(oracle):
    import math
    for x in (1.0, 2.0, 3.0, 6.5, 7.0, 20.0, 101.0, 1e4):
        assert abs(oracle.lib().orc_loggam(x) - math.lgamma(x)) < 1e-9 * max(1, abs(math.lgamma(x)))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_numpy_sum_order(oracle, dtype):
    """numpy add.reduce order (sequential < 8, 8 accumulators <= 128, pairwise split)."""
    rng = np.random.default_rng(1)
    fn = oracle.lib().orc_sum_f32 if dtype == np.float32 else oracle.lib().orc_sum_f64
    for n in list(range(0, 40)) + [127, 128, 129, 200, 300]:
        for _ in range(20):
            a = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 8, n)).astype(dtype)
            got = fn(oracle._p(a), n)
            assert _bits_equal(np.array(got, dtype), a.sum()), n


def test_numpy_clip_semantics():
    """newsvendor.py:132 clips a Python float with np.clip -> np.float64 (NaN kept)."""
    assert np.isnan(np.clip(float("nan"), 0, 2000))
    assert np.clip(float("inf"), 0, 2000) == 2000.0
    assert np.signbit(np.clip(-0.0, 0, 2000))           # numpy keeps -0.0 (oracle/kernel do too)
    assert np.clip(-5e-324, 0, 2000) == 0.0 and not np.signbit(np.clip(-5e-324, 0, 2000))


# ---------------------------------------------------------------- envs vs goldens
def drive(env, fx, cfg):
    n, n_ep, L = cfg["n_env"], cfg["n_ep"], cfg["ep_len"]
    env.seed([cfg["base_seed"] + i for i in range(n)])
    for ep in range(n_ep):
        o = env.reset()
        assert _bits_equal(o, fx["reset_obs"][:, ep])
        for k in range(L):
            s = ep * L + k
            res = env.step(fx["actions"][:, s])
            assert _bits_equal(res[0], fx["obs"][:, s]), f"obs step {s}"
            assert _bits_equal(res[1], fx["reward"][:, s]), f"reward step {s}"
            assert np.array_equal(res[2], fx["truncated"][:, s])


@pytest.mark.parametrize("name", NV_GOLDENS)
def test_oracle_newsvendor_golden(oracle, name):
    fx, cfg = load_golden(name)
    env = oracle.OracleNewsvendor(cfg["n_env"], **nv_kwargs(cfg))
    drive(env, fx, cfg)
    assert _bits_equal(env.params(), fx["params"][:, -1])


@pytest.mark.parametrize("name", IM_GOLDENS)
def test_oracle_invmgmt_golden(oracle, name):
    fx, cfg = load_golden(name)
    env = oracle.OracleInvMgmt(cfg["n_env"], **im_kwargs(cfg))
    drive(env, fx, cfg)


def test_oracle_invmgmt_info_golden(oracle):
    fx, cfg = load_golden("invmgmt_backlog_default")
    env = oracle.OracleInvMgmt(cfg["n_env"], **im_kwargs(cfg))
    env.seed([cfg["base_seed"] + i for i in range(cfg["n_env"])])
    env.reset()
    for s in range(cfg["ep_len"]):
        _, _, _, info = env.step(fx["actions"][:, s], info=True)
        assert np.array_equal(info["demand"], fx["demand"][:, s])
        assert np.array_equal(info["sales"], fx["sales"][:, s])
        assert np.array_equal(info["unfulfilled"], fx["unfulfilled"][:, s])
        assert np.array_equal(info["ending_inventory"], fx["ending_inventory"][:, s])
        assert np.array_equal(info["backlog_next"], fx["backlog_next"][:, s])


@pytest.mark.parametrize("name", NET_GOLDENS)
def test_oracle_net_golden(oracle, name):
    fx, cfg = load_golden(name)
    g = oracle.custom_graph() if cfg["module"].endswith("custom") else oracle.default_graph()
    env = oracle.OracleNet(cfg["n_env"], graph=g, num_periods=cfg.get("num_periods", 30),
                           backlog=cfg["topology"]["backlog"], alpha=cfg.get("alpha", 1.0))
    assert env.obs_dim == cfg["topology"]["obs_dim"]
    n = cfg["n_env"]
    env.seed([cfg["base_seed"] + i for i in range(n)])
    L = cfg["ep_len"]
    for ep in range(cfg["n_ep"]):
        assert _bits_equal(env.reset(), fx["reset_obs"][:, ep])
        for k in range(L):
            s = ep * L + k
            o, r, tr, info = env.step(fx["actions"][:, s], info=True)
            assert _bits_equal(o, fx["obs"][:, s]) and _bits_equal(r, fx["reward"][:, s])
            for key in ("X", "U", "D", "R", "Y", "P"):
                if key in fx.files:
                    assert _bits_equal(info[key], fx[key][:, s]), (key, s)


def test_golden_coverage_of_quirk_branches():
    """The fixtures reach the reference's edge branches (so parity means something)."""
    fx, _ = load_golden("invmgmt_backlog_default")
    assert (fx["ending_inventory"] < 0).any(), "off-by-one supplier decrement driving I < 0"
    assert (fx["backlog_next"][:, :, 1:] > 10**11).any(), "huge requests -> huge backlog"
    fx, _ = load_golden("newsvendor_capped_L9")
    assert (fx["obs"][:, :, 5:].sum(-1) >= 550).any(), "inventory cap branch (f32 cap) reached"
    fx, _ = load_golden("newsvendor_default")
    assert np.isnan(fx["actions"]).any() and np.isinf(fx["actions"]).any()
    fx, _ = load_golden("net_master_truelost_alpha")
    assert (fx["U"] == 0).all(), "true lost sales keeps U at 0"
    fx, _ = load_golden("net_lostsales_default")
    assert (fx["U"] > 0).any(), "reference LostSales class runs backlog=True"


# ---------------------------------------------------------------- numpy demand samplers (dist 2-4)
def _npg(seed):
    return np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed)))


@pytest.mark.parametrize("seed", [0, 7, 123456])
def test_standard_exponential_vs_numpy(oracle, seed):
    a, _ = oracle.exponential_stream(seed, 100000)
    assert np.array_equal(a.view(np.uint64), _npg(seed).standard_exponential(100000).view(np.uint64))


def _same_generator(st, buf, g):
    """the oracle's PCG64 state (and, for integers, its buffered 32-bit half) is numpy's bit generator's"""
    d = g.bit_generator.state
    m = 2**64 - 1
    assert [int(x) for x in st] == [d["state"]["state"] >> 64, d["state"]["state"] & m,
                                    d["state"]["inc"] >> 64, d["state"]["inc"] & m]
    if buf is not None:
        assert (int(buf[0]), int(buf[1])) == (d["has_uint32"], d["uinteger"])


# (low, high exclusive).  Powers of two have threshold 0 and most other ranges reject with probability
# <= 2^-32, so the Lemire rejection loops run only on the ranges of the second line: 2^31 + 1 and
# 3 * 2^30 + 1 (32-bit loop, probability 1/2 and ~1/4), 2^57 + 1 and 2^63 + 1 (64-bit loop, 2^-7 and 1/2).
# The third line: rng == 0 (no draw), rng == 0xFFFFFFFF (a raw 32-bit draw), the widest int64 range,
# and rng + 1 == 2^31, where every even draw has leftover == threshold == 0 (accepted).
@pytest.mark.parametrize("lo,hi", [(0, 11), (5, 300), (-50, 50), (0, 2**32), (0, 2**32 + 1), (0, 2**40),
                                   (-2**62, 2**62), (3, 4), (0, 41), (-5, 2**40 + 1),
                                   (0, 2**31 + 1), (0, 3 * 2**30 + 1), (0, 2**57 + 1), (-2**62, 2**62 + 1),
                                   (5, 6), (7, 8), (0, 2**32 - 1), (-3, 2**63 - 1), (0, 2**31)])
def test_integers_vs_numpy(oracle, lo, hi):
    a, st, buf = oracle.dist_stream(3, 3, 20001, lo, hi)
    g = _npg(3)
    assert np.array_equal(a, np.array([g.integers(lo, hi) for _ in range(20001)]))
    _same_generator(st, buf, g)


@pytest.mark.parametrize("n,p", [(10, 0.5), (100, 0.2), (100, 0.35), (1000, 0.5), (20, 0.9), (1000, 0.97),
                                 (50, 0.01), (5000, 0.3), (7, 1.0), (0, 0.3), (40, 0.0),
                                 (1000, 0.3), (300, 0.8), (400, 0.05), (100000, 0.5)])
def test_binomial_vs_numpy(oracle, n, p):
    a, st, _ = oracle.dist_stream(11, 2, 20000, n, 0, p)
    g = _npg(11)
    assert np.array_equal(a, np.array([g.binomial(n, p) for _ in range(20000)]))
    _same_generator(st, None, g)


@pytest.mark.parametrize("p", [1.0, 0.5, 0.34, 1 / 3, 0.3333333333333333, float(np.nextafter(1 / 3, 0)), 0.2, 0.05,
                               0.001, 1e-4, 1e-9, 1e-300])
def test_geometric_vs_numpy(oracle, p):
    a, st, _ = oracle.dist_stream(5, 4, 20000, 0, 0, p)
    g = _npg(5)
    assert np.array_equal(a, np.array([g.geometric(p) for _ in range(20000)]))
    _same_generator(st, None, g)
    if p == 1e-300:
        assert (a == 2**63 - 1).all()                  # the clamp, every draw


def test_no_draw_parameters_in_numpy_itself():
    """What the GPU cases marked no_draw rest on, from numpy directly:
    integers(7, 8), binomial(0, p) and binomial(n, 0.0) return without touching
    the bit generator; binomial(7, 1.0) does NOT (it flips to q = 0 and draws
    the inversion's one uniform), though it always returns 7."""
    for c in cases.CASES:
        if not (c.get("no_draw") or "constant" in c):
            continue
        g = _npg(cases.BASE_SEED)
        before = g.bit_generator.state
        lo, hi, p = cases.oracle_args(c)
        fn = {2: lambda: g.binomial(lo, p), 3: lambda: g.integers(lo, hi), 4: lambda: g.geometric(p)}[c["dist"]]
        vals = {int(fn()) for _ in range(50)}
        if "constant" in c:
            assert vals == {c["constant"]}, c["id"]
        assert (g.bit_generator.state == before) == bool(c.get("no_draw")), c["id"]


# ---------------------------------------------------------------- branch counters and the GPU cases' coverage
@pytest.mark.parametrize("case", cases.CASES, ids=cases.CASE_IDS)
def test_counted_fill_equals_uncounted(oracle, case):
    """orc_dist_fill_counted draws what orc_dist_fill draws: values, generator
    state and buffered half, also when a stream is continued in pieces."""
    lo, hi, p = cases.oracle_args(case)
    for seed in (cases.BASE_SEED, cases.BASE_SEED + 999, 2**70 + 3):
        a, st, buf = oracle.dist_stream(seed, case["dist"], 300, lo, hi, p)
        b, st2, buf2, cnt = oracle.dist_stream_counts(seed, case["dist"], 300, lo, hi, p)
        assert np.array_equal(a, b) and np.array_equal(st, st2) and np.array_equal(buf, buf2)
        assert set(cnt) == set(oracle.COUNTERS) and all(v >= 0 for v in cnt.values())
        c1, st3, buf3, _ = oracle.dist_stream_counts(seed, case["dist"], 101, lo, hi, p)
        c2, st3, buf3, _ = oracle.dist_stream_counts(seed, case["dist"], 199, lo, hi, p, state=st3, buf=buf3)
        assert np.array_equal(np.concatenate([c1, c2]), a) and np.array_equal(st3, st) and np.array_equal(buf3, buf)
        assert cnt["zig_slow"] == cnt["zig_tail"] + cnt["zig_wedge_accept"] + cnt["zig_wedge_reject"]
        assert cnt["btpe_step52"] == cnt["btpe_quick_accept"] + cnt["btpe_quick_reject"] + cnt["btpe_four_log"]


@pytest.mark.parametrize("case", cases.CASES, ids=cases.CASE_IDS)
def test_gpu_sampler_cases_reach_their_branches(oracle, case):
    """Over exactly the streams tests/test_gpu_numpy_samplers.py compares on the
    device (seeds BASE_SEED .. BASE_SEED + N_ENV - 1, the phases' draw counts),
    every branch the case targets is taken at least FLOOR times, and the
    branches it is there to avoid are not taken at all."""
    s = cases.streams(case["id"])
    cnt = s["counts"]
    print(case["id"], s["marks"][-1], "draws/env:", {k: v for k, v in cnt.items() if v})
    for name in case["targets"]:
        assert cnt[name] >= cases.FLOOR, (case["id"], name, cnt[name])
    for name in case["never"]:
        assert cnt[name] == 0, (case["id"], name, cnt[name])
    # the inversion's restart needs X > np + 10 sqrt(npq + 1), about 10 sigma out:
    # 0 is the expected count on any feasible number of draws, and no case targets it
    assert cnt["inv_restart"] == 0
    d = s["draws"]
    if "constant" in case:
        assert (d == case["constant"]).all()
    if case.get("no_draw"):                    # the generator never moves: every mark holds the seeded state
        assert (s["states"] == s["states"][:1]).all() and (s["bufs"] == 0).all()
    if "int32_reject" in case["targets"]:      # a rejected draw shifts the buffered half: both parities are live
        assert 0 < (s["bufs"] != 0).sum() < s["bufs"].size


@pytest.mark.parametrize("id,dist,dp", cases.FAST_CASES, ids=[c[0] for c in cases.FAST_CASES])
def test_chi_square_check_passes_numpys_own_samplers(id, dist, dp):
    """The fast stream's GPU check (chi2_pmf against the exact pmf, p > P_MIN on
    FAST_ENVS x FAST_DRAWS draws) is one the reference sampler itself stays
    within: numpy's own draws, as many, at a fixed seed."""
    pytest.importorskip("scipy")
    g = np.random.Generator(np.random.PCG64(2024))
    n = cases.FAST_ENVS * cases.FAST_DRAWS
    x = {2: lambda: g.binomial(dp["n"], dp["p"], n), 3: lambda: g.integers(dp["low"], dp["high"] + 1, n),
         4: lambda: g.geometric(dp["p"], n)}[dist]()
    kmax = cases.fast_kmax(dist, dp)
    counts = np.bincount(np.minimum(x, kmax), minlength=kmax + 1)
    stat, dof, p = cases.chi2_pmf(counts, cases.exact_pmf(dist, dp, kmax))
    print(id, f"chi-square {stat:.1f} on {dof} dof, p = {p:.3g}")
    assert dof >= 30 and p > cases.P_MIN


@pytest.mark.parametrize("dist,dp", [(2, {"n": 40, "p": 0.5}), (2, {"n": 400, "p": 0.05}),
                                     (3, {"low": 0, "high": 40}), (4, {"p": 0.05}), (4, {"p": 0.5})])
def test_oracle_invmgmt_demand_stream_is_numpys(oracle, dist, dp):
    """The env draws np_random.<sampler>(...) once per step (inventory_management.py:173-182,
    :280): env i's demand sequence is numpy's sequence for seed base + i (the
    32-bit buffer of integers() carried across steps; reset without seed keeps it)."""
    n, base = 6, 321
    orc = oracle.OracleInvMgmt(n, dist=dist, dist_param=dp)
    orc.seed(range(base, base + n))
    orc.reset()
    a = np.full((n, 3), 60, np.int64)
    dem = []
    for ep in range(2):
        if ep:
            orc.reset()
        for _ in range(30):
            dem.append(orc.step(a, info=True)[3]["demand"])
    dem = np.stack(dem, 1)
    for i in range(n):
        g = _npg(base + i)
        if dist == 2:
            e = [g.binomial(dp["n"], dp["p"]) for _ in range(60)]
        elif dist == 3:
            e = [g.integers(dp["low"], dp["high"] + 1) for _ in range(60)]
        else:
            e = [g.geometric(dp["p"]) for _ in range(60)]
        assert np.array_equal(dem[i], np.maximum(np.array(e), 0)), i


@pytest.mark.parametrize("fam", ["nv", "im", "net"])
def test_oracle_thread_count_independent(oracle, fam):
    """The OpenMP env loop (bench.py's multi-core cpu_baseline) gives the same
    trajectories as the single-thread loop."""
    n, T = 301, 12
    outs = []
    for threads in (1, 4):
        oracle.set_threads(threads)
        rng = np.random.default_rng(3)
        if fam == "nv":
            env = oracle.OracleNewsvendor(n)
            acts = [rng.uniform(0, 400, size=n).astype(np.float32) for _ in range(T)]
        elif fam == "im":
            env = oracle.OracleInvMgmt(n, backlog=True)
            acts = [rng.integers(0, 231, size=(n, 3)).astype(np.int64) for _ in range(T)]
        else:
            env = oracle.OracleNet(n)
            acts = [rng.uniform(0, 200, size=(n, 11)).astype(np.float32) for _ in range(T)]
        env.seed(range(5, 5 + n))
        rec = [env.reset()]
        for a in acts:
            rec.extend(np.asarray(x).copy() for x in env.step(a)[:3])
        outs.append(rec)
    oracle.set_threads(1)
    for x, y in zip(*outs):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


@pytest.mark.parametrize("fn,dp", [("binomial", {"n": 40, "p": 0.5}), ("binomial", {"n": 400, "p": 0.05}),
                                   ("integers", {"low": 3, "high": 45}), ("integers", {"low": 25}),
                                   ("geometric", {"p": 0.05}), ("poisson", {"lam": 7.5})])
def test_oracle_net_market_samplers_vs_numpy(oracle, fn, dp):
    """A market link whose demand_dist_func calls np_random.<fn>(**dist_param)
    (network_management.py:257-263): the market draws are the only consumer of
    the env's Generator, so D[t] of env i is numpy's own <fn> stream of seed i
    through max(0, int(round(.)))."""
    from invsim.topology import custom_graph
    g = custom_graph()
    orc = None
    for e in list(g.edges()):
        if "L" not in g.edges[e]:
            g.edges[e]["dist_param"] = dict(dp)
            # the reference's lambda shape for poisson (:125), over the env itself
            # (bound below: the oracle env plays the reference's `self`), a method
            # name otherwise
            g.edges[e]["demand_dist_func"] = (lambda **p: orc.np_random.poisson(**p)) if fn == "poisson" else fn
    n, T = 16, 12
    orc = oracle.OracleNet(n, graph=g, num_periods=T)
    orc.seed(range(100, 100 + n))
    orc.reset()
    D = []
    for _ in range(T):
        _, _, _, info = orc.step(np.full((n, orc.act_dim), 30.0, np.float32), info=True)
        D.append(info["D"])
    D = np.stack(D, 1)                              # [n, T, markets]
    for i in range(n):
        gen = np.random.Generator(np.random.PCG64(np.random.SeedSequence(100 + i)))
        exp = [[max(0, int(round(getattr(gen, fn)(**dp)))) for _ in range(3)] for _ in range(T)]
        assert np.array_equal(D[i], np.array(exp, np.float64)), (fn, i)


# ---------------------------------------------------------------- the fast demand stream (Philox4x32-10)
def _random_blocks(n, seed=5):
    g = np.random.default_rng(seed)
    w = g.integers(0, 2**32, size=(n, 6), dtype=np.uint64)
    w[:8] = [[0] * 6, [2**32 - 1] * 6, [2**32 - 1, 0, 0, 0, 0, 0], [0, 2**32 - 1, 0, 0, 0, 0],
             [0, 0, 2**32 - 1, 2**32 - 1, 0, 0], [1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 2**32 - 1, 0],
             [0, 0, 0, 0, 0, 2**32 - 1]]
    return [[int(x) for x in row] for row in w]


def test_philox_block_known_answers_and_python_model(oracle):
    """The oracle's C block function == tests/philox_model.py (Python ints) on
    the Random123 known-answer inputs, whose outputs rocRAND's host ten_rounds
    printed (philox_cases.KAT), and on 10 000 random (counter, key) pairs."""
    import philox_cases
    import philox_model
    for ctr, key, exp in philox_cases.KAT:
        assert tuple(philox_model.block(ctr, key)) == exp, (ctr, key)
        assert tuple(oracle.philox_block(ctr, key)) == exp, (ctr, key)
    for w in _random_blocks(10_000):
        assert oracle.philox_block(w[:4], w[4:]) == philox_model.block(w[:4], w[4:]), w


def test_philox_block_vs_rocrand_host(oracle, tmp_path):
    """rocRAND's own philox4x32_10_engine::ten_rounds (the function the device
    stream calls), compiled for and run on the host: the known answers and 2 000
    random blocks against the oracle's block function.  No GPU."""
    import shutil
    import subprocess
    import philox_cases
    from conftest import ORACLE
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found: rocRAND's host block function cannot be built")
    if not os.path.exists(os.path.join(rocm, "include", "rocrand", "rocrand_philox4x32_10.h")):
        pytest.skip("rocrand/rocrand_philox4x32_10.h not found next to hipcc")
    exe = tmp_path / "philox_rocrand_host"
    subprocess.run([hipcc, "-O1", "--offload-host-only", "-o", str(exe), os.path.join(ORACLE, "philox_rocrand_host.cpp")],
                   check=True, capture_output=True)
    blocks = [list(c) + list(k) for c, k, _ in philox_cases.KAT] + _random_blocks(2000, seed=6)
    text = "".join(" ".join(f"{x:x}" for x in w) + "\n" for w in blocks)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    got = [[int(x, 16) for x in line.split()] for line in out if line]
    assert len(got) == len(blocks)
    for (_, _, exp), g in zip(philox_cases.KAT, got):
        assert tuple(g) == exp
    for w, g in zip(blocks, got):
        assert oracle.philox_block(w[:4], w[4:]) == g, w


def test_philox_generator_semantics(oracle):
    """The C generator against philox_model.Gen on hand-built cases: the first
    uniform of a draw is (x.y:x.x) >> 11 of block 0 of (key, step, r); the
    second output is (x.w:x.z) of the same block; the third opens block 1 (a
    PTRS rejection continues the same (step, r) sequence); sub() drops a held
    half and restarts the block index; set_step keeps neither; the step's high
    word is counter word 3 and the key's low half key word 0."""
    import philox_model
    key = 0x0123456789ABCDEF
    step = (5 << 32) | 7
    kw = (key & 0xFFFFFFFF, key >> 32)
    assert kw == (0x89ABCDEF, 0x01234567)
    b0 = philox_model.block((0, 3, 7, 5), kw)
    b1 = philox_model.block((1, 3, 7, 5), kw)
    g = oracle.PhiloxGen(key)
    g.set_step(step)
    g.sub(3)
    assert g.next_double() == ((b0[1] << 32 | b0[0]) >> 11) * 2.0 ** -53
    assert g.next64() == b0[3] << 32 | b0[2]
    assert g.next64() == b1[1] << 32 | b1[0]          # one half of block 1 is now held
    g.sub(3)
    assert g.next64() == b0[1] << 32 | b0[0], "sub() restarts at block 0 and drops the held half"
    g.sub(philox_model.RESET)
    r0 = philox_model.block((0, 0xFFFFFFFF, 7, 5), kw)
    assert g.next64() == r0[1] << 32 | r0[0]
    g.set_step(step + 2**32)                          # the step's high word moves alone
    g.sub(0)
    h0 = philox_model.block((0, 0, 7, 6), kw)
    assert g.next64() == h0[1] << 32 | h0[0]
    # a longer walk with interleaved repositioning, against the model generator
    m, g = philox_model.Gen(key), oracle.PhiloxGen(key)
    rg = np.random.default_rng(1)
    for _ in range(400):
        op = int(rg.integers(0, 6))
        if op == 0:
            s = int(rg.integers(0, 2**63)) * 2 + int(rg.integers(0, 2))
            m.set_step(s), g.set_step(s)
            r = int(rg.integers(0, 2**32))
            m.sub(r), g.sub(r)
        elif op == 1:
            r = int(rg.integers(0, 2**32))
            m.sub(r), g.sub(r)
        else:
            assert m.next64() == g.next64()
    assert m.next_double() == g.next_double()


def _model_poisson(gen, lam):
    """numpy's random_poisson on a philox_model.Gen, for lam where no PTRS log test is needed to tell
    the uniform count: the multiplication branch (lam < 10)"""
    import math
    enlam, X, prod = math.exp(-lam), 0, 1.0
    while True:
        prod *= gen.next_double()
        if prod > enlam:
            X += 1
        else:
            return X


def test_philox_env_streams_follow_the_model(oracle):
    """The env oracles on the fast stream against the Python model: InvMgmt's
    demand of launch step s is the draw of stream 0 at counter s; a Net market
    r draws from stream r; the Newsvendor reset's uniforms come from stream
    RESET of the counter's value, and the step after it uses the next one."""
    import philox_model
    n, seed = 5, 77
    keys = [oracle.philox_key(seed + i) for i in range(n)]
    im = oracle.OracleInvMgmt(n, dist_param={"mu": 4.5}, demand_stream="philox")
    im.seed(range(seed, seed + n))
    im.reset()
    im.philox_step = 2**32 - 2
    for k in range(4):
        d = im.step(np.zeros((n, 3), np.int64), info=True)[3]["demand"]
        for i in range(n):
            g = philox_model.Gen(keys[i])
            g.set_step(2**32 - 2 + k)
            g.sub(0)
            assert d[i] == _model_poisson(g, 4.5), (k, i)
    assert im.philox_step == 2**32 + 2
    nv = oracle.OracleNewsvendor(n, mu_max=9.0, demand_stream="philox")
    nv.seed(range(seed, seed + n))
    assert nv.philox_step == 0
    nv.reset()
    assert nv.philox_step == 1
    mu = nv.params()[:, 4]
    d = nv.step(np.zeros(n, np.float32))[3]
    for i in range(n):
        g = philox_model.Gen(keys[i])
        g.set_step(0)
        g.sub(philox_model.RESET)
        u = [g.next_double() for _ in range(5)]
        assert mu[i] == u[4] * 9.0
        g.set_step(1)
        g.sub(0)
        assert d[i] == _model_poisson(g, mu[i])
    from invsim.topology import custom_graph
    gr = custom_graph()
    for e in [e for e in gr.edges() if "L" not in gr.edges[e]]:
        gr.edges[e]["dist_param"] = {"lam": 6.0}
    net = oracle.OracleNet(n, graph=gr, demand_stream="philox")
    net.seed(range(seed, seed + n))
    net.reset()
    net.philox_step = 11
    D = net.step(np.zeros((n, net.act_dim), np.float32), info=True)[3]["D"]
    for i in range(n):
        for r in range(3):
            g = philox_model.Gen(keys[i])
            g.set_step(11)
            g.sub(r)
            assert D[i, r] == _model_poisson(g, 6.0), (i, r)


def test_philox_streams_are_independent(oracle):
    """Guards of the restatement against the defects it is there to catch: the
    custom graph's three Poisson(20) markets differ pairwise in more than half
    of 1 000 envs x 30 steps, and the Newsvendor reset's mu is not a function
    of the first demand's block (stream 0 of the same counter value)."""
    import philox_model
    from invsim.topology import custom_graph
    n, T = 1000, 30
    net = oracle.OracleNet(n, graph=custom_graph(), demand_stream="philox")
    net.seed(range(900, 900 + n))
    net.reset()
    a = np.zeros((n, net.act_dim), np.float32)
    D = np.stack([net.step(a, info=True)[3]["D"] for _ in range(T)])
    assert D.shape == (T, n, 3)
    for p, q in ((0, 1), (0, 2), (1, 2)):
        assert (D[..., p] != D[..., q]).mean() > 0.5, (p, q)
    assert (D[1:] != D[:-1]).mean() > 0.5, "consecutive launch steps draw from different blocks"
    nv = oracle.OracleNewsvendor(n, demand_stream="philox")
    nv.seed(range(900, 900 + n))
    nv.reset()
    mu = nv.params()[:, 4]
    hits = 0
    for i in range(n):
        b = philox_model.block((0, 0, 0, 0), (lambda k: (k & 0xFFFFFFFF, k >> 32))(oracle.philox_key(900 + i)))
        us = [((b[1] << 32 | b[0]) >> 11) * 2.0 ** -53, ((b[3] << 32 | b[2]) >> 11) * 2.0 ** -53]
        hits += any(mu[i] == u * 200.0 for u in us)
    assert hits == 0, "the reset's uniforms share the demand stream's block"


@pytest.mark.parametrize("case", list(__import__("philox_cases").IM_CASES))
def test_philox_gpu_cases_reach_their_branches(oracle, case):
    """The floors of tests/test_gpu_philox_oracle.py, on the oracle's own draws
    over exactly its seeds and launch steps: every Poisson case with lam >= 10
    has >= 100 PTRS rejections (blocks j >= 1 are drawn), every multiplication
    case >= 100 draws with an odd number of uniforms (a held half is dropped),
    the integers case runs the 32-bit path and its rejection loop, and the
    binomial / geometric ones BTPE's Step 52 and the ziggurat's slow path."""
    import philox_cases
    cnt = philox_cases.im_counts(case)
    print(case, {k: v for k, v in cnt.items() if v})
    for name in philox_cases.IM_FLOORS[case]:
        assert cnt[name] >= philox_cases.FLOOR, (case, name, cnt[name])
    if case == "int_0_3x2p30":
        assert cnt["int64_draw"] == 0


def test_philox_newsvendor_case_reaches_both_branches(oracle):
    """The (L 2, limit 12, mu_max 14) Newsvendor case of the GPU test: over its
    seeds, at least 100 episodes on each Poisson branch already at the first
    reset (mu < 10: multiplication, mu >= 10: PTRS)."""
    import philox_cases
    (L, limit, mu_max), seed = philox_cases.NV_CASES["L2_mu14"]
    n = philox_cases.N_ENV
    nv = oracle.OracleNewsvendor(n, lead_time=L, step_limit=limit, mu_max=mu_max, demand_stream="philox")
    nv.seed(range(seed, seed + n))
    nv.reset()
    mu = nv.params()[:, 4]
    print("episodes with mu < 10:", int((mu < 10).sum()), " mu >= 10:", int((mu >= 10).sum()))
    assert (mu < 10).sum() >= philox_cases.FLOOR and (mu >= 10).sum() >= philox_cases.FLOOR


def test_numpy_stream_untouched_by_stream_api(oracle):
    """set_demand_stream("philox") steps leave the PCG64 states alone, and a
    handle switched back continues numpy's stream where it stood."""
    n = 50
    a = np.full((n, 3), 7, np.int64)
    x = oracle.OracleInvMgmt(n, dist=3, dist_param={"low": 0, "high": 3 * 2**30})
    y = oracle.OracleInvMgmt(n, dist=3, dist_param={"low": 0, "high": 3 * 2**30})
    for o in (x, y):
        o.seed(range(3, 3 + n))
        o.reset()
    for _ in range(3):
        x.step(a), y.step(a)
    st = x.rng_state().copy()
    x.set_demand_stream("philox")
    for _ in range(4):
        x.step(a)
    assert np.array_equal(x.rng_state(), st) and x.philox_step == 4
    x.set_demand_stream("numpy")
    for _ in range(5):
        ox, oy = x.step(a, info=True), y.step(a, info=True)
        assert np.array_equal(ox[3]["demand"], oy[3]["demand"])
    assert np.array_equal(x.rng_state(), y.rng_state())


@pytest.mark.parametrize("graph,markets", [("default", 1), ("custom", 3)])
def test_philox_net_cases_reach_ptrs_rejections(oracle, graph, markets):
    """The Net cases of the GPU test (Poisson(20) markets, draw stream r per
    market): at least 100 PTRS rejections on every stream over its seeds and
    the 78 launch steps of the step + rollout drive."""
    import philox_cases
    seed = philox_cases.NET_SEED[graph]
    for r in range(markets):
        rej = 0
        for i in range(philox_cases.N_ENV):
            _, cnt = oracle.philox_stream_counts(seed + i, 1, philox_cases.IM_STEPS, 0, r, p=20.0)
            rej += cnt["pois_ptrs_reject"]
        print(graph, "stream", r, "PTRS rejections:", rej)
        assert rej >= philox_cases.FLOOR
