"""The case table of the numpy demand samplers' branch tests (dist 2-4:
csrc/numpy_dists.hpp on the device, oracle/oracle.c on the CPU), shared by

* tests/test_oracle.py: the oracle against numpy itself on these parameters,
  and the COVERAGE test: over exactly the seeds and draw counts of the GPU test,
  every branch a case is listed as targeting is taken at least FLOOR times
  (the oracle's branch counters, pyoracle.dist_stream_counts);
* tests/test_gpu_numpy_samplers.py: the device against the oracle's streams.

So a parity result on the GPU is a statement about the branches named here,
not about whichever ones the seeds happened to reach.

A case: id, dist, dist_param (the env's: integers `high` INCLUSIVE, as
inventory_management.py:178 draws integers(low, high + 1)), the counters it
targets, and optionally `phases` (default PHASES) and `never` (counters that
must stay 0: the case is there for the other path).
"""
import functools

import numpy as np

N_ENV = 1000          # not a multiple of 64 or 128: padded lanes in the last workgroup
BASE_SEED = 40        # env i draws numpy's stream of seed BASE_SEED + i
PERIODS = 30          # the env's default horizon: call 31 of an episode is the NEXT_STEP reset, which draws nothing
FLOOR = 10            # hits of every targeted branch over a case's streams
# 20 split steps (the first draws inline, the rest hit the lookahead cache), one
# 15-row rollout (im_run_kernel; commits the cache; its row 10 is the reset
# call), 20 more split steps
PHASES = (("steps", 20), ("rollout", 15), ("steps", 20))

_BTPE_REGIONS = ("btpe_triangle", "btpe_parallelogram", "btpe_left_tail", "btpe_right_tail")
_STEP52 = ("btpe_step52", "btpe_quick_accept", "btpe_quick_reject", "btpe_four_log", "btpe_four_log_reject")


def _case(id, dist, dp, targets, **kw):
    return dict(id=id, dist=dist, dist_param=dp, targets=tuple(targets), phases=kw.pop("phases", PHASES),
                never=tuple(kw.pop("never", ())), **kw)


CASES = [
    # ---- dist 3: integers(low, high + 1)
    _case("int_0_2p31", 3, {"low": 0, "high": 2**31}, ["int32_reject"]),            # rejects with probability 1/2
    _case("int_0_3x2p30", 3, {"low": 0, "high": 3 * 2**30}, ["int32_reject"]),
    _case("int_0_2p57", 3, {"low": 0, "high": 2**57}, ["int64_reject"]),            # rejects with probability 2^-7
    _case("int_m5_2p40", 3, {"low": -5, "high": 2**40}, ["int64_draw"], never=["int32_draw"]),
    _case("int_full32", 3, {"low": 0, "high": 2**32 - 1}, ["int_full32"]),          # rng == 0xFFFFFFFF
    _case("int_const", 3, {"low": 7, "high": 7}, ["int_const"], no_draw=True),      # rng == 0
    _case("int_0_40", 3, {"low": 0, "high": 40}, ["int32_draw"], never=["int32_reject"]),
    # rng + 1 = 2^31: threshold 0 and leftover 0 for every even 32-bit draw, so half the draws sit exactly
    # on the rejection test's boundary (leftover == threshold accepts); on the other ranges here that
    # equality has probability ~2^-32 a draw, so only this case tells `<` from `<=`
    _case("int_0_2p31m1", 3, {"low": 0, "high": 2**31 - 1}, ["int32_draw"], never=["int32_reject"]),
    # ---- dist 2: binomial(n, p)
    _case("bin_1000_.3", 2, {"n": 1000, "p": 0.3}, _BTPE_REGIONS + ("btpe_fproduct", "btpe_fproduct_reject") + _STEP52),
    _case("bin_100_.35", 2, {"n": 100, "p": 0.35}, _BTPE_REGIONS + ("btpe_fproduct", "btpe_fproduct_reject"),
          never=["btpe_step52"]),                                                   # n r q / 2 - 1 < 20: F product only
    _case("bin_300_.8", 2, {"n": 300, "p": 0.8}, ("binom_flip",) + _BTPE_REGIONS + ("btpe_fproduct",)),
    _case("bin_20_.9", 2, {"n": 20, "p": 0.9}, ["binom_flip", "binom_inversion"]),
    _case("bin_400_.05", 2, {"n": 400, "p": 0.05}, ["binom_inversion"], never=["binom_flip"]),
    # p == 1: numpy flips to q = 0 and runs the inversion (qn = 1: one uniform per draw, X = 0), always n
    _case("bin_7_1", 2, {"n": 7, "p": 1.0}, ["binom_flip", "binom_inversion"], constant=7),
    _case("bin_0_.3", 2, {"n": 0, "p": 0.3}, ["binom_zero"], no_draw=True, constant=0),
    _case("bin_40_0", 2, {"n": 40, "p": 0.0}, ["binom_zero"], no_draw=True, constant=0),
    # ---- dist 4: geometric(p)
    _case("geo_.05", 4, {"p": 0.05}, ["geom_inversion", "zig_slow", "zig_tail", "zig_wedge_accept", "zig_wedge_reject"]),
    _case("geo_.5", 4, {"p": 0.5}, ["geom_search"], never=["geom_inversion"]),
    _case("geo_1/3", 4, {"p": 1 / 3}, ["geom_search"], never=["geom_inversion"]),
    # the decimal literal 0.3333333333333333 is the double 1/3 itself, and so is numpy's switch constant
    # (0.333333333333333333333333): this case takes the search.  The double just BELOW the switch is the next one.
    _case("geo_.3333333333333333", 4, {"p": 0.3333333333333333}, ["geom_search"], never=["geom_inversion"]),
    _case("geo_below_1/3", 4, {"p": float(np.nextafter(1 / 3, 0))}, ["geom_inversion"], never=["geom_search"]),
    # every draw is INT64_MAX: 3 steps, and nothing downstream of that demand is looked at
    _case("geo_1e-300", 4, {"p": 1e-300}, ["geom_clamp"], phases=(("steps", 3),), constant=2**63 - 1, demand_only=True),
]
CASE_IDS = [c["id"] for c in CASES]


def oracle_args(case):
    """(n_or_low, high exclusive, p) as pyoracle.dist_stream takes them"""
    dp = case["dist_param"]
    if case["dist"] == 2:
        return int(dp["n"]), 0, float(dp["p"])
    if case["dist"] == 3:
        return int(dp["low"]), int(dp["high"]) + 1, 0.0
    return 0, 0, float(dp["p"])


def call_plan(phases, periods=PERIODS):
    """Per phase the list, per call (a step, or a rollout row), of the index of
    the draw it makes, or None for the NEXT_STEP reset call."""
    t = draws = 0
    plan = []
    for _, k in phases:
        calls = []
        for _ in range(k):
            if t == periods:
                calls.append(None)
                t = 0
            else:
                calls.append(draws)
                draws += 1
                t += 1
        plan.append(calls)
    return plan


def draws_after(phases, periods=PERIODS):
    """draws made by the end of each phase"""
    out, n = [], 0
    for calls in call_plan(phases, periods):
        n += sum(c is not None for c in calls)
        out.append(n)
    return out


def u32_word(buf):
    """the oracle's (has, value) pair as the device keeps it: has << 32 | value, 0 when empty"""
    return (1 << 32) | int(buf[1]) if buf[0] else 0


@functools.lru_cache(maxsize=None)
def streams(case_id, n_env=N_ENV, base=BASE_SEED):
    """The oracle's streams of a case, computed once and shared (read-only):
    draws int64 [n_env, D], and at the end of every phase the generator states
    uint64 [P, n_env, 4] and buffered halves int64 [P, n_env] (device encoding),
    plus the branch counters summed over all streams."""
    import pyoracle
    case = CASES[CASE_IDS.index(case_id)]
    lo, hi, p = oracle_args(case)
    marks = draws_after(case["phases"])
    draws = np.zeros((n_env, marks[-1]), np.int64)
    states = np.zeros((len(marks), n_env, 4), np.uint64)
    bufs = np.zeros((len(marks), n_env), np.int64)
    total = dict.fromkeys(pyoracle.COUNTERS, 0)
    for i in range(n_env):
        st = buf = None
        done = 0
        for k, m in enumerate(marks):
            d, st, buf, cnt = pyoracle.dist_stream_counts(base + i, case["dist"], m - done, lo, hi, p, state=st, buf=buf)
            draws[i, done:m] = d
            done = m
            states[k, i] = st
            bufs[k, i] = u32_word(buf)
            for name, v in cnt.items():
                total[name] += v
    for a in (draws, states, bufs):
        a.setflags(write=False)
    return dict(draws=draws, states=states, bufs=bufs, counts=total, marks=marks)


# ---------------------------------------------------------------- the fast stream's distribution check
FAST_ENVS, FAST_DRAWS = 20_000, 100
FAST_CASES = [   # id, dist, dist_param (env form)
    ("bin_1000_.3", 2, {"n": 1000, "p": 0.3}),
    ("int_3_37", 3, {"low": 3, "high": 37}),
    ("geo_.05", 4, {"p": 0.05}),
]
P_MIN = 1e-4          # tests/test_gpu_fast_stream.py's threshold


def exact_pmf(dist, dp, kmax):
    """pmf over 0 .. kmax of the env's demand, the last bin taking the upper tail (scipy.stats)"""
    from scipy import stats
    if dist == 2:
        rv = stats.binom(dp["n"], dp["p"])
    elif dist == 3:
        rv = stats.randint(dp["low"], dp["high"] + 1)
    else:
        rv = stats.geom(dp["p"])
    p = rv.pmf(np.arange(kmax + 1))
    p[-1] += rv.sf(kmax)
    return p


def fast_kmax(dist, dp):
    """the histogram's last bin (values above it are clamped into it)"""
    if dist == 2:
        return int(dp["n"])
    if dist == 3:
        return int(dp["high"]) + 1
    return int(60 / dp["p"])            # geometric: P(X > 60 / p) ~ e^-60


def chi2_pmf(counts, pmf, min_expected=5.0):
    """Chi-square of a histogram against an exact pmf, bins pooled left to right
    until each holds an expected count of at least `min_expected` (the rest
    joins the last bin), as _chi2_poisson of tests/test_gpu_fast_stream.py pools.
    Returns (statistic, degrees of freedom, p value)."""
    from scipy.stats import chi2
    counts = np.asarray(counts, np.float64)
    exp = np.asarray(pmf, np.float64) * counts.sum()
    obs_b, exp_b = [], []
    o_acc = e_acc = 0.0
    for o, e in zip(counts, exp):
        o_acc += o
        e_acc += e
        if e_acc >= min_expected:
            obs_b.append(o_acc)
            exp_b.append(e_acc)
            o_acc = e_acc = 0.0
    if e_acc > 0 or o_acc > 0:
        obs_b[-1] += o_acc
        exp_b[-1] += e_acc
    obs_b, exp_b = np.array(obs_b), np.array(exp_b)
    stat = float(((obs_b - exp_b) ** 2 / exp_b).sum())
    dof = len(obs_b) - 1
    return stat, dof, float(chi2.sf(stat, dof))
