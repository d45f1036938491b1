"""The case table of the Poisson rate tests: rates whose PTRS table window
(csrc/ptrs_table.hpp rhs_table) starts above k = 0, is cut to its central 512
entries, or does not exist, so that draws leave the table.  Shared by

* tests/test_ptrs_table.py (CPU): the window rule restated here (`window`)
  against the host program tests/ptrs_table_check.cpp, and, over exactly the
  seeds, env counts and call plans of the GPU tests, (a) the restatement of
  numpy's PTRS loop below against numpy and the oracle draw for draw, (b) the
  FLOORS: how many log tests fall inside, below and above each rate's window
  and how many accepted draws lie outside it, (c) the tie margins MARGINS;
* tests/test_gpu_poisson_rates.py: every device path against the oracle.

The tie margin (c).  Inside the window the device reads the host's right-hand
side; outside it (and for every Newsvendor draw, whose log(lam) is the
device's) it evaluates  -lam + k log lam - loggam(k + 1)  with its own f64
log, where the host and numpy use glibc's.  Two logs that are each within
1 ulp of the true value move (x - 0.5) log x (loggam, x = k + 1) and k log lam
by up to 2 * 2^-52 (k + 1) ln(k + 1) each, so a log test of the reference
decides the same way on the device when

    |lhs - rhs| > 8 * 2^-52 * (k + 1) * ln(k + 1)        (DEVICE_BOUND)

(those two terms, times 2).  The 1-ulp figure for the device's f64 log is an
ASSUMPTION: it is what the HIP math API documents for double-precision log,
but no copy of that document was at hand to cite when this was written.  Every
other log test must keep |lhs - rhs| > 1e-12 (TABLE_BOUND).  Each case's seed
base was chosen so that the reference alone satisfies both; MARGINS records the
smallest margins found.
"""
import functools
import math

import numpy as np

N_ENV = 1000                  # a multiple of neither 64 nor 256
RHS_LDS_MAX = 512             # csrc/ptrs_table.hpp
TABLE_MAX_LAM = 1e8           # no table above this rate
TABLE_BOUND = 1e-12
RESET_STREAM = 0xFFFFFFFF     # the fast stream's draw stream of Newsvendor's reset uniforms


def window(lam):
    """(k0, nk) of rhs_table: lam +- 12 sd (-10 / +40), cut to the RHS_LDS_MAX
    entries from floor(lam) - 236 when wider; none below 10 or above 1e8"""
    if not (lam >= 10) or lam > TABLE_MAX_LAM:
        return 0, 0
    sd = math.sqrt(lam)
    k0 = max(0, int(math.floor(lam - 12 * sd - 10)))
    k1 = int(math.ceil(lam + 12 * sd + 40))
    n = k1 - k0
    if n > RHS_LDS_MAX:
        k0 = max(0, int(math.floor(lam)) - RHS_LDS_MAX // 2 + 20)
        n = RHS_LDS_MAX
    return k0, n


# the rates of the host probe, with the windows stated when these tests were specified
PROBE_RATES = [9.99, 10.0, 20.0, 162.6540478400545, 165.0, 166.0, 200.0, 370.0, 371.0, 1000.0, 1e4, 1e6, 1e8, 1.5e8]
STATED_WINDOWS = {166.0: (1, 360), 200.0: (20, 390), 370.0: (129, 512), 371.0: (135, 512), 1000.0: (764, 512),
                  1e4: (9764, 512), 1e8: (99999764, 512), 1.5e8: (0, 0)}


def device_bound(k):
    return 8 * 2.0 ** -52 * (k + 1) * math.log(k + 1)


# ---------------------------------------------------------------- numpy's samplers, restated
CLASSES = ("inside", "below", "above", "accepted_outside")


class Tally:
    """what the log tests and accepted draws of one rate (one market link) did"""

    def __init__(self):
        self.n = dict.fromkeys(CLASSES + ("draws", "candidates", "k_lt_512", "k_ge_512"), 0)
        self.table_margin = math.inf       # min |lhs - rhs| over log tests the device decides from a host table
        self.device_ratio = math.inf       # min |lhs - rhs| / device_bound(k) over those it evaluates itself
        self.rel_margin = math.inf         # min |lhs - rhs| / (|lhs| + |rhs|) over all

    def as_dict(self):
        return dict(self.n, table_margin=self.table_margin, device_ratio=self.device_ratio, rel_margin=self.rel_margin)


def poisson(u, lam, win, tally, loggam, device_loglam=False):
    """numpy's random_poisson (distributions.c) over u() = next_double.  `win`
    is the (k0, nk) of the table the device reads for this rate; with
    device_loglam (Newsvendor: the rate is the episode's, its constants the
    device's own) every log test counts as evaluated on the device."""
    if lam == 0:
        return 0
    tally.n["draws"] += 1
    if lam < 10:
        enlam, X, prod = math.exp(-lam), 0, 1.0
        while True:
            prod *= u()
            if prod > enlam:
                X += 1
            else:
                return X
    slam = math.sqrt(lam)
    loglam = math.log(lam)
    b = 0.931 + 2.53 * slam
    a = -0.059 + 0.02483 * b
    invalpha = 1.1239 + 1.1328 / (b - 3.4)
    vr = 0.9277 - 3.6224 / (b - 2)
    k0, nk = win
    n = tally.n
    while True:
        n["candidates"] += 1
        U = u() - 0.5
        V = u()
        us = 0.5 - abs(U)
        k = int(math.floor((2 * a / us + b) * U + lam + 0.43))
        inside = k0 <= k < k0 + nk
        if us >= 0.07 and V <= vr:
            n["accepted_outside"] += not inside
            return k
        if k < 0 or (us < 0.013 and V > us):
            continue
        lhs = math.log(V) + math.log(invalpha) - math.log(a / (us * us) + b)
        rhs = -lam + k * loglam - loggam(float(k + 1))
        n["inside" if inside else "below" if k < k0 else "above"] += 1
        n["k_lt_512" if k < RHS_LDS_MAX else "k_ge_512"] += 1
        d = abs(lhs - rhs)
        tally.rel_margin = min(tally.rel_margin, d / (abs(lhs) + abs(rhs)))
        if inside and not device_loglam:
            tally.table_margin = min(tally.table_margin, d)
        else:
            tally.device_ratio = min(tally.device_ratio, d / device_bound(k)) if k > 0 else tally.device_ratio
        if device_loglam:                  # Newsvendor: both bounds (the device's bound is below 1e-12 for small k)
            tally.table_margin = min(tally.table_margin, d)
        if lhs <= rhs:
            n["accepted_outside"] += not inside
            return k


class _NumpyUniforms:
    """numpy's own Generator.random() of the env's seed"""

    def __init__(self, seed):
        self.u = np.random.Generator(np.random.PCG64(seed)).random

    def at(self, step, r):
        return self.u


class _PhiloxUniforms:
    """the oracle's fast-stream generator put at (launch step, draw stream) before each draw"""

    def __init__(self, seed):
        import pyoracle
        self.g = pyoracle.PhiloxGen(pyoracle.philox_key(seed))

    def at(self, step, r):
        self.g.set_step(step)
        self.g.sub(r)
        return self.g.next_double


def _uniforms(stream, seed):
    return (_NumpyUniforms if stream == "numpy" else _PhiloxUniforms)(seed)


# ---------------------------------------------------------------- call plans
# InvMgmt and NetInvMgmt: 12 steps (the split step draws the first inline, then
# reads the lookahead slot; call T is the NEXT_STEP reset step), a 23-row
# rollout with two reset rows inside, 8 more steps with a reset step: 43 calls
PHASES = (("steps", 12), ("rollout", 23), ("steps", 8))
IM_T = 9
NET_T = 10
# Newsvendor: lead time 2, step limit 7; steps across two reset steps, an explicit
# reset(), steps, a rollout with resets inside, steps: 42 calls and the reset()
NV_L, NV_T = 2, 7
NV_PHASES = (("steps", NV_T + 6), ("reset", 0), ("steps", 5), ("rollout", 2 * NV_T + 7), ("steps", 3))


def fixed_rate_events(phases, T):
    """per call, in order: its launch step when it draws, None for a NEXT_STEP
    reset call (which owns a launch step on the fast stream and draws nothing)"""
    out, t, s = [], 0, 0
    for _, k in phases:
        for _ in range(k):
            if t == T:
                out.append(None)
                t = 0
            else:
                out.append(s)
                t += 1
            s += 1
    return out


def nv_events(phases, T):
    """("reset" | "draw", launch step) in order, from reset(seed) on: every
    reset (the first, a reset step, an explicit reset()) and every step owns
    one launch step of the fast stream"""
    out, t, s = [("reset", 0)], 0, 1
    for kind, k in phases:
        if kind == "reset":
            out.append(("reset", s))
            t, s = 0, s + 1
            continue
        for _ in range(k):
            if t == T:
                out.append(("reset", s))
                t = 0
            else:
                out.append(("draw", s))
                t += 1
            s += 1
    return out


# ---------------------------------------------------------------- the cases
# family "im": rates = (mu,); "net": one rate per market link in draw order
# (None: a link that draws nothing); "nv": rates = (mu_max,).  `seed`: env i is
# seeded seed + i.  `floors`: per rate, class -> floor (about half the count
# observed over the case's N_ENV envs and call plan; the observed counts are in
# the comments).  A class that is not listed is not targeted by the case.
def _case(fam, stream, rates, seed, floors, **kw):
    return dict(fam=fam, stream=stream, rates=tuple(rates), seed=seed, floors=floors, **kw)


CASES = {
    # ---- InvMgmt, numpy stream.  200 and 371 test the offset (every k inside a window that starts at 20 / 135),
    # 1e4 and 1e8 every class, 1.5e8 and 3e9 have no table (every k is "above" the empty window).
    # Observed counts of (inside, below, above, accepted_outside) in the comments.
    "im_200": _case("im", "numpy", (200.0,), 7000, [dict(inside=6000)],                       # 12019, 0, 0, 0
                    cls="InvManagementBacklogEnv"),
    "im_371": _case("im", "numpy", (371.0,), 7100, [dict(inside=5400)],                       # 10867, 0, 0, 0
                    cls="InvManagementLostSalesEnv"),
    "im_1e4": _case("im", "numpy", (1e4,), 7200,                                              # 5790, 1535, 1013, 420
                    [dict(inside=2900, below=750, above=500, accepted_outside=200)], cls="InvManagementBacklogEnv"),
    "im_1e8": _case("im", "numpy", (1e8,), 7300,                                              # 67, 3901, 3764, 38224
                    [dict(inside=33, below=1950, above=1900, accepted_outside=19000)], cls="InvManagementLostSalesEnv"),
    "im_1.5e8": _case("im", "numpy", (1.5e8,), 7400, [dict(above=3800, accepted_outside=19500)],    # 0, 0, 7695, 39000
                      cls="InvManagementLostSalesEnv"),
    # bound (c) is 1.2e-4 at this rate and about seven of a base's 7 700 log tests miss it: base 1 405 000 is
    # the first of 1 306 tried (100 000, 101 000, ...) whose 1 000 envs all keep it
    "im_3e9": _case("im", "numpy", (3e9,), 1405000, [dict(above=3800, accepted_outside=19500)],     # 0, 0, 7690, 39000
                    cls="InvManagementBacklogEnv"),
    # ---- InvMgmt, fast stream
    "im_371_ph": _case("im", "philox", (371.0,), 7600, [dict(inside=5400)],                   # 10768, 0, 0, 0
                       cls="InvManagementBacklogEnv"),
    "im_1e6_ph": _case("im", "philox", (1e6,), 7700,                                          # 576, 3567, 3582, 30923
                       [dict(inside=290, below=1750, above=1750, accepted_outside=15000)], cls="InvManagementLostSalesEnv"),
    # ---- NetInvMgmt.  The custom graph's three markets get three windows: (0, 114), (50, 430), (9764, 512)
    "net_custom": _case("net", "numpy", (20.0, 250.0, 1e4), 8000,
                        [dict(inside=12000),                                                  # 23890, 0, 0, 0
                         dict(inside=5900),                                                   # 11765, 0, 0, 0
                         dict(inside=2850, below=700, above=550, accepted_outside=230)],      # 5734, 1443, 1109, 467
                        graph="custom"),
    "net_custom_ph": _case("net", "philox", (20.0, 250.0, 1e4), 8100,
                           [dict(inside=12000),                                               # 24042, 0, 0, 0
                            dict(inside=5900),                                                # 11907, 0, 0, 0
                            dict(inside=3000, below=790, above=520, accepted_outside=240)],   # 6027, 1585, 1056, 480
                           graph="custom"),
    "net_default_1e4": _case("net", "numpy", (1e4,), 8200,                                    # 5741, 1541, 1143, 501
                             [dict(inside=2850, below=770, above=570, accepted_outside=250)], graph="default"),
    "net_default_1.5e8": _case("net", "numpy", (1.5e8,), 8300, [dict(above=3900, accepted_outside=20000)],  # 0, 0, 7844, 40000
                               graph="default"),
    # tests/net_graphs.py mixed(): retailer 5's market, a user_D replay (no draw; an empty window between the
    # other two in the table vector), retailer 3's market
    "net_mixed": _case("net", "numpy", (371.0, None, 1e6), 8400,
                       [dict(inside=5400), None,                                              # 10914, 0, 0, 0
                        dict(inside=280, below=1900, above=1800, accepted_outside=15900)],    # 566, 3805, 3621, 31893
                       graph="mixed"),
    # ---- Newsvendor: the rate is the episode's, uniform on [0, mu_max); its table is loggam(k + 1), k < 512.
    # Observed (k_lt_512, k_ge_512, both_envs); both_envs: envs whose own stream has log tests on both sides of 512
    "nv_600": _case("nv", "numpy", (600.0,), 9000, [dict(k_lt_512=5100, k_ge_512=720, both_envs=300)]),     # 10242, 1449, 618
    "nv_3000": _case("nv", "numpy", (3000.0,), 9100, [dict(k_lt_512=1000, k_ge_512=3700, both_envs=310)]),  # 2026, 7467, 628
    "nv_1e6": _case("nv", "numpy", (1e6,), 9200, [dict(k_ge_512=3800)]),                                    # 10, 7611, 4
    "nv_3000_ph": _case("nv", "philox", (3000.0,), 9300, [dict(k_lt_512=1000, k_ge_512=3700, both_envs=300)]),  # 2072, 7522, 615
}

# The smallest margins of every case over its N_ENV envs and whole call plan, as
# tests/test_ptrs_table.py prints them: (min |lhs - rhs| over log tests decided
# from a host table, min |lhs - rhs| / DEVICE_BOUND over those the device
# evaluates itself, min |lhs - rhs| / (|lhs| + |rhs|) over all).  The first must
# stay above TABLE_BOUND, the second above 1.
MARGINS = {
    "im_200": [(1.055e-05, math.inf, 1.389e-06)],
    "im_371": [(3.837e-05, math.inf, 4.479e-06)],
    "im_1e4": [(1.477e-05, 1.746e+07, 1.049e-06)],
    "im_1e8": [(8.981e-05, 2.76, 4.455e-07)],
    "im_1.5e8": [(math.inf, 1.94, 4.706e-07)],
    "im_3e9": [(math.inf, 1.005, 4.106e-06)],
    "im_371_ph": [(1.75e-05, math.inf, 2.213e-06)],
    "im_1e6_ph": [(7.539e-05, 664.6, 1.004e-06)],
    "net_custom": [(3.884e-06, math.inf, 7.087e-07), (1.418e-05, math.inf, 1.603e-06), (3.553e-05, 1.601e+06, 2.715e-06)],
    "net_custom_ph": [(1.95e-05, math.inf, 3.606e-06), (1.069e-05, math.inf, 1.198e-06), (9.449e-06, 1.667e+07, 8.396e-07)],
    "net_default_1e4": [(2.023e-06, 1.263e+06, 1.83e-07)],
    "net_default_1.5e8": [(math.inf, 4.951, 1.158e-06)],
    "net_mixed": [(2.258e-06, math.inf, 2.044e-07), (9.862e-06, 750.8, 6.293e-07)],
    "nv_600": [(6.25e-06, 2.064e+06, 7.25e-07)],
    "nv_3000": [(3.712e-06, 1.575e+05, 3.232e-07)],
    "nv_1e6": [(6.496e-06, 704.7, 4.092e-07)],
    "nv_3000_ph": [(2.608e-05, 1.315e+06, 2.584e-06)],
}


def net_graph(name):
    """(graph, market rates applied) for a NetInvMgmt case"""
    import net_graphs
    from invsim.topology import custom_graph, default_graph
    g = {"custom": custom_graph, "default": default_graph, "mixed": lambda: net_graphs.mixed(net_graphs.by_name, NET_T)}[name]()
    return g


def apply_rates(g, rates):
    """give the graph's drawing market links, in graph.edges() (draw) order, the case's rates"""
    markets = [e for e in g.edges() if "L" not in g.edges[e]]
    assert len(markets) == len(rates), (markets, rates)
    for e, lam in zip(markets, rates):
        if lam is None:
            assert "demand_dist_func" not in g.edges[e]
            continue
        g.edges[e]["demand_dist_func"] = "poisson"
        g.edges[e]["dist_param"] = {"lam": lam}
    return g


@functools.lru_cache(maxsize=None)
def reference(case_id, n_env=N_ENV):
    """The restatement over a case's envs and call plan, computed once and
    shared (read-only): demands int64 [calls that draw, n_env, links] (for
    Newsvendor also params float64 [resets, n_env] of the episode rates), and
    per link a Tally as a dict."""
    import pyoracle
    loggam = pyoracle.lib().orc_loggam
    c = CASES[case_id]
    fam, rates = c["fam"], c["rates"]
    tallies = [Tally() for _ in rates]
    if fam == "nv":
        ev = nv_events(NV_PHASES, NV_T)
        nd, nr = sum(e[0] == "draw" for e in ev), sum(e[0] == "reset" for e in ev)
        dem, mus = np.zeros((nd, n_env, 1), np.int64), np.zeros((nr, n_env))
        both = 0
        for i in range(n_env):
            src = _uniforms(c["stream"], c["seed"] + i)
            before = dict(tallies[0].n)
            d = r = 0
            mu = None
            for kind, s in ev:
                if kind == "reset":
                    u = src.at(s, RESET_STREAM)
                    for _ in range(4):
                        u()
                    mu = u() * rates[0]
                    mus[r, i] = mu
                    r += 1
                else:
                    dem[d, i, 0] = poisson(src.at(s, 0), mu, (0, RHS_LDS_MAX), tallies[0], loggam, device_loglam=True)
                    d += 1
            both += (tallies[0].n["k_lt_512"] > before["k_lt_512"]) and (tallies[0].n["k_ge_512"] > before["k_ge_512"])
        tallies[0].n["both_envs"] = both
        out = dict(demand=dem, mu=mus)
    else:
        ev = [s for s in fixed_rate_events(PHASES, IM_T if fam == "im" else NET_T) if s is not None]
        wins = [window(lam) if lam is not None else (0, 0) for lam in rates]
        dem = np.zeros((len(ev), n_env, len(rates)), np.int64)
        for i in range(n_env):
            src = _uniforms(c["stream"], c["seed"] + i)
            for d, s in enumerate(ev):
                for q, lam in enumerate(rates):
                    if lam is not None:
                        dem[d, i, q] = poisson(src.at(s, q), lam, wins[q], tallies[q], loggam)
        out = dict(demand=dem)
    for a in out.values():
        a.setflags(write=False)
    out["tallies"] = [t.as_dict() for t in tallies]
    return out
