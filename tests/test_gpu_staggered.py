"""Staggered-period stepping against the cohort oracle (tests/staggered.py),
bit for bit, in all three env families.

After a masked reset or a set_state the host knows no common period, every
launch passes t_u = -1 and the per-env-period instantiations of the one-wave
kernels run (im_run_kernel / nv_run_kernel / net_spec_kernel / net_run_kernel
with TU = false): per-lane alpha_pow[t], user_D[t], ring slots and order pipe,
reset and step lanes side by side in one wave, final_obs rows for a subset of
lanes.  Each case asserts the "period unknown" token of position() after the
first mask, so these are the kernels compared here.

Shape: 197 envs = three full 64-env groups and a last group of 5.  The runs
are staggered.script's: lock-step steps, the mask e % 3 == 0, two steps, the
mask of group 1 entirely plus e % 5 == 1 (or 2), steps through two horizons and
more, the final state, then an unmasked reset and five lock-step rows.
test_staggered_model.py checks the harness and the coverage of these same
scripts without a GPU.

Compared per row: obs (int64 / f32 bits), reward (f64 bits), terminated == 0,
truncated, info["demand"] on the stepped envs (the others keep their record),
SAME_STEP's _final_obs and the final_obs rows under it; at the end the PCG64
states, the period row and Newsvendor's params.
"""
import numpy as np
import pytest
import torch

import staggered
from conftest import knob_envs
from staggered import N

pytestmark = pytest.mark.gpu

UNKNOWN = 0xFFFFFFFF          # invsim_position's low word when the periods differ per env
MODES = ("next_step", "same_step", "disabled")
SEED = 400


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize]) if x.dtype.kind == "f" else x


def _eq(got, exp, what, where, rows=None):
    """bit equality of two arrays (on `rows`); a float mismatch reports max |diff| and still fails"""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape and got.dtype == exp.dtype, f"{what} {where}: {got.dtype}{got.shape} vs {exp.dtype}{exp.shape}"
    if rows is not None:
        got, exp = got[rows], exp[rows]
    if np.array_equal(_bits(got), _bits(exp)):
        return
    bad = np.argwhere(_bits(got) != _bits(exp))[:4].tolist()
    msg = f"{what} {where}: first mismatches at {bad}"
    if got.dtype.kind == "f":
        msg += f", max|diff|={np.nanmax(np.abs(got.astype(np.float64) - exp.astype(np.float64)))}"
    pytest.fail(msg)


def _np(x):
    return x.cpu().numpy()


class _Dev:
    """one device handle and what the previous step() left in its demand record"""

    def __init__(self, env, name):
        self.env, self.name, self.prev_dem = env, name, None


def _check_row(out, row, where):
    obs, rew, term, trunc = out
    d = row.defined
    _eq(_np(obs), row.obs, "obs", where, d)
    _eq(_np(rew), row.reward, "reward", where, d)
    assert not _np(term)[d].any(), f"terminated {where}"
    _eq(_np(trunc), row.truncated, "truncated", where, d)


def _drive(devs, h, events, make=None, agent=None):
    """Apply every op of the script to every handle and compare with the harness."""
    gpu = devs[0].env.device
    masked = False
    for i, (op, arg, exp) in enumerate(events):
        for dv in list(devs):
            env, where = dv.env, f"[{dv.name}] op {i} ({op})"
            if op == "reset":
                obs, mask = exp
                if arg is None:
                    o, _ = env.reset(seed=SEED) if i == 0 else env.reset()
                    assert env.position() & UNKNOWN != UNKNOWN, f"lock-step after an unmasked reset {where}"
                else:
                    o, _ = env.reset(options={"reset_mask": torch.from_numpy(mask).to(gpu)})
                    assert env.position() & UNKNOWN == UNKNOWN, f"per-env periods after a mask {where}"
                    masked = True
                _eq(_np(o), obs, "reset obs", where, mask)
            elif op == "step":
                a = torch.from_numpy(arg).to(gpu)
                if exp.raises:
                    with pytest.raises(IndexError):
                        env.step(a)
                    assert env.status() == 0, f"status word cleared {where}"
                    dv.prev_dem = None
                    continue
                o, r, te, tr, info = env.step(a)
                _check_row((o, r, te, tr), exp, where)
                dem = _np(info["demand"]).reshape(N, -1)
                _eq(dem, exp.demand, "demand", where, exp.stepped)
                if dv.prev_dem is not None:
                    _eq(dem, dv.prev_dem, "demand record of an env that did not step", where, ~exp.stepped)
                dv.prev_dem = dem
                if h.mode == "same_step":
                    _eq(_np(info["_final_obs"]), exp.final_mask, "_final_obs", where)
                    _eq(_np(info["final_obs"]), exp.final_obs, "final_obs", where, exp.final_mask)
            elif op == "rollout":
                out = [_np(x) for x in env.rollout(torch.from_numpy(arg).to(gpu))]
                for k, row in enumerate(exp):
                    _check_row([torch.from_numpy(x[k]) for x in out], row, f"{where} row {k}")
                dv.prev_dem = None
            elif op == "policy":
                rows, met = exp
                m = torch.zeros((N, h.met_dim), dtype=torch.float64, device=gpu)
                out = env.rollout_policy(agent, arg[1], obs=True, actions=True, metrics=m)
                acts = _np(out["actions"])
                for k, row in enumerate(rows):
                    w = f"{where} row {k}"
                    _eq(acts[k], row.actions, "actions", w)
                    _check_row((out["obs"][k], out["reward"][k], out["terminated"][k], out["truncated"][k]), row, w)
                _eq(_np(m), met, "metrics", where)
                steps = sum(r.stepped.astype(np.float64) for r in rows)
                _eq(_np(m)[:, 1], steps, "metrics[:, 1] = stepped rows", where)
                dv.prev_dem = None
            elif op == "state":
                f = env.state_fields()
                _eq(_np(f["rng"]).view(np.uint64).T, h.rng_state(), "PCG64 state", where)
                _eq(_np(f["period"])[0], h.periods(), "period", where)
                if h.family == "nv":
                    _eq(_np(env.params()), h.params(), "params", where)
            elif op == "checkpoint":
                if dv is not devs[0]:
                    continue
                assert masked
                fresh = make()                 # never seeded, never stepped: only the blob positions it
                fresh.set_state(env.get_state().clone())
                assert fresh.position() & UNKNOWN == UNKNOWN
                devs.append(_Dev(fresh, "from checkpoint"))
    return devs


# ---------------------------------------------------------------- InvMgmt
_M1_8 = dict(periods=12, I0=(30, 40, 50, 60, 70, 80, 90, 100), r=(9, 8, 7, 6, 5, 4, 3, 2, 1),
             k=(0.3, 0.2, 0.1, 0.1, 0.05, 0.05, 0.05, 0.02, 0.01), h=(0.2, 0.15, 0.12, 0.1, 0.08, 0.06, 0.04, 0.02),
             c=(60, 70, 80, 90, 100, 110, 120, 130), L=(0, 1, 2, 3, 0, 4, 2, 6), p=11, alpha=0.9,
             dist_param={"mu": 35})
IM_CASES = {
    # periods = 7 < lt_max = 10: the obs window and the rings hold rows of the env's previous episode
    "backlog": dict(periods=7, backlog=True),
    "lostsales": dict(periods=7, backlog=False),
    "m1_8": dict(_M1_8, backlog=True),
    "integers": dict(periods=7, backlog=False, dist=3, dist_param={"low": 0, "high": 40}),   # u32buf is per-env state
    "binomial": dict(periods=7, backlog=True, dist=2, dist_param={"n": 400, "p": 0.05}),
    "user_D": dict(periods=7, backlog=True, dist=5, user_D=[3, 11, 0, 25, 7, 40, 18]),
    "mu4": dict(periods=7, backlog=False, dist_param={"mu": 4}),                            # multiplication sampler
}


def _im_make(gpu, mode, kw):
    import invsim
    kw = dict(kw)
    cls = invsim.InvManagementBacklogEnv if kw.pop("backlog") else invsim.InvManagementLostSalesEnv
    return lambda: cls(N, device=gpu, autoreset_mode=mode, record_demand=True, **kw)


def _variant(mode):
    return "b" if mode == "same_step" else "a"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", list(IM_CASES))
def test_invmgmt(gpu, oracle, case, mode):
    kw = IM_CASES[case]
    h = staggered.make(oracle, "im", SEED, _variant(mode), mode, **kw)
    cap = max(kw.get("c", (100, 200, 230)))
    _drive([_Dev(_im_make(gpu, mode, kw)(), case)], h, staggered.script(h, np.random.default_rng(1), cap=cap))


def test_invmgmt_wide_orders(gpu, oracle):
    """capacity 2^40 and requested orders of 65535, 2^32 - 1, 2^32 and more:
    the int64 side ring of the order log, per-lane slots"""
    kw = dict(periods=7, backlog=True, c=(2 ** 40,) * 3)
    h = staggered.make(oracle, "im", SEED, "b", "next_step", **kw)
    _drive([_Dev(_im_make(gpu, "next_step", kw)(), "wide")], h,
           staggered.script(h, np.random.default_rng(2), wide=True))


# ---------------------------------------------------------------- Newsvendor
NV_CASES = [(5, 200.0, "next_step"), (5, 200.0, "same_step"), (5, 200.0, "disabled"),
            (0, 8.0, "next_step"), (0, 8.0, "same_step"), (0, 8.0, "disabled"),
            (5, 8.0, "next_step"), (0, 200.0, "same_step")]


def _nv_make(gpu, mode, kw):
    import invsim
    return lambda: invsim.NewsvendorEnv(N, device=gpu, autoreset_mode=mode, record_demand=True, **kw)


@pytest.mark.parametrize("L,mu_max,mode", NV_CASES)
def test_newsvendor(gpu, oracle, L, mu_max, mode):
    """mu_max 200: PTRS draws; 8: the multiplication sampler.  A masked reset and
    a reset lane draw five parameters from the env's own stream while the lanes
    beside them draw a demand; DISABLED steps on past step_limit, truncated."""
    kw = dict(lead_time=L, step_limit=7, mu_max=mu_max)
    h = staggered.make(oracle, "nv", SEED, "a" if L else "b", mode, **kw)
    _drive([_Dev(_nv_make(gpu, mode, kw)(), "nv")], h, staggered.script(h, np.random.default_rng(3)))


# ---------------------------------------------------------------- NetInvMgmt
def _graph(name):
    from invsim.topology import custom_graph, default_graph
    if name == "default":
        return default_graph()
    g = custom_graph()
    if name == "samplers":                     # a non-Poisson market: the generic kernel only
        params = {"binomial": {"n": 60, "p": 0.3}, "integers": {"low": 2, "high": 41}, "poisson": {"lam": 20}}
        markets = [e for e in g.edges() if "L" not in g.edges[e]]
        for e, fn in zip(markets, ("integers", "binomial", "poisson")):
            g.edges[e]["dist_param"] = dict(params[fn])
            g.edges[e]["demand_dist_func"] = fn
    return g


def _net_make(gpu, mode, g, T, backlog):
    import invsim
    return lambda: invsim.NetInvMgmtMasterEnv(N, device=gpu, graph=g, num_periods=T, backlog=backlog,
                                              autoreset_mode=mode, record_demand=True)


NET_CASES = [("default", True, 30, "next_step"), ("default", True, 30, "same_step"), ("default", True, 30, "disabled"),
             ("custom", False, 4, "next_step"), ("custom", False, 4, "same_step"), ("custom", False, 4, "disabled"),
             ("default", False, 4, "next_step"), ("custom", True, 30, "same_step")]


@pytest.mark.parametrize("graph,backlog,T,mode", NET_CASES)
def test_net(gpu, oracle, monkeypatch, graph, backlog, T, mode):
    """the compiled kernel of the graph and, on a second handle, the generic
    table-walking kernel, each against the harness; num_periods 4 keeps t < L
    on most links at every step"""
    g = _graph(graph)
    h = staggered.make(oracle, "net", SEED, _variant(mode), mode, graph=g, num_periods=T, backlog=backlog)
    spec, gen = knob_envs(monkeypatch, "INVSIM_NET_GENERIC", (None, "1"), _net_make(gpu, mode, g, T, backlog))
    assert spec.kernel_variant == (1 if graph == "default" else 2) and gen.kernel_variant == 0
    _drive([_Dev(spec, "compiled"), _Dev(gen, "generic")], h, staggered.script(h, np.random.default_rng(4)))


def test_net_market_samplers(gpu, oracle):
    g = _graph("samplers")
    h = staggered.make(oracle, "net", SEED, "a", "next_step", graph=g, num_periods=12, backlog=True)
    env = _net_make(gpu, "next_step", g, 12, True)()
    assert env.kernel_variant == 0
    _drive([_Dev(env, "samplers")], h, staggered.script(h, np.random.default_rng(5)))


# ---------------------------------------------------------------- rollouts, policy rollouts, checkpoints
def _family(gpu, family, mode):
    """(make, oracle kw, agent of the device, the harness's agent tuple given an env)"""
    import invsim
    if family == "im":
        kw = IM_CASES["backlog"]
        return (_im_make(gpu, mode, kw), kw, invsim.BaseStockAgent(1.1),
                lambda e: ("base_stock", 1.1, e.dist_param.get("mu", 10), e.lead_time, e.supply_capacity))
    if family == "nv":
        kw = dict(lead_time=5, step_limit=7)
        return (_nv_make(gpu, mode, kw), kw, invsim.OrderUpToHeuristicAgent(1.2),
                lambda e: ("order_up_to", 1.2, e.lead_time, e.max_order_quantity))
    if family == "nv_classic":                 # its per-episode ppf level is recomputed by a reset lane
        kw = dict(lead_time=5, step_limit=7)
        return (_nv_make(gpu, mode, kw), kw, invsim.ClassicNewsvendorAgent("k_vs_h", 1.1),
                lambda e: ("classic_nv", "k_vs_h", 1.1, e.lead_time, e.max_order_quantity))
    g = _graph("default")
    ag = invsim.ConstantOrderAgent(0.07)
    return (_net_make(gpu, mode, g, 12, True), dict(graph=g, num_periods=12, backlog=True), ag,
            lambda e: ("constant", ag.action(e)))


@pytest.mark.parametrize("family,mode", [(f, m) for f in ("im", "nv", "net") for m in ("next_step", "disabled")]
                         + [("nv_classic", "next_step")])
def test_rollouts_with_mixed_periods(gpu, oracle, family, mode):
    """One rollout of 2 * horizon + 5 rows (every cohort resets inside the launch
    at a row of its own) and one policy rollout (BaseStock / OrderUpTo /
    ConstantOrder, and ClassicNewsvendor for the level it keeps per episode)
    with obs, actions and metrics; metrics[:, 1] counts the
    stepped rows only.  DISABLED InvMgmt / Net: as many rows as the horizon
    leaves."""
    make, kw, agent, tup = _family(gpu, family, mode)
    env = make()
    h = staggered.make(oracle, family[:2] if family != "net" else family, SEED, "b", mode, **kw)
    _drive([_Dev(env, family)], h, staggered.script(h, np.random.default_rng(6), calls=tup(env)), agent=agent)


@pytest.mark.parametrize("family", ["im", "nv", "net"])
def test_entry_by_checkpoint(gpu, oracle, family):
    """get_state() of a staggered handle loaded into a fresh handle of the same
    spec (never stepped: its lookahead cache and lock-step period are stale by
    construction); both continue identically against the harness."""
    make, kw, _, _ = _family(gpu, family, "next_step")
    h = staggered.make(oracle, family, SEED, "a", "next_step", **kw)
    devs = _drive([_Dev(make(), family)], h, staggered.script(h, np.random.default_rng(7), checkpoint=True), make=make)
    assert len(devs) == 2


@pytest.mark.parametrize("family", ["im", "net"])
def test_disabled_horizon_fault(gpu, oracle, family):
    """step() with some envs past their horizon (per-env periods, DISABLED)
    raises IndexError and clears the status word; the other envs' steps applied
    and the refused envs' state is untouched: after their masked reset the run
    continues bit-exact for horizon + 2 rows."""
    make, kw, _, _ = _family(gpu, family, "disabled")
    h = staggered.make(oracle, family, SEED, "a", "disabled", **kw)
    events = list(staggered.fault_script(h, np.random.default_rng(8)))
    assert sum(op == "step" and exp.raises for op, _, exp in events) == 1
    h = staggered.make(oracle, family, SEED, "a", "disabled", **kw)
    _drive([_Dev(make(), family)], h, staggered.fault_script(h, np.random.default_rng(8)))
