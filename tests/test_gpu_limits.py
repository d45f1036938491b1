"""GPU: every env family at the ends of the parameter range its create call
accepts (tests/limit_cases.py), bit for bit against the C oracle: observations,
reward bits, both flags, info["demand"] and the final state fields.

The oracle keeps the reference's full history arrays, so it shares no ring
arithmetic with the kernels; tests/test_limit_cases.py holds it to a second
numpy restatement on these very cases, and checks that the Newsvendor and
NetInvMgmt cases reach what they are there for.

130 envs: two full waves and a partial one, a partial second lookahead
workgroup.  The launch paths of a case are pinned through the launch switches
(conftest.knob_envs): the split step and its one-wave twin, the fused rollouts
and the run kernels.
"""
import numpy as np
import pytest
import torch

import agents
import levels_model
import limit_cases as lc
import net_levels_model
import random_agent_model
from conftest import knob_envs

pytestmark = pytest.mark.gpu

ASEED = 77     # RandomAgent(seed=)
SF = 1.1       # BaseStockAgent's safety factor


def _np(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.bool_:
        return a.view(np.uint8)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(got, exp, what):
    """equal bit patterns (exp in got's dtype)"""
    g, e = _np(got), _np(exp)
    g, e = _bits(g), _bits(e.astype(g.dtype))
    assert g.shape == e.shape, f"{what}: {g.shape} vs {e.shape}"
    if not np.array_equal(g, e):
        bad = np.argwhere(g != e)[:4].tolist()
        pytest.fail(f"{what}: {int((g != e).sum())} entries differ, first at {bad}")


def _metrics(env):
    import invsim
    return torch.zeros((env.num_envs, invsim.policies.metrics_dim(env)), dtype=torch.float64, device=env.device)


def _run(env, agent, K):
    met = _metrics(env)
    out = env.rollout_policy(agent, K, obs=True, actions=True, metrics=met)
    out["metrics"] = met
    return out


def _check_row(row, o, r, te, tr, info, what):
    _same(o, row["obs"], f"{what}: obs")
    _same(r, row["reward"], f"{what}: reward bits")
    _same(tr, row["truncated"], f"{what}: truncated")
    assert not bool(torch.as_tensor(te).any()), f"{what}: terminated"
    if info is not None and row["demand"] is not None:
        assert "demand" in info, f"{what}: no demand record"
        _same(info["demand"].reshape(row["demand"].shape), row["demand"], f"{what}: demand")
    if "final_obs" in row:
        _same(info["final_obs"], row["final_obs"], f"{what}: final_obs")
        assert bool(info["_final_obs"].all()), f"{what}: _final_obs"


def _drive(env, plan, acts, rows, what):
    """the call plan on the device env, every call (every rollout row) against its reference row"""
    c = 0
    for kind, k in plan:
        if kind == "step":
            for _ in range(k):
                o, r, te, tr, info = env.step(torch.from_numpy(acts[c]).to(env.device))
                _check_row(rows[c], o, r, te, tr, info, f"{what} call {c} (step)")
                if "reset_obs" in rows[c]:
                    _same(env.reset()[0], rows[c]["reset_obs"], f"{what} call {c}: reset() after the truncation")
                c += 1
        else:
            o, r, te, tr = (x.cpu() for x in env.rollout(torch.from_numpy(acts[c:c + k]).to(env.device)))
            for j in range(k):
                _check_row(rows[c + j], o[j], r[j], te[j], tr[j], None, f"{what} call {c + j} (rollout row {j} of {k})")
            c += k
    assert c == len(rows)


# ------------------------------------------------------------------ InvMgmt
_REF = {}


def _im_ref(oracle, case, stream="numpy", key=None):
    """(reset obs, actions, reference rows) of a case's plan, computed once and shared read-only"""
    key = (case["id"], case["autoreset"], case["plan"], stream) if key is None else key
    if key not in _REF:
        ref = lc.OracleIm(oracle, case, demand_stream=stream)
        obs0 = ref.reset()
        acts = lc.im_actions(case)
        rows = lc.reference_rows(ref, acts, case["autoreset"])
        for row in rows:
            for v in row.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        _REF[key] = (obs0, acts, rows)
    return _REF[key]


def _im_cls(case):
    import invsim
    return invsim.InvManagementBacklogEnv if case["backlog"] else invsim.InvManagementLostSalesEnv


def _im_make(gpu, case, n=None, **kw):
    kw.setdefault("autoreset_mode", case["autoreset"])
    return _im_cls(case)(case["n_envs"] if n is None else n, device=gpu, record_demand=True, **case["kwargs"], **kw)


def _order_log(env, D, m1):
    """The requested-orders ring alog32 [D][Npad][m1] (uint32) out of the state
    blob; state_fields() leaves fields of that layout out."""
    from invsim import _capi
    C = _capi.C
    found, i = {}, 0
    while True:
        name = C.create_string_buffer(32)
        off, eb, rows, stride = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int64()
        if env._lib.invsim_state_field(env._h, i, name, C.byref(off), C.byref(eb), C.byref(rows), C.byref(stride)) != 0:
            break
        found[name.value.decode()] = (off.value, eb.value, rows.value, stride.value)
        i += 1
    off, eb, rows, stride = found["alog32"]
    npad = found["I"][3]
    assert eb == 4 and stride == 0 and rows == D * m1 and npad >= env.num_envs
    raw = env.get_state()[off: off + rows * npad * 4].view(torch.int32).view(D, npad, m1)
    return raw[:, :env.num_envs].cpu().numpy().view(np.uint32)


def _im_final_state(env, case, acts, rows, what):
    """I, B and both rings against the oracle's records of the current episode"""
    ep = []                                   # (record, call) of the episode the plan ends in, oldest first
    for c, r in enumerate(rows):
        if r["reset"]:
            ep = []
            continue
        ep.append((r["info"], c))
        if "final_obs" in r or "reset_obs" in r:
            ep = []
    st = env.state_fields()
    if not ep:                                # the plan ended on a reset: the initial state
        _same(st["I"].t(), np.tile(np.asarray(env.init_inv, np.int64), (env.num_envs, 1)), f"{what}: I after the reset")
        return
    last = ep[-1][0]
    _same(st["I"].t(), last["ending_inventory"], f"{what}: final I")
    if case["backlog"]:
        _same(st["B"].t(), last["backlog_next"], f"{what}: final B")
    # Rring row ring_off[i] + s % L_i holds what stage i + 1 shipped in period s, for the last L_i periods
    t, off = len(ep), 0
    for i, L in enumerate(case["kwargs"]["L"]):
        for s_ in range(max(0, t - L), t):
            _same(st["Rring"][off + s_ % L], ep[s_][0]["sales"][:, i + 1], f"{what}: Rring stage {i} period {s_}")
        off += L
    # alog32 slot s % D holds the orders requested in period s, for the episode's last min(t, D) periods: the
    # observation window.  (Older slots keep earlier episodes' rows by design, masked by the period counter.)
    D, m1 = case["D"], case["m1"]
    if D > 0:
        log = _order_log(env, D, m1)
        for s_ in range(max(0, t - D), t):
            _same(log[s_ % D], np.maximum(acts[ep[s_][1]], 0).astype(np.uint32), f"{what}: alog32 period {s_}")


IM_PLAIN = [c["id"] for c in lc.IM_CASES]


@pytest.mark.parametrize("cid", IM_PLAIN)
def test_invmgmt_step_and_rollout(gpu, oracle, monkeypatch, cid):
    """step() (inline draw, then lookahead hits on im_split_kernel, the reset
    step on im_run_kernel) and rollout() behind it (im_run_kernel STEPS, or the
    fused kernels for the default lead times), on the split handle and its
    one-wave twin (INVSIM_IM_SPLIT=0)."""
    case = lc.IM_BY_ID[cid]
    obs0, acts, rows = _im_ref(oracle, case)
    envs = knob_envs(monkeypatch, "INVSIM_IM_SPLIT", [None, "0"], lambda: _im_make(gpu, case))
    for env, what in zip(envs, ("split", "one-wave")):
        assert env.obs_dim == case["obs_dim"]
        _same(env.reset(seed=case["seed"])[0], obs0, f"{what}: reset obs")
        _drive(env, case["plan"], acts, rows, what)
        _im_final_state(env, case, acts, rows, what)
    assert torch.equal(envs[0].get_state(), envs[1].get_state()), "state blobs of the split handle and its twin"


@pytest.mark.parametrize("cid", ["L255", "od_max_4", "od_max_6", "od_max_9"])
def test_invmgmt_philox(gpu, oracle, cid):
    """one pass per stage count on the fast stream"""
    case = lc.IM_BY_ID[cid]
    obs0, acts, rows = _im_ref(oracle, case, stream="philox")
    env = _im_make(gpu, case, demand_stream="philox")
    _same(env.reset(seed=case["seed"])[0], obs0, "reset obs")
    _drive(env, case["plan"], acts, rows, "philox")
    _im_final_state(env, case, acts, rows, "philox")


def test_invmgmt_same_step_final_obs(gpu, oracle):
    """SAME_STEP autoreset at more than 64 KB of LDS: final_obs is the step's window, obs the reset's"""
    base = lc.IM_BY_ID["above_64k"]
    case = dict(base, autoreset="same_step", plan=(("step", base["kwargs"]["periods"] + 6),))
    obs0, acts, rows = _im_ref(oracle, case)
    assert sum("final_obs" in r for r in rows) == 1
    env = _im_make(gpu, case)
    _same(env.reset(seed=case["seed"])[0], obs0, "reset obs")
    _drive(env, case["plan"], acts, rows, "same_step")
    _im_final_state(env, case, acts, rows, "same_step")


def test_invmgmt_early_instantiation_above_64k(gpu, oracle):
    """32 768 + 197 envs: the EARLY split instantiation with a window that does
    not fit registers and more than 64 KB of LDS; a handful of steps"""
    base = lc.IM_BY_ID["above_64k"]
    n, steps = 32768 + 197, 5
    case = dict(base, n_envs=n, plan=(("step", steps),))
    ref = lc.OracleIm(oracle, case)
    obs0 = ref.reset()
    acts = lc.im_actions(case)
    rows = lc.reference_rows(ref, acts)
    env = _im_make(gpu, case)
    _same(env.reset(seed=case["seed"])[0], obs0, "reset obs")
    _drive(env, case["plan"], acts, rows, "early")
    _im_final_state(env, case, acts, rows, "early")


def _im_oracle(oracle, case):
    ref = lc.OracleIm(oracle, case)
    return ref.orc, ref.reset()


def _closed_loop(orc, obs, K, T, act, reset_rows_record=False, autoreset=True):
    """K policy rows of the oracle from a reset, as rollout_policy writes them:
    act(obs, t, k, log) is the agent's order on the oracle's own observation (log:
    the episode's requested orders so far, [t, n, m1]).  A NEXT_STEP reset row
    has the reset observation, reward 0, no flag, adds nothing to the sums and
    leaves its action row unwritten (zeros), unless the agent records one on
    every launch step (RandomAgent).  Returns (actions, obs, reward, truncated,
    sums [n, 6] as oracle/agents.py run_invmgmt keeps them)."""
    n, m1 = obs.shape[0], orc.m - 1
    A, O, R, TR = np.zeros((K, n, m1), np.int64), [], np.zeros((K, n)), np.zeros((K, n), bool)
    sums, t, log = np.zeros((n, 6)), 0, np.zeros((0, n, m1), np.int64)
    for k in range(K):
        if t == T:
            assert autoreset, "stepping past the horizon"
            if reset_rows_record:
                A[k] = act(obs, t, k, log)
            obs, t, log = orc.reset(), 0, np.zeros((0, n, m1), np.int64)
            O.append(obs)
            continue
        a = act(obs, t, k, log)
        obs, r, tr, info = orc.step(a, info=True)
        log = np.concatenate([log, np.maximum(a, 0)[None]], axis=0)
        sums[:, 0] += r
        sums[:, 1] += 1
        sums[:, 2] += info["demand"]
        sums[:, 3] += info["sales"][:, 0]
        sums[:, 4] += info["unfulfilled"][:, 0]
        sums[:, 5] += np.maximum(0, info["ending_inventory"]).sum(axis=1)
        A[k], R[k], TR[k] = a, r, tr
        O.append(obs)
        t += 1
    return A, np.stack(O), R, TR, sums


def _against(out, exp, what):
    e_act, e_obs, e_rew, e_tr, e_sum = exp
    _same(out["actions"], e_act, f"{what}: actions")
    _same(out["obs"], e_obs, f"{what}: obs")
    _same(out["reward"], e_rew, f"{what}: reward bits")
    _same(out["truncated"], e_tr, f"{what}: truncated")
    _same(out["metrics"], e_sum, f"{what}: metrics bits")
    assert not bool(out["terminated"].any()), f"{what}: terminated"


def _agents(case, env):
    """name -> (the device agent, its numpy rule act(obs, t, k, log), whether it records an action on reset rows)"""
    import invsim
    kw, n = case["kwargs"], case["n_envs"]
    L, c = np.array(kw["L"], np.int64), lc.im_capacity(case)
    rng = np.random.default_rng(case["seed"] + 2)
    lv = rng.uniform(0.0, (L + 1) * 20 * 1.5 + 30 + np.asarray(env.init_inv, np.float64), size=(n, len(L)))
    ro = lv * rng.uniform(0.5, 1.0, size=lv.shape)
    rnd, _ = random_agent_model.expected_actions(ASEED, 0, n, 400, env._action_high(), np.int64)
    const = invsim.ConstantOrderAgent(0.1)
    ca = np.broadcast_to(const.action(env), (n, len(L))).astype(np.int64)
    return {
        "BaseStock": (lambda: invsim.BaseStockAgent(SF), lambda o, t, k, log: agents.base_stock(o, t, log, L, 20, SF, c), False),
        "Levels": (lambda: invsim.LevelsAgent(lv, ro), lambda o, t, k, log: levels_model.action(o, t, L, c, lv, ro), False),
        "Random": (lambda: invsim.RandomAgent(seed=ASEED), lambda o, t, k, log: rnd[k], True),
        "ConstantOrder": (lambda: const, lambda o, t, k, log: ca, False),
    }


AGENT_CASES = [c["id"] for c in lc.IM_CASES if c["autoreset"] == "next_step"]


@pytest.mark.parametrize("cid", AGENT_CASES)
def test_invmgmt_in_kernel_agents(gpu, oracle, cid):
    """Every NEXT_STEP case under each in-kernel agent, from the reset through
    the whole episode, its reset row and three more periods (periods = 1:
    seven rows, every other one a reset row): im_run_kernel's policy
    instantiations, the fused kernels for the default lead times.  The
    BaseStock actions again through rollout_metrics (the EXTERNAL unit) on a
    twin.  The reference is the oracle in closed loop: oracle/agents.py,
    tests/levels_model.py, tests/random_agent_model.py."""
    case = lc.IM_BY_ID[cid]
    T = case["kwargs"]["periods"]
    K = T + 4 if T > 1 else 7
    env, twin = _im_make(gpu, case), _im_make(gpu, case)
    for name, (make, act, rec) in _agents(case, env).items():
        orc, o0 = _im_oracle(oracle, case)
        exp = _closed_loop(orc, o0, K, T, act, rec)
        assert K > T and exp[3][T - 1].all() and not exp[2][T].any(), "the rows cross a reset row"
        _same(env.reset(seed=case["seed"])[0], o0, f"{name}: reset obs")
        out = _run(env, make(), K)
        _against(out, exp, name)
        if name == "Levels" and T > 1:
            assert (exp[0] > 0).mean() > 0.05 and (exp[0] == 0).mean() > 0.05, "the rule orders and holds back"
        if name == "BaseStock":       # ... and its recorded actions through rollout_metrics
            twin.reset(seed=case["seed"])
            met = _metrics(twin)
            rep = twin.rollout_metrics(out["actions"], metrics=met)
            _same(rep["obs"], exp[1], "rollout_metrics: obs"), _same(rep["reward"], exp[2], "rollout_metrics: reward bits")
            _same(rep["truncated"], exp[3], "rollout_metrics: truncated"), _same(met, exp[4], "rollout_metrics: metrics bits")
            assert torch.equal(env.get_state(), twin.get_state()), "state blob after the replay"


def test_invmgmt_in_kernel_agents_disabled_one_period(gpu, oracle):
    """periods = 1 with autoreset off: a policy rollout or rollout_metrics of one
    row is the whole episode, a second row is past the horizon and refused
    before any launch; reset() between the episodes (the second and third unseeded)"""
    case = lc.IM_BY_ID["T1_off"]
    env, twin = _im_make(gpu, case), _im_make(gpu, case)
    for name, (make, act, rec) in _agents(case, env).items():
        orc, o0 = _im_oracle(oracle, case)
        _same(env.reset(seed=case["seed"])[0], o0, f"{name}: reset obs")
        twin.reset(seed=case["seed"])
        agent = make()
        for ep in range(3):
            exp = _closed_loop(orc, o0, 1, 1, lambda o, t, k, log: act(o, t, ep, log), autoreset=False)
            assert exp[3].all()
            out = _run(env, agent, 1)
            _against(out, exp, f"{name} episode {ep}")
            met = _metrics(twin)
            rep = twin.rollout_metrics(out["actions"], metrics=met)
            _same(rep["obs"], exp[1], f"{name} episode {ep}: rollout_metrics obs")
            _same(met, exp[4], f"{name} episode {ep}: rollout_metrics metrics bits")
            with pytest.raises(IndexError, match="horizon"):
                env.rollout_policy(agent, 1)
            o0 = orc.reset()
            _same(env.reset()[0], o0, f"{name}: reset() after episode {ep}")
            twin.reset()
        assert torch.equal(env.get_state(), twin.get_state()), name


def test_invmgmt_in_kernel_agents_refused_under_same_step(gpu):
    """include/invsim.h: policy rollouts and rollout_metrics are unavailable with
    SAME_STEP autoreset, so T1_same has no agent pass: the refusal is the contract"""
    import invsim
    from invsim._capi import InvsimError
    case = lc.IM_BY_ID["T1_same"]
    env = _im_make(gpu, case)
    env.reset(seed=case["seed"])
    with pytest.raises(InvsimError, match=r"\(-22\)"):
        env.rollout_policy(invsim.BaseStockAgent(SF), 1)
    with pytest.raises(InvsimError, match=r"\(-22\)"):
        env.rollout_metrics(torch.zeros((1, case["n_envs"], 3), dtype=torch.int64, device=gpu), metrics=_metrics(env))


def _base_stock_rows(orc, obs, t, log, K, T, L, c):
    """K rows of the oracle under BaseStock from period t (log: the episode's
    requested orders so far), across the NEXT_STEP reset row: (actions, obs,
    reward, truncated, sums) as rollout_policy writes them"""
    n, m1 = obs.shape[0], len(L)
    A, O, R, TR = np.zeros((K, n, m1), np.int64), [], np.zeros((K, n)), np.zeros((K, n), bool)
    sums = np.zeros((n, 6))
    for k in range(K):
        if t == T:
            obs, t, log = orc.reset(), 0, np.zeros((0, n, m1), np.int64)
            O.append(obs)
            continue
        a = agents.base_stock(obs, t, log, L, 20, SF, c)
        obs, r, tr, info = orc.step(a, info=True)
        log = np.concatenate([log, np.maximum(a, 0)[None]], axis=0)
        sums[:, 0] += r
        sums[:, 1] += 1
        sums[:, 2] += info["demand"]
        sums[:, 3] += info["sales"][:, 0]
        sums[:, 4] += info["unfulfilled"][:, 0]
        sums[:, 5] += np.maximum(0, info["ending_inventory"]).sum(axis=1)
        A[k], R[k], TR[k] = a, r, tr
        O.append(obs)
        t += 1
    return A, np.stack(O), R, TR, sums


@pytest.mark.parametrize("n", [130, 256])
@pytest.mark.parametrize("cid", ["T256", "T257"])
def test_invmgmt_fused_rollouts_around_the_alpha_table(gpu, oracle, monkeypatch, cid, n):
    """periods on either side of IM_AP_LDS: rollouts of 30 up to period 240, then
    30 rows across the horizon, open loop and under BaseStock, on the fused
    kernels and their one-wave twins.  256 envs are four groups: the policy
    rollout takes the two-group 3-role launch (T256), 130 the one-group launch."""
    import invsim
    base = lc.IM_BY_ID[cid]
    T = base["kwargs"]["periods"]
    case = dict(base, n_envs=n, plan=(("rollout", 30),) * 9)
    ref = lc.OracleIm(oracle, case)
    obs0 = ref.reset()
    acts = lc.im_actions(case)
    rows = lc.reference_rows(ref, acts)
    assert rows[T]["reset"] and 240 < T < 270
    # the closed loop from period 240 on a second oracle
    pol = lc.OracleIm(oracle, case)
    pol.reset()
    pre = lc.reference_rows(pol, acts[:240])
    L, c = np.array([1, 5, 10], np.int64), lc.im_capacity(case)
    e_act, e_obs, e_rew, e_tr, e_sum = _base_stock_rows(pol.orc, pre[-1]["obs"], 240, np.maximum(acts[:240], 0), 30, T, L, c)
    for var in ("INVSIM_IM_ROLL", "INVSIM_IM_POL_ROLL"):
        envs = knob_envs(monkeypatch, var, [None, "0"], lambda: _im_make(gpu, case))
        for env, what in zip(envs, ("fused", "one-wave")):
            _same(env.reset(seed=case["seed"])[0], obs0, f"{what}: reset obs")
            if var == "INVSIM_IM_ROLL":
                _drive(env, case["plan"], acts, rows, what)
                _im_final_state(env, case, acts, rows, what)
            else:
                _drive(env, case["plan"][:8], acts[:240], rows[:240], what)
                out = _run(env, invsim.BaseStockAgent(SF), 30)
                _same(out["actions"], e_act, f"{what}: BaseStock actions")
                _same(out["obs"], e_obs, f"{what}: BaseStock obs")
                _same(out["reward"], e_rew, f"{what}: BaseStock reward bits")
                _same(out["truncated"], e_tr, f"{what}: BaseStock truncated")
                _same(out["metrics"], e_sum, f"{what}: BaseStock metrics bits")
        assert torch.equal(envs[0].get_state(), envs[1].get_state()), f"{var}: state blobs of the twins"


@pytest.mark.parametrize("cid", ["L255_short", "all_zero_backlog", "all_zero_lost"])
def test_invmgmt_compat_view_histories(gpu, cid):
    """invsim.compat.make: one env through the kernels with record_info, at stage
    counts other than 4; the view's action_log, I and R histories (and D, S, B)
    of one episode against tests/invmgmt_model.py"""
    import invsim.compat
    from invmgmt_model import InvMgmtModel
    case = lc.IM_BY_ID[cid]
    T = case["kwargs"]["periods"]
    view = invsim.compat.make(_im_cls(case).__name__, device=gpu, **case["kwargs"])
    model = InvMgmtModel(case["seed"], backlog=case["backlog"], **case["kwargs"])
    o, _ = view.reset(seed=case["seed"])
    _same(o, model.reset(), "reset obs")
    acts = lc.im_actions(case)[:T, 0]
    for t in range(T):
        o, r, te, tr, info = view.step(acts[t])
        e_o, e_r, e_tr, e_d = model.step(acts[t])
        _same(o, e_o, f"period {t}: obs")
        _same(np.float64(r), np.float64(e_r), f"period {t}: reward bits")
        assert tr == e_tr and not te and info["demand_realized"] == e_d, t
    _same(view.action_log, model.action_log, "action_log")
    _same(view.I, model.I, "I")
    _same(view.R, model.R, "R")
    _same(view.D, model.demand, "D")
    _same(view.B, model.B, "B")
    view.close()


# ------------------------------------------------------------------ Newsvendor
def _nv_case(cid):
    return next(c for c in lc.NV_CASES if c["id"] == cid)


@pytest.mark.parametrize("cid", lc.NV_IDS)
def test_newsvendor_step_and_rollout(gpu, oracle, monkeypatch, cid):
    """the plan with the demand lookahead on and off (INVSIM_NV_AHEAD)"""
    from invsim import NewsvendorEnv
    case = _nv_case(cid)
    ref = lc.OracleNv(oracle, case)
    obs0 = ref.reset()
    acts = lc.nv_actions(case)
    rows = lc.reference_rows(ref, acts)
    envs = knob_envs(monkeypatch, "INVSIM_NV_AHEAD", [None, "0"],
                     lambda: NewsvendorEnv(case["n_envs"], device=gpu, record_demand=True, **case["kwargs"]))
    for env, what in zip(envs, ("lookahead", "no lookahead")):
        _same(env.reset(seed=case["seed"])[0], obs0, f"{what}: reset obs")
        _drive(env, case["plan"], acts, rows, what)
        _same(env.params(), ref.orc.params(), f"{what}: episode params")
    fa, fb = envs[0].state_fields(), envs[1].state_fields()
    for k in ("rng", "params", "pipeline"):
        assert torch.equal(fa[k], fb[k]), k


NV_BIG = dict(lead_time=128, step_limit=300, max_order_quantity=40000, max_inventory=100000)
# name -> (the device agent, agents.run_newsvendor's arguments after max_order)
NV_AGENTS = {
    "order_up_to": (lambda inv: inv.OrderUpToHeuristicAgent(1.2), 1.2, dict(agent="order_up_to")),
    "classic_k_vs_h": (lambda inv: inv.ClassicNewsvendorAgent("k_vs_h", 1.0), 1.0, dict(agent="classic_nv", cr_method="k_vs_h")),
    "classic_profit_margin": (lambda inv: inv.ClassicNewsvendorAgent("profit_margin", 1.1), 1.1,
                              dict(agent="classic_nv", cr_method="profit_margin")),
    "sS": (lambda inv: inv.sSPolicyAgent(0.5, 1.2), 1.2, dict(agent="ss")),
}


@pytest.mark.parametrize("name", list(NV_AGENTS))
def test_newsvendor_policies_at_lead_time_128(gpu, oracle, monkeypatch, name):
    """The Poisson mean of the agents' quantile is mu * 129 * sf: far above the
    lam > 700 switch of nv_poisson_ppf for almost every env.  The order bounds
    are wide, so the quantile itself is the recorded action.  The fused policy
    rollout and its run-kernel twin (INVSIM_NV_POL_ROLL=0)."""
    import invsim
    from invsim import NewsvendorEnv
    n, K, seed = lc.N_ENV, 20, 9800
    make, sf, okw = NV_AGENTS[name]
    orc = oracle.OracleNewsvendor(n, **NV_BIG)
    orc.seed(range(seed, seed + n))
    o0 = orc.reset()
    assert (o0[:, 4] * 129 > 700).mean() > 0.9
    e_act, e_rew, e_obs, e_sum = agents.run_newsvendor(orc, o0, K, 128, sf, NV_BIG["max_order_quantity"], **okw)
    assert (e_act[0] > 700).mean() > 0.8, "the first order is the quantile itself"
    envs = knob_envs(monkeypatch, "INVSIM_NV_POL_ROLL", [None, "0"], lambda: NewsvendorEnv(n, device=gpu, **NV_BIG))
    for env, what in zip(envs, ("fused", "run kernel")):
        _same(env.reset(seed=seed)[0], o0, f"{what}: reset obs")
        out = _run(env, make(invsim), K)
        _same(out["actions"], e_act, f"{what}: actions")
        _same(out["obs"], e_obs, f"{what}: obs")
        _same(out["reward"], e_rew, f"{what}: reward bits")
        _same(out["metrics"], e_sum, f"{what}: metrics bits")
    assert torch.equal(envs[0].get_state(), envs[1].get_state())


def test_newsvendor_policy_rate_bound(gpu, oracle):
    """mu_max * (lead_time + 1) * max(1, sf) <= 1e6: 7751 * 129 = 999 879 runs
    (8 envs, 3 steps, against the oracle), 7752 * 129 = 1 000 008, the smallest
    whole mu_max past it, is refused"""
    import invsim
    from invsim import NewsvendorEnv
    from invsim._capi import INVSIM_ERANGE, InvsimError
    kw = dict(lead_time=128, step_limit=40, max_order_quantity=4e6, max_inventory=1e9)
    n, K, seed = 8, 3, 9900
    orc = oracle.OracleNewsvendor(n, mu_max=7751.0, **kw)
    orc.seed(range(seed, seed + n))
    o0 = orc.reset()
    e_act, e_rew, e_obs, e_sum = agents.run_newsvendor(orc, o0, K, 128, 1.0, kw["max_order_quantity"], agent="classic_nv")
    env = NewsvendorEnv(n, device=gpu, mu_max=7751.0, **kw)
    _same(env.reset(seed=seed)[0], o0, "reset obs")
    out = _run(env, invsim.ClassicNewsvendorAgent("k_vs_h", 1.0), K)
    _same(out["actions"], e_act, "actions"), _same(out["obs"], e_obs, "obs")
    _same(out["reward"], e_rew, "reward bits"), _same(out["metrics"], e_sum, "metrics bits")
    assert float(e_act.max()) > 1e5
    over = NewsvendorEnv(n, device=gpu, mu_max=7752.0, **kw)
    over.reset(seed=seed)
    with pytest.raises(InvsimError, match=rf"\({INVSIM_ERANGE}\)"):
        over.rollout_policy(invsim.ClassicNewsvendorAgent("k_vs_h", 1.0), K)


# ------------------------------------------------------------------ NetInvMgmt
def _net_case(cid):
    return next(c for c in lc.NET_CASES if c["id"] == cid)


def _net_make(gpu, case, **kw):
    import invsim
    return invsim.NetInvMgmtMasterEnv(case["n_envs"], device=gpu, graph=lc.net_graph(case), num_periods=case["num_periods"],
                                      record_demand=True, **kw)


@pytest.mark.parametrize("cid", lc.NET_IDS)
def test_net_step_and_rollout(gpu, oracle, monkeypatch, cid):
    """The series graphs run on the table-walking kernel; the default graph with
    257 periods on the fused rollout and its one-wave twin (INVSIM_NET_ROLL=0)
    across row 256, past the rollout's alpha**t LDS table."""
    case = _net_case(cid)
    ref = lc.OracleNetRef(oracle, case)
    obs0 = ref.reset()
    acts = lc.net_actions(case, ref.orc.act_dim)
    rows = lc.reference_rows(ref, acts)
    last = ref.info
    envs = knob_envs(monkeypatch, "INVSIM_NET_ROLL", [None, "0"], lambda: _net_make(gpu, case))
    for env, what in zip(envs, ("default", "INVSIM_NET_ROLL=0")):
        if case["graph"][0] == "series":
            assert env.kernel_variant == 0
        _same(env.reset(seed=case["seed"])[0], obs0, f"{what}: reset obs")
        _drive(env, case["plan"], acts, rows, what)
        st = env.state_fields()
        _same(st["X"].view(torch.float64).t(), last["X"], f"{what}: final X")
        _same(st["Y"].view(torch.float64).t(), last["Y"], f"{what}: final Y")
    assert torch.equal(envs[0].get_state(), envs[1].get_state())


@pytest.mark.parametrize("cid", ["series1_L255", "series3_L85"])
def test_net_policies_on_the_table_walking_kernel(gpu, oracle, cid):
    """one episode of 300 periods under ConstantOrder and under NetLevelsAgent"""
    import invsim
    case = _net_case(cid)
    n, K = case["n_envs"], case["num_periods"]
    env = _net_make(gpu, case, autoreset_mode="disabled")

    def fresh():
        ref = lc.OracleNetRef(oracle, case)
        return ref.orc

    agent = invsim.ConstantOrderAgent(0.005)
    a = agent.action(env)
    orc = fresh()
    o0 = orc.reset()
    _same(env.reset(seed=case["seed"])[0], o0, "reset obs")
    out = _run(env, agent, K)
    e_rew, e_obs, e_sum = agents.run_net(orc, o0, K, a)
    _same(out["actions"], np.broadcast_to(a, (K, n, len(a))), "ConstantOrder: actions")
    _same(out["obs"], e_obs, "ConstantOrder: obs"), _same(out["reward"], e_rew, "ConstantOrder: reward bits")
    _same(out["metrics"], e_sum, "ConstantOrder: metrics bits")

    orc = fresh()
    high = net_levels_model.action_high(lc.net_graph(case))
    assert np.array_equal(env._action_high(), high)
    lv = np.random.default_rng(case["seed"] + 2).uniform(0.0, 60.0, size=(n, orc.act_dim))
    exp = net_levels_model.ClosedLoop(orc, lv, None, high).run(K)
    env.reset(seed=case["seed"])
    out = _run(env, invsim.NetLevelsAgent(lv), K)
    for k in ("actions", "obs", "reward", "truncated", "metrics"):
        _same(out[k], exp[k], f"NetLevels: {k}")
    inside, zero = net_levels_model.shares(out["actions"].cpu().numpy(), high)
    assert inside >= 0.10 and zero >= 0.05, (inside, zero)
