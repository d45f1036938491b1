"""CPU: the references of tests/test_gpu_limits.py are sound at the parameter
limits (tests/limit_cases.py).

InvMgmt: the C oracle against tests/invmgmt_model.py (plain numpy, full history
arrays, numpy's own Poisson) on a subset of every case's envs, over the case's
whole call plan: observations, reward bits, truncation and demand, the
unseeded later episodes included.

Newsvendor, NetInvMgmt: no second restatement exists, so what is checked is
that the cases REACH what they are there for, over exactly the GPU test's seeds
and actions: the counts in the table are asserted as lower bounds.
"""
import numpy as np
import pytest

import limit_cases as lc


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


@pytest.mark.parametrize("cid", lc.IM_IDS)
def test_oracle_equals_numpy_model(oracle, cid):
    case = lc.IM_BY_ID[cid]
    envs = list(lc.MODEL_ENVS)
    acts = lc.im_actions(case)[:, envs]
    o_ref, m_ref = lc.OracleIm(oracle, case, envs), lc.ModelIm(case, envs)
    assert np.array_equal(o_ref.reset(), m_ref.reset()), "reset obs"
    want = lc.reference_rows(m_ref, acts, case["autoreset"])
    got = lc.reference_rows(o_ref, acts, case["autoreset"])
    assert sum(r["truncated"].all() for r in want) >= 1, "the plan crosses a horizon"
    for c, (g, w) in enumerate(zip(got, want)):
        assert g["reset"] == w["reset"], c
        for k in ("obs", "final_obs", "reset_obs"):
            assert (k in g) == (k in w)
            if k in w:
                assert np.array_equal(g[k], w[k]), f"call {c}: {k}"
        assert np.array_equal(_bits(g["reward"]), _bits(w["reward"])), f"call {c}: reward bits"
        assert np.array_equal(g["truncated"], w["truncated"]), f"call {c}: truncated"
        if not w["reset"]:
            assert np.array_equal(g["demand"], w["demand"]), f"call {c}: demand"


def test_invmgmt_table_is_at_the_limits():
    by = lc.IM_BY_ID
    assert by["L255"]["lds"] == 128 * 1024 + 4096 + 512 and by["L255"]["obs_dim"] == 256
    assert by["above_64k"]["obs_dim"] == 123 and lc.im_lds_bytes(3, 40, split=False) > 64 * 1024 >= lc.im_lds_bytes(3, 39, split=False)
    for m, (L, periods) in lc.OD_MAX.items():
        m1, D, Dr = m - 1, max(L), max(lc.OD_REFUSED[m])
        assert len(L) == m1 == len(lc.OD_REFUSED[m])
        assert m1 * (D + 1) <= lc.OBS_DIM_MAX < m1 * (D + 2), "the largest accepted of this stage count"
        assert Dr == D + 1, "the smallest refused"
        assert lc.im_lds_bytes(m1, D) <= lc.LDS_LIMIT < lc.im_lds_bytes(m1, Dr)
        assert min(L) == 0 and sum(L) > 63 and periods > D
    assert lc.im_lds_bytes(1, lc.OBS_DIM_MAX - 1) == lc.LDS_LIMIT, "obs_dim 311 asks exactly the limit"


@pytest.mark.parametrize("cid", lc.NV_IDS)
def test_newsvendor_reach(oracle, cid):
    case = next(c for c in lc.NV_CASES if c["id"] == cid)
    L, T = case["kwargs"]["lead_time"], case["kwargs"]["step_limit"]
    assert (T - 1) // max(L, 1) >= case["wraps"] if L else True
    ref = lc.OracleNv(oracle, case)
    ref.reset()
    rows = lc.reference_rows(ref, lc.nv_actions(case))
    assert sum(r["truncated"].all() for r in rows) >= 1
    if not case["wraps"]:
        return
    # an order shows as the ring's newest entry (obs[:, 4 + L]) after the step that places it and as its
    # oldest (obs[:, 5]) L - 1 steps later: those at a step >= 2 L were placed after the first lap
    late, t = 0, 0
    hist = []
    for r in rows:
        if r["reset"]:
            t, hist = 0, []
            continue
        hist.append(r["obs"])
        if t >= 2 * L:
            placed, arriving = hist[t - (L - 1)][:, 4 + L], r["obs"][:, 5]
            assert np.array_equal(placed, arriving), t
            late += int((arriving > 0).sum())
        t += 1
    print(f"{cid}: {late} late arrivals")
    assert late >= case["late_arrivals"]


@pytest.mark.parametrize("cid", lc.NET_IDS)
def test_net_reach(oracle, cid):
    """Every link with L > 0 delivers orders placed L periods earlier: its
    pipeline Y falls by exactly that order, and the stock X of the node that
    bought it rises by exactly its arrivals, net of what the node ships and sells
    in the period (distributors; a factory's stock also pays for its production)."""
    case = next(c for c in lc.NET_CASES if c["id"] == cid)
    ref = lc.OracleNetRef(oracle, case)
    ref.reset()
    tb = ref.orc.topo["tables"]
    Ls, pur, sup, rl_node = (np.asarray(tb[k]) for k in ("L", "pur", "sup", "rl_node"))
    E, J, RL = ref.orc.topo["E"], ref.orc.topo["J"], ref.orc.topo["RL"]
    I0 = np.tile(np.asarray(tb["I0"], np.float64)[:J], (case["n_envs"], 1))
    acts = lc.net_actions(case, E)
    count = np.zeros(E, np.int64)
    R, Y, X, t = [], [], [I0], 0
    pending = False
    for a in acts:
        if pending:
            ref.reset()
            R, Y, X, t, pending = [], [], [I0], 0, False
            continue
        _, _, tr, _ = ref.step(a)
        info = ref.info
        R.append(info["R"].copy()), Y.append(info["Y"].copy()), X.append(info["X"].copy())
        inflow = np.zeros_like(I0)
        for e in range(E):
            Le = int(Ls[e])
            if t >= Le:
                inflow[:, pur[e]] += R[t - Le][:, e]
            if Le > 0 and t >= Le and t >= 1:
                due = R[t - Le][:, e]
                # the pipeline of the link loses exactly what was placed L periods ago (and gains this period's order)
                assert np.array_equal(Y[t][:, e] - Y[t - 1][:, e], R[t][:, e] - due), (t, e)
                count[e] += int((due > 0).sum())
        for j in range(J):
            if tb["is_factory"][j]:
                continue
            out = sum(R[t][:, e] for e in range(E) if sup[e] == j) + sum(info["S"][:, r] for r in range(RL) if rl_node[r] == j)
            assert np.allclose(X[t + 1][:, j] - X[t][:, j] + out, inflow[:, j], rtol=0, atol=1e-9), (t, j)
        pending = bool(tr.all())
        t += 1
    lead = [int(c) for e, c in enumerate(count) if Ls[e] > 0]
    print(f"{cid}: deliveries per link with L > 0: {lead}")
    assert min(lead) >= case["deliveries"]


def test_net_series_graphs_fit_the_lds(oracle):
    """net_lds_bytes of the two series graphs (net_graphs.lds_bytes restates it):
    both far inside the 160 KiB, so neither needs a refusal twin"""
    from net_graphs import lds_bytes
    want = {"series1_L255": 70400, "series3_L85": 77056}
    for cid, b in want.items():
        case = next(c for c in lc.NET_CASES if c["id"] == cid)
        tp = lc.OracleNetRef(oracle, case).orc.topo
        assert lds_bytes(tp["J"], tp["E"], tp["RL"], int(np.asarray(tp["tables"]["L"]).sum())) == b <= lc.LDS_LIMIT
