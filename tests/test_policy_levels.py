"""CPU: the numpy model of the LEVELS action rule (tests/levels_model.py) against
the oracle's BaseStockAgent with an array safety factor, the model's own edge
cases, and the new symbol's declaration and export."""
import os
import re

import numpy as np

import agents
import levels_model
from conftest import ROOT

L = np.array([1, 5, 10], np.int64)
C = np.array([100, 200, 230], np.int64)


def _obs_and_log(rng, n, t, L, hi=260):
    """A period-t observation and the action_log it shows: I[t] random (negative
    too, as the reference's supplier quirk allows), requested orders in [0, hi)."""
    M1, D = len(L), int(L.max())
    log = rng.integers(0, hi, size=(t, n, M1)).astype(np.int64)
    obs = np.zeros((n, M1 * (D + 1)), np.int64)
    obs[:, :M1] = rng.integers(-300, 900, size=(n, M1))
    k = min(t, D)
    if k:
        obs[:, M1:M1 + k * M1] = log[t - k:].transpose(1, 0, 2).reshape(n, k * M1)
    return obs, log


def test_model_equals_base_stock_with_array_safety_factor():
    rng = np.random.default_rng(5)
    n, mu = 64, 20
    for Lv in (L, np.array([0, 3], np.int64), np.array([2], np.int64)):
        cv = C[:len(Lv)]
        for t in (0, 1, 2, 4, 5, 6, 9, 10, 11, 29):
            obs, log = _obs_and_log(rng, n, t, Lv)
            sf = rng.uniform(0.2, 2.5, size=(n, len(Lv)))
            exp = agents.base_stock(obs, t, log, Lv, mu, sf, cv)
            got = levels_model.action(obs, t, Lv, cv, (Lv + 1) * mu * sf)
            assert np.array_equal(got, exp), (Lv.tolist(), t)
    # per-env periods: every env at its own t
    ts = rng.integers(0, 30, size=n)
    rows, exps = [], []
    for e, t in enumerate(ts):
        obs, log = _obs_and_log(rng, 1, int(t), L)
        rows.append(obs[0])
        exps.append(agents.base_stock(obs, int(t), log, L, mu, 1.37, C)[0])
    got = levels_model.action(np.stack(rows), ts, L, C, (L + 1) * mu * 1.37)
    assert np.array_equal(got, np.stack(exps))


def test_model_edge_levels():
    obs = np.zeros((6, 33), np.int64)
    obs[:, :3] = [40, 50, 60]
    lv = np.array([[0.0, -5.0, 1e12], [np.inf, np.nan, 60.5], [-np.inf, 61.0, 59.0],
                   [40.0, 50.0, 60.0], [41.9, 250.0, 290.0], [141.0, 250.5, 291.0]])
    got = levels_model.action(obs, 0, L, C, lv)
    exp = np.array([[0, 0, 230], [100, 0, 0], [0, 11, 0], [0, 0, 0], [1, 200, 230], [100, 200, 230]])
    assert np.array_equal(got, exp)


def test_model_reorder_points():
    obs = np.zeros((5, 33), np.int64)
    obs[:, :3] = [40, 50, 60]
    lv = np.full((5, 3), 100.0)
    ro = np.array([[40.0, 50.0, 60.0],            # pos == s: the strict < does not order
                   [40.5, 50.5, 60.5],            # just above: orders
                   [np.inf, -np.inf, np.nan],
                   [41.0, 0.0, 1e300],
                   [np.nan, np.inf, -1.0]])
    got = levels_model.action(obs, 0, L, C, lv, ro)
    exp = np.array([[0, 0, 0], [60, 50, 40], [60, 0, 0], [60, 0, 40], [0, 50, 0]])
    assert np.array_equal(got, exp)
    assert np.array_equal(levels_model.action(obs, 0, L, C, lv, np.inf), levels_model.action(obs, 0, L, C, lv))


def test_model_position_wraps_and_windows():
    # t = 3 < L_1: only three orders exist; stage 0 takes the newest one
    obs = np.zeros((1, 33), np.int64)
    obs[0, :3] = [10, 20, 30]
    obs[0, 3:12] = [1, 2, 3, 4, 5, 6, 7, 8, 9]      # periods 0, 1, 2
    assert levels_model.position(obs, 3, L).tolist() == [[10 + 7, 20 + 2 + 5 + 8, 30 + 3 + 6 + 9]]
    obs[0, 0] = np.iinfo(np.int64).max
    assert levels_model.position(obs, 3, L)[0, 0] == np.iinfo(np.int64).min + 6


def test_symbol_is_declared_and_exported():
    from invsim import _capi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "invsim.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+invsim_set_policy_levels\s*\(", src)
    assert re.search(r"#define\s+INVSIM_POLICY_LEVELS\s+7\b", src)
    assert "invsim_set_policy_levels" in _capi.EXPORTS
    assert _capi.POLICY_KINDS["levels"] == 7
    lib = _capi.load_library()
    assert hasattr(lib, "invsim_set_policy_levels")
    assert lib.invsim_abi_version() == 4 == _capi.ABI_VERSION
