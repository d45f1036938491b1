"""CPU: the numpy model of the in-kernel RandomAgent (tests/random_agent_model.py)
against numpy's own Generator.uniform, and the RandomAgent surface that needs
no GPU.  The device side is tests/test_gpu_random_agent.py."""
import numpy as np
import pytest

import random_agent_model as model

HIGH_I64 = np.array([100, 200, 230], np.int64)             # InvMgmt supply_capacity
HIGH_F32 = np.array([2000.0, 0.1, 1234.5678, 3.0e7], np.float32)


@pytest.mark.parametrize("high,dtype", [(HIGH_I64, np.int64), (HIGH_F32, np.float32)])
def test_model_formula_is_generator_uniform(high, dtype):
    """scale(random()) is Generator.uniform(0, high) (f32) / floor(uniform(0, high + 1))
    (int64) bit for bit, with the same final generator state."""
    K, A = 37, len(high)
    for g in (0, 1, 77):
        a = model.generator(5, g)
        b = model.generator(5, g)
        got = model.scale(a.random(K * A).reshape(K, A), high, dtype)
        if dtype is np.int64:
            exp = np.floor(b.uniform(low=0, high=(high + 1).astype(np.float64), size=(K, A))).astype(np.int64)
        else:
            exp = b.uniform(low=0, high=high.astype(np.float64), size=(K, A)).astype(np.float32)
        assert got.dtype == exp.dtype and np.array_equal(got, exp)
        assert a.bit_generator.state == b.bit_generator.state


@pytest.mark.parametrize("high,dtype", [(HIGH_I64, np.int64), (HIGH_F32, np.float32)])
def test_expected_actions_bounds_streams_and_states(high, dtype):
    acts, st = model.expected_actions(9, 64, 6, 50, high, dtype)
    assert acts.shape == (50, 6, len(high)) and st.shape == (4, 6) and st.dtype == np.uint64
    assert (acts >= 0).all() and (acts <= high).all()
    if dtype is np.int64:
        assert acts[..., 0].max() > 90 and acts[..., 0].min() < 10       # the whole range, high included
    assert (st[3] & np.uint64(1)).all()                                  # PCG64 increments are odd
    # env g of seed s is env g - 1 of seed s + 1, and a later launch continues the stream
    b, _ = model.expected_actions(10, 63, 6, 50, high, dtype)
    assert np.array_equal(acts, b)
    head, _ = model.expected_actions(9, 64, 6, 20, high, dtype)
    tail, st2 = model.expected_actions(9, 64, 6, 30, high, dtype, skip=20)
    assert np.array_equal(np.concatenate([head, tail]), acts) and np.array_equal(st, st2)
    # not the demand generator's stream of reset(seed=9): that one is SeedSequence(9 + g)
    dem = np.random.Generator(np.random.PCG64(np.random.SeedSequence(9 + 64))).random(3)
    assert not np.array_equal(model.generator(9, 64).random(3), dem)


def test_random_agent_surface():
    import invsim
    from invsim import policies
    ag = invsim.RandomAgent(seed=5)
    assert ag.name == "Random" and ag.seed == 5
    free = invsim.RandomAgent()
    assert 0 <= free.seed < 2**63 and free.seed != invsim.RandomAgent().seed
    assert "RandomAgent" in invsim.__all__ and policies.RandomAgent is invsim.RandomAgent
    # seed=None under more than one rank: refused before any collective
    with pytest.raises(ValueError, match="same seed"):
        policies._require_agreed_seed(None, 2)
    policies._require_agreed_seed(None, 1)
    policies._require_agreed_seed(3, 8)


def test_policy_kind_matches_header():
    import os
    import re
    from conftest import ROOT
    from invsim import _capi
    src = open(os.path.join(ROOT, "include", "invsim.h")).read()
    assert int(re.search(r"#define INVSIM_POLICY_RANDOM (\d+)", src).group(1)) == _capi.POLICY_KINDS["random"] == 6
    assert int(re.search(r"#define INVSIM_ABI_VERSION (\d+)", src).group(1)) == 4
