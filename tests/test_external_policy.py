"""CPU: invsim.policies.convert_actions against the reference wrapper's
post-processing, ``np.clip(raw, low, high).astype(action_space.dtype)``
(SB3 ``predict`` clips an unsquashed policy's actions to the Box bounds, then
benchmark_InvManagementBacklogEnv.py:342 casts), bit for bit on a table of
values, and TorchPolicyAgent's argument checks.  No GPU, no library.
"""
import numpy as np
import pytest
import torch

from invsim.policies import TorchPolicyAgent, convert_actions, rollout_policy

INF = np.inf
# negatives, fractions just under an integer (f32 and f64 neighbours), values at
# and above `high`, both infinities
VALUES = [-INF, -1e30, -250.0, -3.2, -1.0, -0.99999994, -0.5, 0.0, 0.49999997, 0.99999994, 1.0, 1.5,
          1.9999999, 2.0000002, 99.99999, 100.0, 100.00001, 100.5, 199.99998, 200.0, 229.99998, 230.0, 230.5, 250.0,
          1999.9999, 2000.0, 2000.0001, 16777216.0, 3e9, 1e30, INF]


def _table(dtype, A):
    """[len(VALUES), A] with column a rotated by a, so every bound meets every value"""
    v = np.array(VALUES, dtype)
    return np.stack([np.roll(v, a) for a in range(A)], axis=1)


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def _expected(raw, low, high, dtype):
    with np.errstate(invalid="ignore"):
        return np.clip(raw, low, high).astype(dtype)


@pytest.mark.parametrize("raw_dtype", [np.float32, np.float64])
def test_int64_space(raw_dtype):
    """InvMgmt's Box(0, supply_capacity, int64): clip in float64 (numpy promotes
    float32 values with int64 bounds), truncation toward zero"""
    low, high = np.zeros(3, np.int64), np.array([100, 200, 230], np.int64)
    raw = _table(raw_dtype, 3)
    got = convert_actions(torch.from_numpy(raw), low, high, torch.int64)
    exp = _expected(raw, low, high, np.int64)
    assert got.dtype == torch.int64 and np.array_equal(got.numpy(), exp)
    # a window that keeps negatives: truncation toward zero, not floor
    low2 = np.array([-5, -300, -1], np.int64)
    got = convert_actions(torch.from_numpy(raw), torch.from_numpy(low2), torch.from_numpy(high), torch.int64)
    exp = _expected(raw, low2, high, np.int64)
    assert np.array_equal(got.numpy(), exp)
    assert (exp[np.isclose(raw, -3.2)] == -3).any() and (exp[np.isclose(raw, -0.5)] == 0).any()


@pytest.mark.parametrize("raw_dtype", [np.float32, np.float64])
def test_float32_space(raw_dtype):
    """Newsvendor's Box(0, max_order, float32) and a NetInvMgmt-like Box with
    infinite upper bounds, which leave the value alone"""
    raw = _table(raw_dtype, 3)
    for low, high in ((np.zeros(3, np.float32), np.array([2000, 100, 230], np.float32)),
                      (np.zeros(3, np.float32), np.array([INF, 100, INF], np.float32)),
                      (np.array([-INF, 0, -2.5], np.float32), np.array([INF, INF, 1.5], np.float32))):
        got = convert_actions(torch.from_numpy(raw), low, high, torch.float32)
        exp = _expected(raw, low, high, np.float32)
        assert got.dtype == torch.float32 and np.array_equal(_bits(got.numpy()), _bits(exp)), (low, high)
    assert np.isinf(exp[:, 0]).any(), "an inf under an inf bound stays"


def test_nan_rules():
    """int64 spaces: NaN -> 0 (numpy leaves that cast undefined); float spaces: NaN passes"""
    raw = torch.tensor([[float("nan"), 5.7, float("nan")], [3.9, float("nan"), -2.0]], dtype=torch.float32)
    gi = convert_actions(raw, np.zeros(3, np.int64), np.array([100, 200, 230], np.int64), torch.int64)
    assert gi.tolist() == [[0, 5, 0], [3, 0, 0]]
    gf = convert_actions(raw, np.zeros(3, np.float32), np.array([100, INF, 230], np.float32), torch.float32)
    assert torch.isnan(gf).tolist() == torch.isnan(raw).tolist()
    assert gf[0, 1].item() == np.float32(5.7) and gf[1, 2].item() == 0.0


def test_negative_zero_at_a_zero_bound():
    """np.clip's result for -0.0 at a bound of 0 is not specified (its scalar and
    vector paths disagree), so this one input is not compared with numpy: the
    rule here is the bound, +0.0, for a value equal to it"""
    raw = torch.tensor([[-0.0, 0.0, -0.0]], dtype=torch.float32)
    got = convert_actions(raw, np.zeros(3, np.float32), np.array([5, 5, INF], np.float32), torch.float32)
    assert np.array_equal(_bits(got.numpy()), _bits(np.zeros((1, 3), np.float32)))
    got = convert_actions(raw, np.array([-1, -1, -INF], np.float32), np.array([0, 0, 0], np.float32), torch.float32)
    assert np.array_equal(_bits(got.numpy()), _bits(np.zeros((1, 3), np.float32)))
    assert convert_actions(raw, np.zeros(3, np.int64), np.ones(3, np.int64), torch.int64).tolist() == [[0, 0, 0]]


def test_leading_dimensions():
    raw = torch.from_numpy(_table(np.float32, 3)[:30]).reshape(5, 6, 3)
    low, high = np.zeros(3, np.int64), np.array([100, 200, 230], np.int64)
    got = convert_actions(raw, low, high, torch.int64)
    assert got.shape == (5, 6, 3)
    assert np.array_equal(got.numpy(), _expected(raw.numpy(), low, high, np.int64))


def test_torch_policy_agent_arguments():
    ag = TorchPolicyAgent(lambda o: o)
    assert ag.name == "TorchPolicy" and ag.clip is True
    assert TorchPolicyAgent(torch.nn.Linear(3, 2), name="PPO", clip=False).name == "PPO"
    with pytest.raises(TypeError):
        TorchPolicyAgent(3)
    with pytest.raises(TypeError):
        ag.device_spec(None)             # not an in-kernel agent
    with pytest.raises(ValueError, match="obs0"):
        rollout_policy(object(), ag, 5)  # refused before the env is touched
