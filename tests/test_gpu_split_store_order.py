"""The split step kernel's store order (im_split_kernel): its dynamics wave
issues the state stores (the Rring rows, the action_log row with its int64 side
ring, I, B, both flags) as soon as the integer dynamics are done, in front of
the tile barrier, and the reward after them.  That is only right while
  - no window row whose value is used is the action_log slot being written,
    also when the straight-line loads past the last logged row fall on it;
  - the Rring slot of a stage is read (arrival) before it is rewritten (R[t]);
  - padded lanes store nothing in front of the barrier either.

Everything goes through the C ABI (the env classes) and is bit-exact: obs,
reward, both flags, the final get_state blob.  The references are the C oracle
on the same seeds wherever it supports the configuration, and a second handle
created with INVSIM_IM_SPLIT=0 (the one-wave kernel, whose stores follow its
tile store).  Every case crosses two NEXT_STEP episode boundaries, the first
step after each reset step included.

The host launches the early-order instantiation only above
IM_EARLY_STORES_MIN_N = 32 768 envs (invmgmt.hip), so every case runs twice: at its small shape (the order
behind the tile copy, with the same row arithmetic) and with 32 768 envs
added, which keeps the partial last groups and puts every workgroup on the
early order.
"""
import numpy as np
import pytest

from test_gpu_parity import _eq_bits
from test_gpu_split_hotargs import _Oracle, _acts, _drive, _lock_step, _np, _pair

gpu_test = pytest.mark.gpu

I64_MAX, I64_MIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min
C3 = [100, 200, 230]
EARLY = 32768   # IM_EARLY_STORES_MIN_N: more envs than this take the early order
both_orders = pytest.mark.parametrize("base", [0, EARLY], ids=["late", "early"])


def _start(envs, orc, seed):
    for env in envs:
        obs, _ = env.reset(seed=seed)
        if orc:
            assert _eq_bits(_np(obs), orc.obs0)


def _two_boundaries(T):
    """calls that cross two NEXT_STEP boundaries: two episodes of T steps, their
    reset steps, and two steps of the third episode"""
    return 2 * (T + 1) + 2


@gpu_test
@both_orders
@pytest.mark.parametrize("cls_name", ["InvManagementBacklogEnv", "InvManagementLostSalesEnv"])
@pytest.mark.parametrize("L", [(1, 0, 1), (2, 1, 0)], ids=["lt_max1", "lt_max2"])
def test_ring_rows(gpu, oracle, monkeypatch, cls_name, L, base):
    """Lead time 1: the stage's one ring row is this launch's arrival and is
    rewritten in the same launch.  Lead time 0: no ring store, R feeds the
    inventory directly.  lt_max = 1: the window has no logged row, and the
    window wave's clamped row load is the very slot the early action_log store
    writes; lt_max = 2: the one logged row is its neighbour."""
    import invsim
    n, seed, T = base + 130, 41, 7
    kw = dict(L=L, periods=T, dist_param={"mu": 9})
    envs = _pair(monkeypatch, lambda: getattr(invsim, cls_name)(n, device=gpu, **kw))
    orc = _Oracle(oracle, n, seed, backlog=cls_name.endswith("BacklogEnv"), **kw)
    _start(envs, orc, seed)
    _drive(envs, _acts(11, _two_boundaries(T), n, 3, C3), orc)


@gpu_test
@both_orders
@pytest.mark.parametrize("n", [1, 65, 197])
def test_partial_groups(gpu, oracle, monkeypatch, n, base):
    """the default chain with one env (63 padded lanes), a second group of one
    env, and four groups with a partial last one: `valid` in front of the barrier"""
    import invsim
    seed = 300 + n
    n += base
    envs = _pair(monkeypatch, lambda: invsim.InvManagementBacklogEnv(n, device=gpu))
    orc = _Oracle(oracle, n, seed)
    _start(envs, orc, seed)
    _drive(envs, _acts(12, _two_boundaries(orc.T), n, 3, C3), orc)


WIDE = np.array([2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32, 2 ** 53 + 1, I64_MAX, -1, -(2 ** 40), I64_MIN], np.int64)

_M1_2 = dict(I0=(100, 150), p=20, r=(15, 10, 7), k=(0.1, 0.075, 0.05), h=(0.15, 0.1), c=(100, 90), L=(3, 9))


def _wide_acts(seed, K, n, m1, c):
    """ordinary orders with every wide value in every call: call k puts WIDE[j]
    into stage (k + j) % m1 of env (5 k + 17 j) % n (so each ring slot, each
    window row and each stage sees wide entries), and a random 10 % on top"""
    a = _acts(seed, K, n, m1, c)
    rng = np.random.default_rng(seed + 1)
    m = rng.random(a.shape) < 0.1
    a[m] = WIDE[rng.integers(0, len(WIDE), size=int(m.sum()))]
    for k in range(K):
        for j, v in enumerate(WIDE):
            a[k, (5 * k + 17 * j) % n, (k + j) % m1] = v
    return a


@gpu_test
@both_orders
@pytest.mark.parametrize("cls_name", ["InvManagementBacklogEnv", "InvManagementLostSalesEnv"])
@pytest.mark.parametrize("kw", [dict(), _M1_2], ids=["packed_m1_3", "unpacked_m1_2"])
def test_wide_actions(gpu, oracle, monkeypatch, cls_name, kw, base):
    """Orders around the 32-bit ring's sentinel, past 2^53, INT64_MAX and
    negative ones, in every call: a wide entry goes to the int64 side ring in
    front of the barrier, and over the next lt_max calls it moves through the
    window rows of both waves (rows 0-5 the window wave's, 6-8 the dynamics
    wave's), each of which reads it back from the side ring.  Three stages
    (M1 = 3) use the packed ImHot word, two (M1 = 2, lt_max = 9) derive
    everything from ImParams."""
    import invsim
    n, seed, T = base + 130, 57, 12
    kw = dict(kw, periods=T)
    c = list(kw.get("c", C3))
    envs = _pair(monkeypatch, lambda: getattr(invsim, cls_name)(n, device=gpu, **kw))
    orc = _Oracle(oracle, n, seed, backlog=cls_name.endswith("BacklogEnv"), **kw)
    _start(envs, orc, seed)
    _drive(envs, _wide_acts(13, _two_boundaries(T), n, len(c), c), orc)


@gpu_test
@both_orders
@pytest.mark.parametrize("cls_name", ["InvManagementBacklogEnv", "InvManagementLostSalesEnv"])
def test_inline_draw_variant(gpu, oracle, monkeypatch, cls_name, base):
    """The !AHEAD instantiation (d comes through the first barrier; it keeps the
    late order at every size) next to the early-order lookahead steps that
    follow it: the first split step after a seed, after a three-row rollout
    (calls 4-6) and after an unmasked reset; two episode boundaries after the
    reset."""
    import invsim
    n, seed, T = base + 130, 63, 12
    kw = dict(periods=T)
    envs = _pair(monkeypatch, lambda: getattr(invsim, cls_name)(n, device=gpu, **kw))
    orc = _Oracle(oracle, n, seed, backlog=cls_name.endswith("BacklogEnv"), **kw)
    _start(envs, orc, seed)
    acts = _acts(14, 10 + _two_boundaries(T), n, 3, C3)
    _drive(envs, acts[:10], orc, rollout_at=4)
    e_obs = orc.reset()
    for env in envs:
        obs, _ = env.reset()
        assert _lock_step(env)
        assert _eq_bits(_np(obs), e_obs), "obs of the unmasked reset"
    _drive(envs, acts[10:], orc)


@gpu_test
@both_orders
def test_philox_stream(gpu, monkeypatch, base):
    """the fast stream's instantiations (invmgmt_ph.hip) with wide orders; the
    oracle has no Philox stream, so the one-wave kernel is the reference"""
    import invsim
    n, T = base + 130, 12
    envs = _pair(monkeypatch, lambda: invsim.InvManagementBacklogEnv(n, device=gpu, demand_stream="philox",
                                                                     periods=T))
    _start(envs, None, 5)
    _drive(envs, _wide_acts(15, _two_boundaries(T), n, 3, C3))
