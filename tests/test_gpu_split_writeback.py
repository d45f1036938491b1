"""The split step kernel's early order (im_split_kernel, EARLY) streams its
state stores: the dynamics wave's ring rows, action_log row, I and B, and the
lookahead workgroups' rows of the next slot, leave as non-temporal stores; the
action_log row of an env is one store of the whole row, with the int64 side
ring's entries behind it in a guarded block.  The kernel's entry derives the
window depth, first slot, last logged row and the arrival rows in one branch
from the packed ImHot word and in another from ImParams.

What that must not change, checked here:
  - another kernel reads the streamed state in the very next launch (get_state
    and its commit kernel, the fused rollout, the reset step's im_run_kernel,
    set_state);
  - the whole-row store at 3 stages (12 B), 2 (8 B) and 4 (16 B), with wide
    entries in each column, in all and in none, in neighbouring lanes, and at
    lt_max = 1, where the window wave's clamped load falls on the row written;
  - both derivations at the early size, the inline-draw step (first after a
    seed) in front of the lookahead steps;
  - nothing is stored for the padded lanes of a partial last group;
  - the Philox stream's instantiations.

Everything goes through the C ABI (the env classes) and is bit-exact: obs,
reward, both flags, the final get_state blob.  The references are the C oracle
on the same seeds wherever it supports the configuration, and a second handle
created with INVSIM_IM_SPLIT=0 (the one-wave kernel).  The host launches the
early order only above IM_EARLY_STORES_MIN_N = 32 768 envs (invmgmt.hip), so
the shapes are 32 768 + 197 envs (a partial last step group and a partial last
lookahead workgroup), 7 periods, two NEXT_STEP boundaries.
"""
import numpy as np
import pytest
import torch

from test_gpu_parity import _eq_bits
from test_gpu_split_hotargs import _Oracle, _acts, _drive, _lock_step, _np, _pair, _same
from test_gpu_split_store_order import C3, EARLY, I64_MAX, _M1_2, _start, _two_boundaries, _wide_acts

gpu_test = pytest.mark.gpu

N = EARLY + 197
T = 7


def _steps(envs, acts, orc):
    """_drive without the get_state at its end: whatever follows is the launch
    right behind the last early step"""
    dev = torch.from_numpy(acts).to(envs[0].device)
    for k in range(acts.shape[0]):
        assert all(_lock_step(env) for env in envs), f"lock-step before call {k}"
        outs = [tuple(x.clone() for x in env.step(dev[k])[:4]) for env in envs]
        for other in outs[1:]:
            _same(outs[0], other, f"step {k}")
        if orc:
            orc.check(outs[0], acts[k], f"step {k}")


def _rollout(envs, acts, orc, where):
    """one invsim_rollout of len(acts) rows on every handle, each row compared"""
    dev = torch.from_numpy(acts).to(envs[0].device)
    outs = [tuple(x.clone() for x in env.rollout(dev)) for env in envs]
    for j in range(acts.shape[0]):
        rows = [tuple(x[j] for x in o) for o in outs]
        for other in rows[1:]:
            _same(rows[0], other, f"{where} row {j}")
        if orc:
            orc.check(rows[0], acts[j], f"{where} row {j}")


# ---------------------------------------------------------------- 1. the next launch reads the state
@gpu_test
@pytest.mark.parametrize("cls_name", ["InvManagementBacklogEnv", "InvManagementLostSalesEnv"])
def test_get_state_behind_early_steps(gpu, oracle, monkeypatch, cls_name):
    """five early steps, then get_state (the commit kernel reads the lookahead
    slot the last launch streamed, the copy kernels read the rings, I and B)"""
    import invsim
    seed = 71
    envs = _pair(monkeypatch, lambda: getattr(invsim, cls_name)(N, device=gpu, periods=T))
    orc = _Oracle(oracle, N, seed, backlog=cls_name.endswith("BacklogEnv"), periods=T)
    _start(envs, orc, seed)
    _drive(envs, _acts(21, 5, N, 3, C3), orc)


@gpu_test
def test_rollout_behind_early_steps(gpu, oracle, monkeypatch):
    """four early steps, a K = 9 rollout (the fused kernel reads the rings and
    the 32-bit action_log of the launch before it, and crosses a reset step),
    then steps over a second boundary"""
    import invsim
    seed = 72
    envs = _pair(monkeypatch, lambda: invsim.InvManagementBacklogEnv(N, device=gpu, periods=T))
    orc = _Oracle(oracle, N, seed, periods=T)
    _start(envs, orc, seed)
    acts = _acts(22, 4 + 9 + T + 3, N, 3, C3)
    _steps(envs, acts[:4], orc)
    _rollout(envs, acts[4:13], orc, "rollout")
    _drive(envs, acts[13:], orc)


@gpu_test
@pytest.mark.parametrize("cls_name", ["InvManagementBacklogEnv", "InvManagementLostSalesEnv"])
def test_reset_step_between_early_steps(gpu, oracle, monkeypatch, cls_name):
    """two NEXT_STEP boundaries: the reset step (im_run_kernel) runs on the state
    the early step in front of it streamed, and the early steps behind it on its"""
    import invsim
    seed = 73
    envs = _pair(monkeypatch, lambda: getattr(invsim, cls_name)(N, device=gpu, periods=T))
    orc = _Oracle(oracle, N, seed, backlog=cls_name.endswith("BacklogEnv"), periods=T)
    _start(envs, orc, seed)
    _drive(envs, _acts(23, _two_boundaries(T), N, 3, C3), orc)


@gpu_test
def test_set_state_behind_early_steps(gpu, oracle, monkeypatch):
    """early steps, a saved blob, more early steps, then set_state of the blob:
    the steps behind it (per env, the periods come from the blob) equal an
    oracle that replayed the calls up to the blob; an unmasked reset brings the
    early order back"""
    import invsim
    seed = 74
    envs = _pair(monkeypatch, lambda: invsim.InvManagementBacklogEnv(N, device=gpu, periods=T))
    orc = _Oracle(oracle, N, seed, periods=T)
    _start(envs, orc, seed)
    acts = _acts(24, 5 + 4 + 4 + 5, N, 3, C3)
    _drive(envs, acts[:5], orc)
    blobs = [env.get_state().clone() for env in envs]
    assert torch.equal(blobs[0], blobs[1])
    _steps(envs, acts[5:9], orc)
    for env, b in zip(envs, blobs):
        env.set_state(b)
        assert not _lock_step(env)
    orc2 = _Oracle(oracle, N, seed, periods=T)
    for k in range(5):
        orc2.row(acts[k])
    _drive(envs, acts[9:13], orc2, state_at=0)
    e_obs = orc2.reset()
    for env in envs:
        obs, _ = env.reset()
        assert _lock_step(env)
        assert _eq_bits(_np(obs), e_obs), "obs of the unmasked reset"
    _drive(envs, acts[13:], orc2)


# ---------------------------------------------------------------- 2. the action_log row as one store
_M1_4 = dict(I0=(100, 100, 150, 150), p=20, r=(15, 12, 10, 8, 6), k=(0.1, 0.08, 0.07, 0.06, 0.05),
             h=(0.15, 0.12, 0.1, 0.08), c=(100, 90, 80, 70), L=(3, 5, 2, 4))
WIDE_POS = np.array([2 ** 32 - 1, 2 ** 32, 2 ** 53 + 1, I64_MAX], np.int64)


def _column_acts(seed, K, n, m1, c):
    """ordinary orders, and in call k env e gets wide entries (>= 2^32 - 1) by
    (e + k) % 5: none, the first column, the middle one, the last, all columns --
    so neighbouring lanes of a wave differ, and every env sees every pattern"""
    a = _acts(seed, K, n, m1, c)
    e = np.arange(n)
    for k in range(K):
        pat = (e + k) % 5
        val = WIDE_POS[(e // 5 + k) % len(WIDE_POS)]
        for p, cols in ((1, [0]), (2, [m1 // 2]), (3, [m1 - 1]), (4, list(range(m1)))):
            m = pat == p
            for col in cols:
                a[k, m, col] = val[m]
    return a


@gpu_test
@pytest.mark.parametrize("kw", [dict(), _M1_2, _M1_4, dict(L=(1, 0, 1), dist_param={"mu": 9})],
                         ids=["m1_3", "m1_2", "m1_4", "lt_max1"])
def test_row_store_wide_columns(gpu, oracle, monkeypatch, kw):
    import invsim
    seed = 75
    kw = dict(kw, periods=T)
    c = list(kw.get("c", C3))
    envs = _pair(monkeypatch, lambda: invsim.InvManagementBacklogEnv(N, device=gpu, **kw))
    orc = _Oracle(oracle, N, seed, **kw)
    _start(envs, orc, seed)
    _drive(envs, _column_acts(25, _two_boundaries(T), N, len(c), c), orc)


# ---------------------------------------------------------------- 3. both derivations at the early size
@gpu_test
@pytest.mark.parametrize("kw", [
    dict(periods=T),                         # packed
    dict(L=(3, 14, 2), periods=17),          # packed, lt_max = 14: the window does not fit the registers
    dict(L=(1, 5, 16), periods=19),          # not packable (lt_max > 15): everything from ImParams
], ids=["default", "lt14", "lt16"])
def test_entry_paths(gpu, oracle, monkeypatch, kw):
    """the first step after the seed draws inline (MISS, the late order), the
    ones behind it are lookahead steps in the early order"""
    import invsim
    seed = 76
    envs = _pair(monkeypatch, lambda: invsim.InvManagementBacklogEnv(N, device=gpu, **kw))
    orc = _Oracle(oracle, N, seed, **kw)
    _start(envs, orc, seed)
    _drive(envs, _acts(26, _two_boundaries(orc.T), N, 3, C3), orc)


# ---------------------------------------------------------------- 4. padded lanes
class _Guard:
    """env._alloc replaced: every buffer the env hands to the library (obs,
    reward, both flags) is followed by GUARD bytes of a pattern"""
    GUARD, PAT = 4096, 0xA5

    def __init__(self, env):
        self.raw = []

        def alloc(*shape, dtype):
            nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
            raw = torch.full((nbytes + self.GUARD,), self.PAT, dtype=torch.uint8, device=env.device)
            self.raw.append((raw, nbytes))
            return raw[:nbytes].view(dtype).view(*shape)

        env._alloc = alloc

    def check(self, where):
        for raw, nbytes in self.raw:
            assert bool((raw[nbytes:] == self.PAT).all()), f"bytes behind a {nbytes}-byte output {where}"


@gpu_test
@pytest.mark.parametrize("extra", [1, 65])
def test_padded_lanes(gpu, oracle, monkeypatch, extra):
    """a last step group of one env: 63 padded lanes in front of the barrier and
    in the tile copy.  The outputs' bytes behind the last env's rows are
    guarded; the state arrays are the library's (row stride Npad), so for them
    the blob and the next launches' results are the check."""
    import invsim
    n, seed = EARLY + extra, 77 + extra
    envs = _pair(monkeypatch, lambda: invsim.InvManagementBacklogEnv(n, device=gpu, periods=T))
    guards = [_Guard(env) for env in envs]
    orc = _Oracle(oracle, n, seed, periods=T)
    _start(envs, orc, seed)
    _drive(envs, _wide_acts(27, _two_boundaries(T), n, 3, C3), orc)
    torch.cuda.synchronize(gpu)
    for g in guards:
        assert g.raw
        g.check(f"at {n} envs")


# ---------------------------------------------------------------- 5. the fast stream
@gpu_test
def test_philox_stream(gpu, monkeypatch):
    """invmgmt_ph.hip's early instantiations (their lookahead workgroups store
    one row); no oracle for this stream, the one-wave kernel is the reference"""
    import invsim
    envs = _pair(monkeypatch, lambda: invsim.InvManagementBacklogEnv(N, device=gpu, demand_stream="philox",
                                                                     periods=T))
    _start(envs, None, 5)
    _drive(envs, _column_acts(28, _two_boundaries(T), N, 3, C3))
